/* mask_host.c -- the privacy masks, the host side: the checked configuration, the table the rule reads, the scalar rule on planes of
 * the visible size, and the element's string form.  Pure integer, no device, no C library beyond malloc / memset / memcpy (the parser reads its numbers
 * itself: no locale). */
#include <stdlib.h>
#include <string.h>

#include "mask_host.h"

int mi355enc_mask_check(const mi355enc_mask_t *cfg) {
    if (!cfg || cfg->n < 0 || cfg->n > MASK_REGIONS_MAX) return MI355ENC_ERR_ARG;
    for (int k = 0; k < cfg->n; k++) {
        const mi355enc_mask_region_t *r = &cfg->region[k];
        if (r->x < -MASK_COORD_MAX || r->x > MASK_COORD_MAX || r->y < -MASK_COORD_MAX || r->y > MASK_COORD_MAX || r->w < 1 || r->w > MASK_COORD_MAX || r->h < 1 ||
            r->h > MASK_COORD_MAX || r->shape < 0 || r->shape > 1 || r->colour > 0xFFFFFFu)
            return MI355ENC_ERR_ARG;
        switch (r->mode) {
        case MASK_MODE_FILL: if (r->param != 0) return MI355ENC_ERR_ARG; break;
        case MASK_MODE_PIXELATE: if (r->param < MASK_CELL_MIN || r->param > MASK_CELL_MAX || (r->param & 1)) return MI355ENC_ERR_ARG; break;
        case MASK_MODE_BLUR: if (r->param < 1 || r->param > MASK_RADIUS_MAX) return MI355ENC_ERR_ARG; break;
        default: return MI355ENC_ERR_ARG;
        }
    }
    return MI355ENC_OK;
}

/* v >> 16 as a floor, whatever the compiler makes of a negative left operand */
static int shr16(int v) { return v >= 0 ? v >> 16 : -((-v + 65535) >> 16); }
static int clip255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
/* v rounded down to even, negative values too */
static int even_floor(int v) { return v >= 0 ? v & ~1 : -((-v + 1) & ~1); }

int mi355enc_mask_colour(unsigned colour, const int32_t coef[10], uint8_t ycc[3]) {
    if (!coef || !ycc || colour > 0xFFFFFFu) return MI355ENC_ERR_ARG;
    const int r = (int)(colour >> 16), g = (int)((colour >> 8) & 255u), b = (int)(colour & 255u);
    ycc[0] = (uint8_t)clip255(shr16(coef[0] * r + coef[1] * g + coef[2] * b + coef[9] * 65536 + 32768));
    ycc[1] = (uint8_t)clip255(shr16(coef[3] * r + coef[4] * g + coef[5] * b + 128 * 65536 + 32768));
    ycc[2] = (uint8_t)clip255(shr16(coef[6] * r + coef[7] * g + coef[8] * b + 128 * 65536 + 32768));
    return MI355ENC_OK;
}

int mask_resolve(const mi355enc_mask_t *cfg, const int32_t coef[10], int vw, int vh, mask_tab_t *tab) {
    if (!tab || !coef || mi355enc_mask_check(cfg) || vw < 2 || vh < 2 || vw > MASK_COORD_MAX || vh > MASK_COORD_MAX || ((vw | vh) & 1)) return MI355ENC_ERR_ARG;
    memset(tab, 0, sizeof *tab);
    tab->n = cfg->n;
    for (int k = 0; k < cfg->n; k++) {
        const mi355enc_mask_region_t *g = &cfg->region[k];
        mask_reg_t *r = &tab->r[k];
        const int x1 = even_floor(g->x + g->w + 1), y1 = even_floor(g->y + g->h + 1);
        r->x0 = even_floor(g->x); r->y0 = even_floor(g->y); r->W2 = x1 - r->x0; r->H2 = y1 - r->y0;
        r->cx0 = r->x0 > 0 ? r->x0 : 0; r->cy0 = r->y0 > 0 ? r->y0 : 0; r->cx1 = x1 < vw ? x1 : vw; r->cy1 = y1 < vh ? y1 : vh;
        r->mode = g->mode; r->param = g->param; r->shape = g->shape;
        uint8_t ycc[3];
        (void)mi355enc_mask_colour(g->colour, coef, ycc);
        r->cy = ycc[0]; r->ccb = ycc[1]; r->ccr = ycc[2];
    }
    return MI355ENC_OK;
}

int mi355enc_mask_ellipse(int W2, int H2, int qx, int qy) {
    if (W2 < 2 || H2 < 2 || W2 > 2 * MASK_COORD_MAX + 2 || H2 > 2 * MASK_COORD_MAX + 2 || ((W2 | H2) & 1) || qx < 0 || qy < 0 || qx >= W2 / 2 || qy >= H2 / 2) return MI355ENC_ERR_ARG;
    mask_reg_t r;
    memset(&r, 0, sizeof r);
    r.W2 = W2; r.H2 = H2; r.cx1 = W2; r.cy1 = H2; r.shape = 1;
    return mask_inside(&r, 2 * qx, 2 * qy);
}

int mi355enc_mask_mean(int sum, int r) {
    if (r < 1 || r > MASK_RADIUS_MAX || sum < 0 || sum > 255 * (2 * r + 1)) return MI355ENC_ERR_ARG;
    return (int)mask_div((uint32_t)(sum + r), mask_recip(2 * r + 1));
}

/* one box pass of rule 6 over a plane of `rows` rows of n elements of `comps` interleaved components each: horizontally (vert 0) or vertically, positions clamped
 * to the plane, from src to dst (both at `stride` bytes a row) */
static void box_pass(const uint8_t *src, uint8_t *dst, int stride, int n, int rows, int comps, int r, int vert) {
    const uint32_t m = mask_recip(2 * r + 1);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < n; x++)
            for (int c = 0; c < comps; c++) {
                uint32_t sum = 0;
                for (int k = -r; k <= r; k++) {
                    int xx = vert ? x : x + k, yy = vert ? y + k : y;
                    xx = xx < 0 ? 0 : xx > n - 1 ? n - 1 : xx; yy = yy < 0 ? 0 : yy > rows - 1 ? rows - 1 : yy;
                    sum += src[(size_t)yy * stride + xx * comps + c];
                }
                dst[(size_t)y * stride + x * comps + c] = (uint8_t)mask_div(sum + (uint32_t)r, m);
            }
}

/* the region's result on its clipped rectangle, from the untouched picture sy / suv (w bytes a row): ry cw x ch, ruv cw x ch / 2, both at cw bytes a row; t:
 * scratch of the same two sizes */
static void region_result(const mask_reg_t *r, const uint8_t *sy, const uint8_t *suv, int w, uint8_t *ry, uint8_t *ruv, uint8_t *ty, uint8_t *tuv) {
    const int cw = r->cx1 - r->cx0, ch = r->cy1 - r->cy0;
    if (r->mode == MASK_MODE_BLUR) {
        const int rl = r->param, rc = (r->param + 1) >> 1;
        for (int y = 0; y < ch; y++) memcpy(ry + (size_t)y * cw, sy + (size_t)(r->cy0 + y) * w + r->cx0, (size_t)cw);
        for (int y = 0; y < ch / 2; y++) memcpy(ruv + (size_t)y * cw, suv + (size_t)(r->cy0 / 2 + y) * w + r->cx0, (size_t)cw);
        for (int p = 0; p < 2; p++) {
            box_pass(ry, ty, cw, cw, ch, 1, rl, 0); box_pass(ty, ry, cw, cw, ch, 1, rl, 1);
            box_pass(ruv, tuv, cw, cw / 2, ch / 2, 2, rc, 0); box_pass(tuv, ruv, cw, cw / 2, ch / 2, 2, rc, 1);
        }
        return;
    }
    /* pixelate: the cells tile from (x0, y0); what of a cell lies inside C is what it is the mean of */
    const int c = r->param;
    for (int gy = r->y0; gy < r->cy1; gy += c)
        for (int gx = r->x0; gx < r->cx1; gx += c) {
            const int ax = gx > r->cx0 ? gx : r->cx0, ay = gy > r->cy0 ? gy : r->cy0, bx = gx + c < r->cx1 ? gx + c : r->cx1, by = gy + c < r->cy1 ? gy + c : r->cy1;
            if (ax >= bx || ay >= by) continue;
            uint32_t sl = 0, sb = 0, sr = 0;
            for (int y = ay; y < by; y++) for (int x = ax; x < bx; x++) sl += sy[(size_t)y * w + x];
            for (int y = ay / 2; y < by / 2; y++) for (int x = ax; x < bx; x += 2) { sb += suv[(size_t)y * w + x]; sr += suv[(size_t)y * w + x + 1]; }
            const uint32_t nl = (uint32_t)(bx - ax) * (uint32_t)(by - ay), nc = nl / 4;
            const uint8_t ml = (uint8_t)((sl + nl / 2) / nl), mb = (uint8_t)((sb + nc / 2) / nc), mr = (uint8_t)((sr + nc / 2) / nc);
            for (int y = ay; y < by; y++) memset(ry + (size_t)(y - r->cy0) * cw + (ax - r->cx0), ml, (size_t)(bx - ax));
            for (int y = ay / 2; y < by / 2; y++) for (int x = ax; x < bx; x += 2) { uint8_t *q = ruv + (size_t)(y - r->cy0 / 2) * cw + (x - r->cx0); q[0] = mb; q[1] = mr; }
        }
}

int mi355enc_mask_apply_host(const mi355enc_mask_t *cfg, const int32_t coef[10], int w, int h, uint8_t *y, uint8_t *uv) {
    mask_tab_t t;
    if (!y || !uv || mask_resolve(cfg, coef, w, h, &t)) return MI355ENC_ERR_ARG;
    int any = 0;
    for (int k = 0; k < t.n; k++) any |= !mask_empty(&t.r[k]);
    if (!any) return MI355ENC_OK;
    const size_t ysz = (size_t)w * h, csz = ysz / 2;
    /* rule 3: the picture as it stood, and room for one region's result and scratch (no region is larger than the picture) */
    uint8_t *buf = (uint8_t *)malloc(3 * (ysz + csz));
    if (!buf) return MI355ENC_ERR_NOMEM;
    uint8_t *sy = buf, *suv = sy + ysz, *ry = suv + csz, *ruv = ry + ysz, *ty = ruv + csz, *tuv = ty + ysz;
    memcpy(sy, y, ysz); memcpy(suv, uv, csz);
    for (int k = 0; k < t.n; k++) {
        const mask_reg_t *r = &t.r[k];
        if (mask_empty(r)) continue;
        const int cw = r->cx1 - r->cx0;
        if (r->mode != MASK_MODE_FILL) region_result(r, sy, suv, w, ry, ruv, ty, tuv);
        for (int py = r->cy0; py < r->cy1; py += 2)
            for (int px = r->cx0; px < r->cx1; px += 2) {
                if (!mask_owns(&t, k, px, py)) continue;
                uint8_t *d0 = y + (size_t)py * w + px, *d1 = d0 + w, *dc = uv + (size_t)(py / 2) * w + px;
                if (r->mode == MASK_MODE_FILL) {
                    d0[0] = d0[1] = d1[0] = d1[1] = (uint8_t)r->cy; dc[0] = (uint8_t)r->ccb; dc[1] = (uint8_t)r->ccr;
                } else {
                    const uint8_t *s0 = ry + (size_t)(py - r->cy0) * cw + (px - r->cx0), *sc = ruv + (size_t)((py - r->cy0) / 2) * cw + (px - r->cx0);
                    d0[0] = s0[0]; d0[1] = s0[1]; d1[0] = s0[cw]; d1[1] = s0[cw + 1]; dc[0] = sc[0]; dc[1] = sc[1];
                }
            }
    }
    free(buf);
    return MI355ENC_OK;
}

/* one decimal integer with optional sign between blanks; moves *p behind it.  0: no number there, or beyond +-10^6 */
static int parse_int(const char **p, int *v) {
    const char *s = *p;
    while (*s == ' ' || *s == '\t') s++;
    int neg = 0;
    if (*s == '-' || *s == '+') { neg = *s == '-'; s++; }
    if (*s < '0' || *s > '9') return 0;
    long a = 0;
    for (; *s >= '0' && *s <= '9'; s++) { a = a * 10 + (*s - '0'); if (a > 1000000) return 0; }
    while (*s == ' ' || *s == '\t') s++;
    *v = neg ? -(int)a : (int)a;
    *p = s;
    return 1;
}

int mi355enc_mask_parse(const char *text, unsigned colour, mi355enc_mask_t *cfg) {
    if (!text || !cfg || colour > 0xFFFFFFu) return MI355ENC_ERR_ARG;
    mi355enc_mask_t c;
    memset(&c, 0, sizeof c);
    const char *s = text;
    while (*s == ' ' || *s == '\t') s++;
    while (*s) {
        if (c.n == MASK_REGIONS_MAX) return MI355ENC_ERR_ARG;
        int v[7] = {0, 0, 0, 0, 0, 0, 0}, k = 0;
        for (;;) {
            if (k == 7 || !parse_int(&s, &v[k])) return MI355ENC_ERR_ARG;
            k++;
            if (*s != ',') break;
            s++;
        }
        if (k < 6) return MI355ENC_ERR_ARG;
        mi355enc_mask_region_t *r = &c.region[c.n++];
        r->x = v[0]; r->y = v[1]; r->w = v[2]; r->h = v[3]; r->mode = v[4]; r->param = v[5]; r->shape = v[6]; r->colour = colour;
        if (*s == ';') { s++; if (!*s) return MI355ENC_ERR_ARG; } /* (a separator, not a terminator) */
        else if (*s) return MI355ENC_ERR_ARG;
    }
    if (mi355enc_mask_check(&c)) return MI355ENC_ERR_ARG;
    *cfg = c;
    return MI355ENC_OK;
}
