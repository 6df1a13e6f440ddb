/* roi_host.c -- region-of-interest quantisation, the host side: the checked configuration, the per-macroblock map it stands for,
 * and the element's string form.  Pure integer, no device, no C library beyond memset / memcpy (the parser reads its numbers itself: no locale). */
#include <string.h>

#include "../../include/mi355enc.h"
#include "roi_host.h"

void mi355enc_roi_default(mi355enc_roi_t *cfg) {
    if (cfg) memset(cfg, 0, sizeof *cfg);
}

int mi355enc_roi_check(const mi355enc_roi_t *cfg) {
    if (!cfg || cfg->n_rects < 0 || cfg->n_rects > ROI_RECTS_MAX || cfg->balance < 0 || cfg->balance > ROI_BALANCE_MAX) return MI355ENC_ERR_ARG;
    for (int k = 0; k < cfg->n_rects; k++) {
        const mi355enc_roi_rect_t *r = &cfg->rect[k];
        if (r->x < -ROI_COORD_MAX || r->x > ROI_COORD_MAX || r->y < -ROI_COORD_MAX || r->y > ROI_COORD_MAX || r->w < 1 || r->w > ROI_COORD_MAX ||
            r->h < 1 || r->h > ROI_COORD_MAX || r->delta == 0 || r->delta < -ROI_DELTA_MAX || r->delta > ROI_DELTA_MAX || r->feather < 0 ||
            r->feather > ROI_FEATHER_MAX)
            return MI355ENC_ERR_ARG;
    }
    return MI355ENC_OK;
}

/* v / 16 as a floor, whatever the compiler makes of a negative left operand of >> */
static int mb_of(int v) { return v >= 0 ? v >> 4 : -((-v + 15) >> 4); }

int mi355enc_roi_map(const mi355enc_roi_t *cfg, const int8_t *user, int mbw, int mbh, int8_t *out, int *active, int *background) {
    if (!out || mbw < 1 || mbh < 1 || mbw > 512 || mbh > 512 || (cfg && mi355enc_roi_check(cfg))) return MI355ENC_ERR_ARG;
    const int nmb = mbw * mbh;
    if (user) for (int m = 0; m < nmb; m++) if (user[m] < -ROI_DELTA_MAX || user[m] > ROI_DELTA_MAX) return MI355ENC_ERR_ARG;
    /* the rectangles in macroblocks; one wholly outside the picture contributes nothing */
    int n = 0, x0[ROI_RECTS_MAX], x1[ROI_RECTS_MAX], y0[ROI_RECTS_MAX], y1[ROI_RECTS_MAX], dl[ROI_RECTS_MAX], fe[ROI_RECTS_MAX];
    for (int k = 0; cfg && k < cfg->n_rects; k++) {
        const mi355enc_roi_rect_t *r = &cfg->rect[k];
        if (r->x >= 16 * mbw || r->y >= 16 * mbh || r->x + r->w <= 0 || r->y + r->h <= 0) continue;
        x0[n] = mb_of(r->x); x1[n] = mb_of(r->x + r->w - 1); y0[n] = mb_of(r->y); y1[n] = mb_of(r->y + r->h - 1); dl[n] = r->delta; fe[n] = r->feather;
        n++;
    }
    long S = 0;
    int N0 = 0, any = 0;
    for (int my = 0, m = 0; my < mbh; my++)
        for (int mx = 0; mx < mbw; mx++, m++) {
            int e = 0, p = 0;
            for (int k = 0; k < n; k++) {
                int d = 0;
                if (x0[k] - mx > d) d = x0[k] - mx;
                if (mx - x1[k] > d) d = mx - x1[k];
                if (y0[k] - my > d) d = y0[k] - my;
                if (my - y1[k] > d) d = my - y1[k];
                if (d > fe[k]) continue;
                const int mag = dl[k] < 0 ? -dl[k] : dl[k], c = d == 0 ? mag : mag * (fe[k] + 1 - d) / (fe[k] + 1);
                if (dl[k] < 0) { if (-c < e) e = -c; } else if (c > p) p = c;
            }
            const int t = roi_clip((e < 0 ? e : p) + (user ? user[m] : 0), -ROI_DELTA_MAX, ROI_DELTA_MAX);
            out[m] = (int8_t)t;
            S += t; N0 += t == 0; any |= t != 0;
        }
    /* balance: move bits, do not add them -- what the emphasis takes is spread over the macroblocks nobody spoke for, up to the cap */
    int b = 0;
    if (cfg && cfg->balance > 0 && S < 0 && N0 > 0) {
        const long q = (-S + N0 / 2) / N0;
        b = q < cfg->balance ? (int)q : cfg->balance;
        if (b > 0) for (int m = 0; m < nmb; m++) if (out[m] == 0) out[m] = (int8_t)b;
    }
    if (active) *active = any;
    if (background) *background = b;
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

int mi355enc_roi_parse(const char *text, mi355enc_roi_t *cfg) {
    if (!text || !cfg) return MI355ENC_ERR_ARG;
    mi355enc_roi_t c;
    memset(&c, 0, sizeof c);
    c.balance = cfg->balance; /* (no part of the string: it stays) */
    const char *s = text;
    while (*s == ' ' || *s == '\t') s++;
    while (*s) {
        if (c.n_rects == ROI_RECTS_MAX) return MI355ENC_ERR_ARG;
        int v[6] = {0, 0, 0, 0, 0, 0}, k = 0;
        for (;;) {
            if (k == 6 || !parse_int(&s, &v[k])) return MI355ENC_ERR_ARG;
            k++;
            if (*s != ',') break;
            s++;
        }
        if (k < 5) return MI355ENC_ERR_ARG;
        mi355enc_roi_rect_t *r = &c.rect[c.n_rects++];
        r->x = v[0]; r->y = v[1]; r->w = v[2]; r->h = v[3]; r->delta = v[4]; r->feather = v[5];
        if (*s == ';') { s++; if (!*s) return MI355ENC_ERR_ARG; } /* (a separator, not a terminator) */
        else if (*s) return MI355ENC_ERR_ARG;
    }
    if (c.balance < 0 || c.balance > ROI_BALANCE_MAX) c.balance = 0;
    if (mi355enc_roi_check(&c)) return MI355ENC_ERR_ARG;
    *cfg = c;
    return MI355ENC_OK;
}
