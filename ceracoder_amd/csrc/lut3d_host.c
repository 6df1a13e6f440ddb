/* lut3d_host.c -- the host side of the 3D colour LUT step: the coefficients, the table's check and identity, the .cube parser and the
 * rule on host planes.  All integers, no device, no locale: the parser reads its numbers itself. */
#include <stddef.h>
#include <string.h>

#include "../../include/mi355enc.h"
#include "lut3d_host.h"

/* floor(n / d + 1 / 2), d > 0 */
static int64_t round_div(int64_t n, int64_t d) {
    const int64_t a = 2 * n + d, b = 2 * d;
    return a >= 0 ? a / b : -((-a + b - 1) / b);
}

int mi355enc_lut3d_coefficients(int matrix, int full_range, int32_t out[LUT3D_COEF_WORDS]) {
    int64_t kr, kb; /* in 1 / 10000 */
    if (!out || (full_range | 1) != 1) return MI355ENC_ERR_ARG;
    switch (matrix) {
    case 1: kr = 2126; kb = 722; break;
    case 5: case 6: kr = 2990; kb = 1140; break;
    case 9: kr = 2627; kb = 593; break;
    default: return MI355ENC_ERR_ARG;
    }
    const int64_t kg = 10000 - kr - kb, ys = full_range ? 255 : 219, cs = full_range ? 255 : 224, Q = (int64_t)1 << 26, F = (int64_t)1 << 20;
    /* Minv = floor(M^-1 * 4096 * 2^14 + 0.5): R' = (Y - yoff) / ys + 2 (1 - kr) (Cr - 128) / cs, B' likewise with kb and Cb, G' what is left */
    out[0] = out[3] = out[6] = (int32_t)round_div(Q, ys);
    out[1] = 0; out[2] = (int32_t)round_div(2 * (10000 - kr) * Q, 10000 * cs);
    out[4] = (int32_t)round_div(-2 * kb * (10000 - kb) * Q, 10000 * kg * cs); out[5] = (int32_t)round_div(-2 * kr * (10000 - kr) * Q, 10000 * kg * cs);
    out[7] = (int32_t)round_div(2 * (10000 - kb) * Q, 10000 * cs); out[8] = 0;
    /* Mf = floor(M / 1023 * 2^20 + 0.5): Y = ys (kr R + kg G + kb B), Cb = cs (B - Y') / (2 (1 - kb)), Cr = cs (R - Y') / (2 (1 - kr)) */
    out[9] = (int32_t)round_div(ys * kr * F, 10000 * 1023); out[10] = (int32_t)round_div(ys * kg * F, 10000 * 1023); out[11] = (int32_t)round_div(ys * kb * F, 10000 * 1023);
    out[12] = (int32_t)round_div(-cs * kr * F, 2 * (10000 - kb) * 1023); out[13] = (int32_t)round_div(-cs * kg * F, 2 * (10000 - kb) * 1023); out[14] = (int32_t)round_div(cs * F, 2 * 1023);
    out[15] = (int32_t)round_div(cs * F, 2 * 1023); out[16] = (int32_t)round_div(-cs * kg * F, 2 * (10000 - kr) * 1023); out[17] = (int32_t)round_div(-cs * kb * F, 2 * (10000 - kr) * 1023);
    out[18] = full_range ? 0 : 16;
    return MI355ENC_OK;
}

int mi355enc_lut3d_check(const uint32_t *nodes, int N) {
    if (!nodes || N < LUT3D_N_MIN || N > LUT3D_N_MAX) return MI355ENC_ERR_ARG;
    for (int k = 0; k < N * N * N; k++) if (nodes[k] >> 30) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

int mi355enc_lut3d_identity(int N, uint32_t *nodes) {
    if (!nodes || N < LUT3D_N_MIN || N > LUT3D_N_MAX) return MI355ENC_ERR_ARG;
    uint32_t q[LUT3D_N_MAX];
    for (int i = 0; i < N; i++) q[i] = (uint32_t)((2 * i * 1023 + (N - 1)) / (2 * (N - 1)));
    for (int b = 0; b < N; b++) for (int g = 0; g < N; g++) for (int r = 0; r < N; r++) nodes[r + N * (g + N * b)] = q[r] | q[g] << 10 | q[b] << 20;
    return MI355ENC_OK;
}

/* ------------------------------------------------------------------ the .cube parser */
#define CUBE_UNIT 1000000000LL          /* a number is held in units of 10^-9 */
#define CUBE_LIMIT 1000000000000000LL   /* 10^6 in those units: a magnitude at or above it is refused */

static int is_space(char c) { return c == ' ' || c == '\t'; }
static int is_digit(char c) { return c >= '0' && c <= '9'; }

/* the token [p, e) as a decimal number -- sign, digits with an optional fraction (one digit at least on either side of the point), optional exponent -- in units
 * of 10^-9, digits beyond that truncated.  0 on success */
static int cube_number(const char *p, const char *e, int64_t *out) {
    int neg = 0;
    if (p < e && (*p == '+' || *p == '-')) neg = *p++ == '-';
    const char *ip = p;
    while (p < e && is_digit(*p)) p++;
    const char *ie = p, *fp = p, *fe = p;
    if (p < e && *p == '.') { fp = ++p; while (p < e && is_digit(*p)) p++; fe = p; }
    if (ie == ip && fe == fp) return -1;
    int ex = 0;
    if (p < e && (*p == 'e' || *p == 'E')) {
        int eneg = 0;
        p++;
        if (p < e && (*p == '+' || *p == '-')) eneg = *p++ == '-';
        if (p >= e || !is_digit(*p)) return -1;
        for (; p < e && is_digit(*p); p++) if (ex < 100000) ex = ex * 10 + (*p - '0');
        if (eneg) ex = -ex;
    }
    if (p != e) return -1;
    /* the digit j places in front of the point (behind it: negative) weighs 10^(j + ex + 9) units */
    int64_t acc = 0;
    for (int part = 0; part < 2; part++) {
        const char *a = part ? fp : ip, *b = part ? fe : ie;
        for (const char *c = a; c < b; c++) {
            const long place = part ? -(long)(c - fp) - 1 : (long)(ie - c) - 1;
            const long w = place + ex + 9;
            const int d = *c - '0';
            if (!d || w < 0) continue;
            if (w > 15) return -1;
            int64_t t = d;
            for (long k = 0; k < w; k++) t *= 10;
            acc += t;
            if (acc >= CUBE_LIMIT) return -1;
        }
    }
    *out = neg ? -acc : acc;
    return 0;
}

/* the next token of [*p, e): 0 at the line's end */
static int cube_token(const char **p, const char *e, const char **t0, const char **t1) {
    const char *c = *p;
    while (c < e && is_space(*c)) c++;
    if (c >= e) return 0;
    *t0 = c;
    while (c < e && !is_space(*c)) c++;
    *t1 = *p = c;
    return 1;
}
static int cube_is(const char *t0, const char *t1, const char *word) { return (size_t)(t1 - t0) == strlen(word) && !memcmp(t0, word, (size_t)(t1 - t0)); }
/* n numbers and nothing else up to the line's end */
static int cube_numbers(const char *p, const char *e, int n, int64_t *v) {
    const char *t0, *t1;
    for (int i = 0; i < n; i++) if (!cube_token(&p, e, &t0, &t1) || cube_number(t0, t1, v + i)) return -1;
    return cube_token(&p, e, &t0, &t1) ? -1 : 0;
}

int mi355enc_lut3d_parse_cube(const char *text, size_t len, uint32_t *nodes, size_t cap, int *N_out) {
    if (!text || !nodes || !N_out) return MI355ENC_ERR_ARG;
    int64_t lo[3] = {0, 0, 0}, hi[3] = {CUBE_UNIT, CUBE_UNIT, CUBE_UNIT};
    int N = 0;
    size_t rows = 0, want = 0;
    const char *p = text, *end = text + len;
    while (p < end) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *e = nl ? nl : end, *next = nl ? nl + 1 : end;
        if (e > p && e[-1] == '\r') e--;
        const char *q = p, *t0, *t1;
        p = next;
        if (!cube_token(&q, e, &t0, &t1) || *t0 == '#') continue;
        if ((*t0 >= 'A' && *t0 <= 'Z') || (*t0 >= 'a' && *t0 <= 'z')) { /* a keyword: in front of the first row only */
            int64_t v[3];
            if (rows) return MI355ENC_ERR_ARG;
            if (cube_is(t0, t1, "TITLE")) continue;
            if (cube_is(t0, t1, "LUT_3D_SIZE")) {
                if (N || cube_numbers(q, e, 1, v) || v[0] % CUBE_UNIT || v[0] < LUT3D_N_MIN * CUBE_UNIT || v[0] > LUT3D_N_MAX * CUBE_UNIT) return MI355ENC_ERR_ARG;
                N = (int)(v[0] / CUBE_UNIT);
                want = (size_t)N * N * N;
                if (want > cap) return MI355ENC_ERR_ARG;
            } else if (cube_is(t0, t1, "DOMAIN_MIN")) {
                if (cube_numbers(q, e, 3, lo)) return MI355ENC_ERR_ARG;
            } else if (cube_is(t0, t1, "DOMAIN_MAX")) {
                if (cube_numbers(q, e, 3, hi)) return MI355ENC_ERR_ARG;
            } else if (cube_is(t0, t1, "LUT_3D_INPUT_RANGE")) { /* the input domain: the rule has no pre-scale, so only the identity passes */
                if (cube_numbers(q, e, 2, v) || v[1] <= v[0] || v[0] != 0 || v[1] != CUBE_UNIT) return MI355ENC_ERR_ARG;
            } else return MI355ENC_ERR_ARG; /* LUT_1D_SIZE and everything unknown */
            continue;
        }
        int64_t v[3];
        if (!N || rows >= want || cube_numbers(t0, e, 3, v)) return MI355ENC_ERR_ARG;
        uint32_t word = 0;
        for (int c = 0; c < 3; c++) {
            const int64_t d = hi[c] - lo[c];
            if (d <= 0) return MI355ENC_ERR_ARG;
            const int64_t num = v[c] >= hi[c] ? 0 : (v[c] - lo[c]) * 2046 + d;
            const uint32_t qv = v[c] >= hi[c] ? 1023u : num < 0 ? 0u : (uint32_t)(num / (2 * d));
            word |= (qv > 1023u ? 1023u : qv) << (10 * c);
        }
        nodes[rows++] = word;
    }
    if (!N || rows != want) return MI355ENC_ERR_ARG;
    for (int c = 0; c < 3; c++) if (hi[c] <= lo[c]) return MI355ENC_ERR_ARG;
    *N_out = N;
    return MI355ENC_OK;
}

/* ------------------------------------------------------------------ the rule on host planes */
int mi355enc_lut3d_apply_host(const uint32_t *nodes, int N, int strength, int matrix, int full_range, uint8_t *y, uint8_t *uv, int stride, int height, const int rect[4]) {
    int32_t coef[LUT3D_COEF_WORDS];
    if (mi355enc_lut3d_check(nodes, N) || strength < 0 || strength > 256 || mi355enc_lut3d_coefficients(matrix, full_range, coef)) return MI355ENC_ERR_ARG;
    if (!y || !uv || !rect || stride < 2 || height < 2 || (stride & 1) || (height & 1)) return MI355ENC_ERR_ARG;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > stride || rect[3] > height || rect[0] >= rect[1] || rect[2] >= rect[3]) return MI355ENC_ERR_ARG;
    if (!strength) return MI355ENC_OK;
    for (int qy = rect[2]; qy < rect[3]; qy += 2) {
        for (int qx = rect[0]; qx < rect[1]; qx += 2) {
            uint8_t *pc = uv + (size_t)(qy >> 1) * stride + qx;
            const int vu = pc[0] - 128, vv = pc[1] - 128;
            int su = 0, sv = 0;
            for (int k = 0; k < 4; k++) {
                uint8_t *py = y + (size_t)(qy + (k >> 1)) * stride + qx + (k & 1);
                const int vy = *py - coef[18];
                int idx[4], w[4];
                lut3d_cell(N, lut3d_rgb(coef, vy, vu, vv), lut3d_rgb(coef + 3, vy, vu, vv), lut3d_rgb(coef + 6, vy, vu, vv), idx, w);
                const uint32_t g = lut3d_blend(nodes[idx[0]], nodes[idx[1]], nodes[idx[2]], nodes[idx[3]], w);
                su += lut3d_dot(coef + 12, g); sv += lut3d_dot(coef + 15, g);
                *py = (uint8_t)lut3d_mix(*py, lut3d_luma(coef, g), strength);
            }
            pc[0] = (uint8_t)lut3d_mix(pc[0], lut3d_chroma(su), strength);
            pc[1] = (uint8_t)lut3d_mix(pc[1], lut3d_chroma(sv), strength);
        }
    }
    return MI355ENC_OK;
}

int mi355enc_lut3d_plan(int N) {
    if (N < LUT3D_N_MIN || N > LUT3D_N_MAX) return MI355ENC_ERR_ARG;
    return N <= LUT3D_STAGED_TO ? 1 : 0;
}
