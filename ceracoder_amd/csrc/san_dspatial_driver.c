/* san_dspatial_driver.c -- the rule of the spatial noise filter (dspatial_host.c) under ASan + UBSan (make san/san_dspatial;
 * tests/test_denoise_spatial_san_cpu.py): every range edge of the setting, one step inside and one outside; the 33 tables into buffers of exactly their size;
 * the filter and the measurement on exactly-sized heap surfaces -- every neighbour clamped, margins, a border, samples of 0 and 255 only, every strength edge;
 * decisions at the ceilings of the measurement and from both ends of the state; and seeded ones checked for what the rule promises.  Prints a JSON count.
 * Host code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355enc.h"

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static const int LO[5] = {0, 0, 250, 1, 1}, HI[5] = {32, 32, 8000, 50, 256};
static int *field(mi355enc_denoise_spatial_t *a, int i) { return i == 0 ? &a->luma : i == 1 ? &a->chroma : i == 2 ? &a->auto_gain : i == 3 ? &a->percentile : &a->speed; }

/* one decision into exactly-sized heap buffers; returns the code, counts what the rule promises as bad */
static int decide(const mi355enc_denoise_spatial_meas_t *m, const mi355enc_denoise_spatial_t *a, int prime, int32_t x_in, long *bad) {
    mi355enc_denoise_spatial_meas_t *mm = (mi355enc_denoise_spatial_meas_t *)malloc(sizeof *mm);
    int32_t *x = (int32_t *)malloc(sizeof *x);
    mi355enc_denoise_spatial_info_t *info = (mi355enc_denoise_spatial_info_t *)malloc(sizeof *info);
    if (!mm || !x || !info) exit(2);
    *mm = *m; *x = x_in;
    const int r = mi355enc_denoise_spatial_decide(mm, a, prime, x, info);
    if (r == MI355ENC_OK) {
        if (*x != info->x || *x < 0 || *x > 65280 || info->v < 0 || info->v > 255) (*bad)++;
        if (info->s_luma < 0 || info->s_luma > a->luma || info->s_chroma < 0 || info->s_chroma > a->chroma) (*bad)++;
        if (info->valid && (prime || a->speed == 256) && *x != 256 * info->v) (*bad)++;
        if (!info->valid && *x != (prime ? 0 : x_in)) (*bad)++;
        if ((uint32_t)info->candidates != m->candidates || (uint32_t)info->voters != m->voters) (*bad)++;
    }
    free(mm); free(x); free(info);
    return r;
}

/* the filter and the measurement on exactly-sized surfaces; the border must keep its bytes, a sample must stay between 0 and 255 of its window (here: of the plane) */
static void surfaces(int W, int H, const int rect[4], int vw, int vh, int kind, int sl, int sc, long *bad, long *runs) {
    const size_t ysz = (size_t)W * H;
    uint8_t *y = (uint8_t *)malloc(ysz), *uv = (uint8_t *)malloc(ysz / 2), *y0 = (uint8_t *)malloc(ysz), *uv0 = (uint8_t *)malloc(ysz / 2);
    mi355enc_denoise_spatial_meas_t *m = (mi355enc_denoise_spatial_meas_t *)malloc(sizeof *m);
    if (!y || !uv || !y0 || !uv0 || !m) exit(2);
    for (size_t i = 0; i < ysz; i++) y[i] = kind == 0 ? (uint8_t)rnd() : kind == 1 ? (uint8_t)((rnd() & 1) * 255) : (uint8_t)(120 + rnd() % 9);
    for (size_t i = 0; i < ysz / 2; i++) uv[i] = kind == 0 ? (uint8_t)rnd() : kind == 1 ? (uint8_t)((rnd() & 1) * 255) : (uint8_t)(126 + rnd() % 5);
    memcpy(y0, y, ysz); memcpy(uv0, uv, ysz / 2);
    for (int full = 0; full < 2; full++) {
        if (mi355enc_denoise_spatial_measure_host(y, W, H, rect, vw, vh, full, m)) (*bad)++;
        uint64_t n = 0;
        for (int v = 0; v < 256; v++) n += m->hist[v];
        if (n != m->voters || m->voters > m->candidates) (*bad)++;
    }
    if (mi355enc_denoise_spatial_apply_host(y, uv, W, H, rect, vw, vh, sl, sc)) (*bad)++;
    for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++) {
            const int in = c >= rect[0] && c < rect[1] && r >= rect[2] && r < rect[3];
            if ((!in || sl < 0) && y[(size_t)r * W + c] != y0[(size_t)r * W + c]) { (*bad)++; r = H; break; }
        }
    for (int r = 0; r < H / 2; r++)
        for (int c = 0; c < W; c++) {
            const int in = c >= rect[0] && c < rect[1] && 2 * r >= rect[2] && 2 * r < rect[3];
            if ((!in || sc < 0) && uv[(size_t)r * W + c] != uv0[(size_t)r * W + c]) { (*bad)++; r = H; break; }
        }
    (*runs)++;
    free(y); free(uv); free(y0); free(uv0); free(m);
}

int main(void) {
    long bad = 0, edges = 0, refused = 0, decisions = 0, sets = 0, tables = 0, runs = 0;
    mi355enc_denoise_spatial_t a;
    mi355enc_denoise_spatial_default(NULL);
    mi355enc_denoise_spatial_default(&a);
    if (a.luma != 0 || a.chroma != 0 || a.auto_gain != 0 || a.percentile != 25 || a.speed != 32) bad++;
    if (mi355enc_denoise_spatial_check(&a) || mi355enc_denoise_spatial_check(NULL) != MI355ENC_ERR_ARG) bad++;
    /* every range edge of every field: the edge and one step inside are taken, one step outside is refused (auto_gain: 0 is taken too, 1 .. 249 are not) */
    for (int i = 0; i < 5; i++)
        for (int e = 0; e < 2; e++)
            for (int d = -1; d <= 1; d++) {
                mi355enc_denoise_spatial_default(&a);
                a.luma = 4;
                *field(&a, i) = (e ? HI[i] : LO[i]) + d;
                const int outside = e ? d > 0 : d < 0, r = mi355enc_denoise_spatial_check(&a);
                if ((r != MI355ENC_OK) != outside) bad++;
                edges++;
            }
    mi355enc_denoise_spatial_default(&a);
    for (int g = -1; g <= 250; g += (g == 1 ? 248 : 1)) { a.auto_gain = g; if ((mi355enc_denoise_spatial_check(&a) == MI355ENC_OK) != (g == 0 || g == 250)) bad++; }
    /* the tables, into exactly 256 entries each */
    for (int s = -1; s <= 33; s++) {
        uint8_t *w = (uint8_t *)malloc(256);
        uint16_t *f = (uint16_t *)malloc(256 * sizeof *f);
        if (!w || !f) exit(2);
        const int r = mi355enc_denoise_spatial_tables(s, w, f);
        if ((r != MI355ENC_OK) != (s < 0 || s > 32)) bad++;
        if (r == MI355ENC_OK) {
            for (int v = 0; v < 256; v++) {
                const int want = s == 0 ? 0 : v <= s ? 16 : v >= 3 * s ? 0 : -1;
                if ((want >= 0 && w[v] != want) || w[v] > 16 || f[v] != v * w[v] || (v && w[v] > w[v - 1])) { bad++; break; }
            }
            if (mi355enc_denoise_spatial_tables(s, w, NULL) || mi355enc_denoise_spatial_tables(s, NULL, f) || mi355enc_denoise_spatial_tables(s, NULL, NULL) != MI355ENC_ERR_ARG) bad++;
            tables++;
        }
        free(w); free(f);
    }
    /* surfaces: every neighbour clamped; margins; a border; the smallest visible part */
    static const int shapes[5][8] = {{16, 16, 0, 16, 0, 16, 16, 16}, {48, 32, 0, 48, 0, 32, 42, 26}, {80, 64, 18, 62, 10, 38, 80, 64}, {80, 64, 18, 80, 10, 64, 70, 50}, {16, 2, 0, 16, 0, 2, 1, 1}};
    static const int strengths[6][2] = {{1, 1}, {32, 32}, {0, 0}, {8, -1}, {-1, 8}, {-1, -1}};
    for (int i = 0; i < 5; i++)
        for (int kind = 0; kind < 3; kind++)
            for (int k = 0; k < 6; k++) surfaces(shapes[i][0], shapes[i][1], shapes[i] + 2, shapes[i][6], shapes[i][7], kind, strengths[k][0], strengths[k][1], &bad, &runs);
    {
        uint8_t px[32 * 2] = {0};
        const int rect[4] = {0, 16, 0, 2}, odd[4] = {1, 16, 0, 2};
        mi355enc_denoise_spatial_meas_t m;
        if (mi355enc_denoise_spatial_apply_host(px, px + 32, 16, 2, rect, 16, 2, 33, 0) != MI355ENC_ERR_ARG || mi355enc_denoise_spatial_apply_host(px, px + 32, 16, 2, odd, 16, 2, 1, 1) != MI355ENC_ERR_ARG) bad++;
        if (mi355enc_denoise_spatial_apply_host(NULL, px, 16, 2, rect, 16, 2, 1, 1) != MI355ENC_ERR_ARG || mi355enc_denoise_spatial_measure_host(px, 16, 2, rect, 17, 2, 0, &m) != MI355ENC_ERR_ARG) bad++;
        if (mi355enc_denoise_spatial_measure_host(px, 24, 2, rect, 16, 2, 0, &m) != MI355ENC_ERR_ARG || mi355enc_denoise_spatial_measure_host(px, 16, 2, rect, 16, 2, 0, NULL) != MI355ENC_ERR_ARG) bad++;
        refused += 6;
    }
    /* decisions at the ceilings: 2^20 candidates that all vote in one bin at either end, from both ends of the state, every speed and gain edge */
    {
        static const int speeds[3] = {1, 128, 256}, gains[2] = {250, 8000};
        static const int32_t ends[3] = {0, 32640, 65280};
        mi355enc_denoise_spatial_meas_t m;
        for (int bin = 0; bin < 256; bin += 255)
            for (int si = 0; si < 3; si++)
                for (int gi = 0; gi < 2; gi++)
                    for (int xi = 0; xi < 3; xi++)
                        for (int prime = 0; prime < 2; prime++) {
                            memset(&m, 0, sizeof m);
                            m.hist[bin] = m.voters = m.candidates = 1u << 20;
                            mi355enc_denoise_spatial_default(&a);
                            a.luma = 32; a.chroma = 7; a.auto_gain = gains[gi]; a.speed = speeds[si]; a.percentile = 50;
                            if (decide(&m, &a, prime, ends[xi], &bad)) bad++;
                            decisions++;
                        }
        memset(&m, 0, sizeof m);
        m.hist[3] = m.voters = 5; m.candidates = 5;
        mi355enc_denoise_spatial_default(&a);
        if (decide(&m, &a, 1, 0, &bad) != MI355ENC_ERR_ARG) bad++; /* manual: nothing to decide */
        a.auto_gain = 1000;
        if (decide(&m, &a, 0, -1, &bad) != MI355ENC_ERR_ARG || decide(&m, &a, 0, 65281, &bad) != MI355ENC_ERR_ARG) bad++;
        if (decide(&m, &a, 1, -1, &bad)) bad++; /* (with prime the state going in is ignored) */
        m.voters = 6;
        if (decide(&m, &a, 1, 0, &bad) != MI355ENC_ERR_ARG) bad++; /* more voters than candidates; the histogram's sum is not the voters */
        m.voters = 5; m.candidates = (1u << 20) + 1;
        if (decide(&m, &a, 1, 0, &bad) != MI355ENC_ERR_ARG) bad++;
        if (mi355enc_denoise_spatial_decide(NULL, &a, 1, NULL, NULL) != MI355ENC_ERR_ARG) bad++;
        refused += 6;
    }
    /* seeded decisions */
    for (int t = 0; t < 4000; t++) {
        mi355enc_denoise_spatial_meas_t m;
        memset(&m, 0, sizeof m);
        const int n = (int)(rnd() % 300);
        for (int k = 0; k < n; k++) m.hist[rnd() & 255]++;
        m.voters = (uint32_t)n; m.candidates = (uint32_t)n * (1 + rnd() % 20) + rnd() % 5;
        a.luma = (int)(rnd() % 33); a.chroma = (int)(rnd() % 33); a.auto_gain = 250 + (int)(rnd() % 7751); a.percentile = 1 + (int)(rnd() % 50); a.speed = 1 + (int)(rnd() % 256);
        if (decide(&m, &a, (int)(rnd() & 1), (int32_t)(rnd() % 65281), &bad)) bad++;
        sets++;
    }
    printf("{\"bad\": %ld, \"edges\": %ld, \"tables\": %ld, \"runs\": %ld, \"decisions\": %ld, \"refused\": %ld, \"sets\": %ld}\n", bad, edges, tables, runs, decisions, refused, sets);
    return bad ? 1 : 0;
}
