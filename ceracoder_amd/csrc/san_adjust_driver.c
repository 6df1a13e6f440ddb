/* san_adjust_driver.c -- the rule of the picture controls (adjust_host.c) under ASan + UBSan (make san/san_adjust; tests/test_adjust_san_cpu.py): every
 * range edge of every parameter, one step inside and one outside, then a few thousand seeded parameter sets for both output ranges, each table built into
 * buffers of exactly its size and checked for what the kernels rely on (non-decreasing table, bounded rotation).  Prints a JSON count.  Host code only. */
#include "adjust_host.h"

#include <stdio.h>
#include <stdlib.h>

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static int between(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static const int k_lo[7] = {-1000, 0, 0, -1000, 100, -16, 0}, k_hi[7] = {1000, 2000, 2000, 1000, 10000, 64, 32};
static int *field(mi355enc_adjust_t *a, int i) {
    switch (i) {
    case 0: return &a->brightness;
    case 1: return &a->contrast;
    case 2: return &a->saturation;
    case 3: return &a->hue;
    case 4: return &a->gamma;
    case 5: return &a->sharpen;
    default: return &a->sharpen_threshold;
    }
}

/* 0: the tables are what the kernels may rely on */
static int tables_bad(const uint8_t *luma, const int32_t *chroma, const mi355enc_adjust_t *a) {
    for (int v = 1; v < 256; v++) if (luma[v] < luma[v - 1]) return 1;
    /* |(cu, su)| = 4096 sat / 1000 up to the two roundings: 127 (|cu| + |su|) + 2048 stays far inside 32 bits */
    const long n2 = (long)chroma[0] * chroma[0] + (long)chroma[1] * chroma[1], g = 4096L * a->saturation / 1000 + 2;
    if (n2 > g * g) return 2;
    return 0;
}

int main(void) {
    long bad = 0, sets = 0, refused = 0, edges = 0;
    /* exactly the sizes asked for, on the heap: a write past either is caught */
    uint8_t *luma = (uint8_t *)malloc(256);
    int32_t *chroma = (int32_t *)malloc(2 * sizeof(int32_t));
    if (!luma || !chroma) return 2;
    mi355enc_adjust_t a;
    mi355enc_adjust_default(&a);
    if (mi355enc_adjust_check(&a) || adjust_parts(&a) || mi355enc_adjust_check(NULL) != MI355ENC_ERR_ARG) bad++;
    mi355enc_adjust_default(NULL);
    for (int full = 0; full < 2; full++) { /* neutral: the identity and {4096, 0} */
        if (mi355enc_adjust_tables(&a, full, luma, chroma)) bad++;
        for (int v = 0; v < 256; v++) if (luma[v] != v) bad++;
        if (chroma[0] != 4096 || chroma[1] != 0) bad++;
    }
    for (int i = 0; i < 7; i++)
        for (int e = 0; e < 2; e++)
            for (int d = -1; d <= 1; d++) {
                mi355enc_adjust_default(&a);
                const int v = (e ? k_hi[i] : k_lo[i]) + d, ok = v >= k_lo[i] && v <= k_hi[i];
                *field(&a, i) = v;
                for (int full = -1; full <= 2; full++) {
                    const int want = ok && (full == 0 || full == 1);
                    const int r = mi355enc_adjust_tables(&a, full, luma, chroma);
                    if ((r == MI355ENC_OK) != want || (mi355enc_adjust_check(&a) == MI355ENC_OK) != ok) bad++;
                    if (r) refused++;
                    else if (tables_bad(luma, chroma, &a)) bad++;
                    edges++;
                }
            }
    mi355enc_adjust_default(&a);
    if (mi355enc_adjust_tables(&a, 0, NULL, chroma) != MI355ENC_ERR_ARG || mi355enc_adjust_tables(&a, 0, luma, NULL) != MI355ENC_ERR_ARG ||
        mi355enc_adjust_tables(NULL, 0, luma, chroma) != MI355ENC_ERR_ARG) bad++;
    /* seeded parameter sets over the whole valid range; every other one with gamma 1000 (the integer path) */
    for (int n = 0; n < 4000; n++) {
        for (int i = 0; i < 7; i++) *field(&a, i) = (rnd() & 15) ? between(k_lo[i], k_hi[i]) : (rnd() & 1) ? k_lo[i] : k_hi[i];
        if (n & 1) a.gamma = 1000;
        if (mi355enc_adjust_tables(&a, (int)(rnd() & 1), luma, chroma) != MI355ENC_OK || tables_bad(luma, chroma, &a)) bad++;
        sets++;
    }
    free(luma);
    free(chroma);
    printf("{\"bad\": %ld, \"sets\": %ld, \"edges\": %ld, \"refused\": %ld}\n", bad, sets, edges, refused);
    return bad ? 1 : 0;
}
