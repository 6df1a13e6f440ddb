/* san_denoise_driver.c -- the rule of the temporal noise filter (denoise_host.c) under ASan + UBSan (make san/san_denoise; tests/test_denoise_san_cpu.py):
 * both strengths at each range edge, one step inside and one outside, then a few thousand seeded parameter sets, each table built into a buffer of exactly
 * 256 bytes on the heap and checked for what the kernel relies on (bounded, non-increasing, the plateau and the zero where the rule puts them).  Prints a JSON
 * count.  Host code only. */
#include "denoise_host.h"

#include <stdio.h>
#include <stdlib.h>

static uint32_t rng_state = 0x2545f491u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static int between(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

/* 0: a sample table of strength s is what the kernel may rely on */
static int sample_bad(const uint8_t *p, int s) {
    for (int a = 0; a < 256; a++) {
        if (s == 0) { if (p[a]) return 1; continue; }
        if (p[a] > 224 || (a && p[a] > p[a - 1])) return 2;
        if ((a <= s) != (p[a] == 224) || (a >= 3 * s) != (p[a] == 0)) return 3;
    }
    return 0;
}
static int block_bad(const uint8_t *b, int s) {
    for (int i = 0; i < 256; i++) {
        if (s == 0) { if (b[i]) return 1; continue; }
        if (i && b[i] > b[i - 1]) return 2;
        if ((i <= 2 * s) != (b[i] == 255) || (i >= 6 * s) != (b[i] == 0)) return 3;
    }
    return 0;
}

int main(void) {
    long bad = 0, sets = 0, refused = 0, edges = 0;
    /* exactly the sizes asked for, on the heap: a write past any of them is caught */
    uint8_t *block = (uint8_t *)malloc(256), *luma = (uint8_t *)malloc(256), *chroma = (uint8_t *)malloc(256);
    if (!block || !luma || !chroma) return 2;
    mi355enc_denoise_t d;
    mi355enc_denoise_default(&d);
    if (d.luma || d.chroma || mi355enc_denoise_check(&d) || denoise_parts(&d) || mi355enc_denoise_check(NULL) != MI355ENC_ERR_ARG) bad++;
    mi355enc_denoise_default(NULL);
    for (int f = 0; f < 2; f++)
        for (int e = 0; e < 2; e++)
            for (int k = -1; k <= 1; k++)
                for (int other = 0; other <= MI355ENC_DENOISE_MAX; other += MI355ENC_DENOISE_MAX / 2) {
                    const int v = (e ? MI355ENC_DENOISE_MAX : 0) + k, ok = v >= 0 && v <= MI355ENC_DENOISE_MAX;
                    d.luma = f ? other : v; d.chroma = f ? v : other;
                    const int r = mi355enc_denoise_tables(&d, block, luma, chroma);
                    if ((r == MI355ENC_OK) != ok || (mi355enc_denoise_check(&d) == MI355ENC_OK) != ok) bad++;
                    if (r) refused++;
                    else if (sample_bad(luma, d.luma) || sample_bad(chroma, d.chroma) || block_bad(block, d.luma ? d.luma : d.chroma)) bad++;
                    edges++;
                }
    d.luma = d.chroma = 8;
    if (mi355enc_denoise_tables(&d, NULL, luma, chroma) != MI355ENC_ERR_ARG || mi355enc_denoise_tables(&d, block, NULL, chroma) != MI355ENC_ERR_ARG ||
        mi355enc_denoise_tables(&d, block, luma, NULL) != MI355ENC_ERR_ARG || mi355enc_denoise_tables(NULL, block, luma, chroma) != MI355ENC_ERR_ARG) bad++;
    for (int n = 0; n < 4000; n++) {
        d.luma = (rnd() & 7) ? between(0, MI355ENC_DENOISE_MAX) : (rnd() & 1) ? 0 : MI355ENC_DENOISE_MAX;
        d.chroma = (rnd() & 7) ? between(0, MI355ENC_DENOISE_MAX) : (rnd() & 1) ? 0 : MI355ENC_DENOISE_MAX;
        if (mi355enc_denoise_tables(&d, block, luma, chroma) != MI355ENC_OK || sample_bad(luma, d.luma) || sample_bad(chroma, d.chroma) ||
            block_bad(block, d.luma ? d.luma : d.chroma) || denoise_parts(&d) != ((d.luma ? DENOISE_LUMA : 0) | (d.chroma ? DENOISE_CHROMA : 0))) bad++;
        sets++;
    }
    free(block);
    free(luma);
    free(chroma);
    printf("{\"bad\": %ld, \"sets\": %ld, \"edges\": %ld, \"refused\": %ld}\n", bad, sets, edges, refused);
    return bad ? 1 : 0;
}
