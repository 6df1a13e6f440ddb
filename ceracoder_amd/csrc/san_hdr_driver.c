/* san_hdr_driver.c -- the parameter block of the HDR tone map (hdr_host.c) under ASan + UBSan (make san/san_hdr; tests/test_hdr_san_cpu.py): the whole
 * argument range of mi355enc_hdr_tables, then a few thousand seeded parameter sets, each block checked for what the device's addressing and arithmetic rely
 * on (non-negative, bounded, monotone tables).  Prints a JSON count.  Host code only. */
#include "hdr_host.h"

#include <stdio.h>
#include <stdlib.h>

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static int between(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

/* 0: the block is what the kernel may rely on */
static int block_bad(const int32_t *b, int transfer) {
    if (b[0] != 1 || b[7] != HDR_WORDS || b[1] != transfer) return 1;
    for (int i = 0; i < HDR_LIN_N; i++) {
        const int32_t v = b[HDR_LIN_AT + i];
        if (v < 0 || v > (1 << 28) || (i && v < b[HDR_LIN_AT + i - 1])) return 2;
    }
    for (int i = 0; i < HDR_GAIN_N; i++) {
        const int32_t ga = b[HDR_GA_AT + i], gb = b[HDR_GB_AT + i];
        if (ga <= 0 || ga > (1 << 30) || (i && ga < b[HDR_GA_AT + i - 1])) return 3;
        if (gb <= 0 || (i && gb > b[HDR_GB_AT + i - 1])) return 4; /* (the tone gain falls) */
    }
    for (int i = 0; i < HDR_OE_N; i++) {
        const int32_t v = b[HDR_OE_AT + i];
        if (v < 0 || v > 65536 || (i && v < b[HDR_OE_AT + i - 1])) return 5;
    }
    for (int r = 0; r < 3; r++) if (b[17 + 3 * r] + b[18 + 3 * r] + b[19 + 3 * r] != (1 << 20)) return 6;
    if (b[14] + b[15] + b[16] != 65536 || b[29] + b[30] + b[31] != 0 || b[32] + b[33] + b[34] != 0) return 7;
    return 0;
}

int main(void) {
    int32_t *blk = (int32_t *)malloc(HDR_WORDS * sizeof(int32_t)); /* exactly the size asked for: a write past it is caught */
    long built = 0, refused = 0, bad = 0;
    size_t n = 0;
    if (!blk) return 2;
    /* the edges of every argument, valid and not */
    static const int transfers[] = {0, 1, 15, 16, 17, 18, 19, -1}, fulls[] = {-1, 0, 1, 2}, peaks[] = {-1, 0, 1, 399, 400, 1000, 2000, 2001, 4000, 10000, 10001, 1 << 30},
                     targets[] = {-1, 0, 99, 100, 203, 400, 401, 1 << 30}, mats[] = {0, 1, 2, 5, 6, 9, 256}, ofulls[] = {-1, 0, 1, 2};
    for (unsigned a = 0; a < sizeof transfers / sizeof *transfers; a++)
    for (unsigned f = 0; f < sizeof fulls / sizeof *fulls; f++)
    for (unsigned p = 0; p < sizeof peaks / sizeof *peaks; p++)
    for (unsigned t = 0; t < sizeof targets / sizeof *targets; t++)
    for (unsigned m = 0; m < sizeof mats / sizeof *mats; m++)
    for (unsigned o = 0; o < sizeof ofulls / sizeof *ofulls; o++) {
        const int tr = transfers[a], fu = fulls[f], pk = peaks[p], tg = targets[t], om = mats[m], of = ofulls[o];
        const int want_ok = (tr == 16 || tr == 18) && (fu == 0 || fu == 1) && (pk == 0 || (pk >= 400 && pk <= (tr == 16 ? 10000 : 2000))) &&
                            (tg == 0 || (tg >= 100 && tg <= 400)) && (om == 1 || om == 5 || om == 6) && (of == 0 || of == 1);
        /* the size alone for most valid sets (a block costs some ten thousand pow() calls); every fourth is built */
        const int build = want_ok && ((a + f + p + t + m + o) & 3) == 0;
        const int r = mi355enc_hdr_tables(tr, fu, pk, tg, om, of, build ? blk : NULL, build ? HDR_WORDS : 0, &n);
        if ((r == MI355ENC_OK) != want_ok || (want_ok && n != HDR_WORDS)) bad++;
        if (r) refused++;
        if (build) { built++; if (block_bad(blk, tr)) bad++; }
    }
    /* a buffer that is too small, no size pointer */
    if (mi355enc_hdr_tables(16, 0, 0, 0, 1, 0, blk, HDR_WORDS - 1, &n) != MI355ENC_ERR_OVERFLOW) bad++;
    if (mi355enc_hdr_tables(16, 0, 0, 0, 1, 0, blk, HDR_WORDS, NULL) != MI355ENC_ERR_ARG) bad++;
    /* seeded parameter sets over the whole valid range */
    long sets = 0;
    for (int i = 0; i < 3000; i++) {
        const int tr = (rnd() & 1) ? 16 : 18, pk = (rnd() & 7) ? between(400, tr == 16 ? 10000 : 2000) : 0, tg = (rnd() & 7) ? between(100, 400) : 0;
        static const int om[3] = {1, 5, 6};
        if (mi355enc_hdr_tables(tr, (int)(rnd() & 1), pk, tg, om[rnd() % 3], (int)(rnd() & 1), blk, HDR_WORDS, &n) != MI355ENC_OK || block_bad(blk, tr)) bad++;
        sets++;
    }
    free(blk);
    printf("{\"bad\": %ld, \"sets\": %ld, \"built\": %ld, \"refused\": %ld}\n", bad, sets, built, refused);
    return bad ? 1 : 0;
}
