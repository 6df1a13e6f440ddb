/* denoise_host.c -- the rule of the temporal noise filter: argument ranges and the three tables of a parameter set -- the weight of
 * the history by a sample's own difference (one table per plane) and by its 8 x 8 block's measure.  Host only, no device needed; tests/denoiseref.py restates it
 * in numpy integers. */
#include "denoise_host.h"

#include <stddef.h>
#include <string.h>

/* floor(n / d), d > 0 (C's division truncates a negative numerator towards zero) */
static long floor_div(long n, long d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }
static long clip(long lo, long hi, long v) { return v < lo ? lo : v > hi ? hi : v; }

void mi355enc_denoise_default(mi355enc_denoise_t *d) {
    if (!d) return;
    d->luma = 0; d->chroma = 0;
}

int mi355enc_denoise_check(const mi355enc_denoise_t *d) {
    if (!d || d->luma < 0 || d->luma > MI355ENC_DENOISE_MAX || d->chroma < 0 || d->chroma > MI355ENC_DENOISE_MAX) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

int denoise_parts(const mi355enc_denoise_t *d) { return (d->luma > 0 ? DENOISE_LUMA : 0) | (d->chroma > 0 ? DENOISE_CHROMA : 0); }

/* P_s[a] = clip(0, 224, floor(224 (3 s - a) / (2 s))): full weight up to a = s, none from 3 s on; s = 0: the plane is not filtered, all zeros */
static void sample_table(int s, uint8_t t[256]) {
    memset(t, 0, 256);
    for (int a = 0; s > 0 && a < 256; a++) t[a] = (uint8_t)clip(0, 224, floor_div(224L * (3 * s - a), 2L * s));
}

int mi355enc_denoise_tables(const mi355enc_denoise_t *d, uint8_t block[256], uint8_t luma[256], uint8_t chroma[256]) {
    if (mi355enc_denoise_check(d) || !block || !luma || !chroma) return MI355ENC_ERR_ARG;
    sample_table(d->luma, luma);
    sample_table(d->chroma, chroma);
    /* B[i] = clip(0, 255, floor(255 (6 s - i) / (4 s))), i = min(255, M >> 4): the mean difference of the block in quarter codes; full weight up to 2 s, none from 6 s on */
    const int s = d->luma ? d->luma : d->chroma;
    memset(block, 0, 256);
    for (int i = 0; s > 0 && i < 256; i++) block[i] = (uint8_t)clip(0, 255, floor_div(255L * (6 * s - i), 4L * s));
    return MI355ENC_OK;
}

/* ---- motion compensation: how the search ranks a candidate (dx, dy) of cost `cost`; tests/denoisemcref.py restates it */
int denoise_motion_lambda(int s) { return 4 * s; }

uint32_t mi355enc_denoise_motion_key(int cost, int dx, int dy, int s) {
    if (cost < 0 || cost > 64 * 255 || dx < -MI355ENC_DENOISE_MOTION_MAX || dx > MI355ENC_DENOISE_MOTION_MAX || dy < -MI355ENC_DENOISE_MOTION_MAX ||
        dy > MI355ENC_DENOISE_MOTION_MAX || s < 0 || s > MI355ENC_DENOISE_MAX)
        return 0xFFFFFFFFu;
    const int n = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
    /* the penalised cost stays below 2^15 (16320 + 128 * 32), the rank below 2^16 (32 * 1089 + 32 * 33 + 32): unique per vector, shorter first, then by dy, then by dx */
    return ((uint32_t)(cost + denoise_motion_lambda(s) * n) << 16) | (uint32_t)(n * 1089 + (dy + 16) * 33 + (dx + 16));
}
