/* rate_host.c -- the rule of the frame-rate conversion: which ticks an input makes due, what they show, when the grid
 * re-anchors.  Integer only; every product is taken in 128 bits (2 N (p - T0) passes 2^63 after ten days of nanoseconds at N = 60000).
 * No device, no allocation: the shim keeps one plan per handle, tests and the stand-alone driver keep their own. */
#include "rate_host.h"

typedef __int128 i128;

/* floor(a / b), b > 0 */
static i128 floordiv(i128 a, i128 b) {
    i128 q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
static i128 plan_d(const mi355enc_rate_plan_t *pl) { return (i128)pl->pps * pl->fps_den; }

int64_t rate_tick_pts(const mi355enc_rate_plan_t *pl, int64_t k) {
    return (int64_t)((i128)pl->t0 + floordiv((i128)k * plan_d(pl), pl->fps_num));
}

int mi355enc_rate_check(const mi355enc_rate_t *r) {
    if (!r || r->mode < 0 || r->mode > 2 || r->pts_per_second <= 0 || r->max_fill < 0) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

void mi355enc_rate_plan_init(mi355enc_rate_plan_t *pl, int mode, int64_t pps, int fps_num, int fps_den, int max_fill, int64_t t0, int64_t k_next) {
    if (!pl) return;
    pl->mode = mode < 0 || mode > 2 ? 0 : mode;
    pl->pps = pps > 0 ? pps : 1;
    pl->fps_num = fps_num > 0 ? fps_num : 1;
    pl->fps_den = fps_den > 0 ? fps_den : 1;
    pl->max_fill = max_fill < 0 ? 0 : max_fill > MI355ENC_RATE_MAX_OUT - 1 ? MI355ENC_RATE_MAX_OUT - 1 : max_fill;
    pl->started = k_next >= 0;
    pl->t0 = pl->started ? t0 : 0;
    pl->k_next = pl->started ? k_next : 0;
    pl->prev_pts = pl->started ? (k_next > 0 ? rate_tick_pts(pl, k_next - 1) : t0) : 0;
}

/* the weight of input p1 in tick k between the inputs at p0 and p1: round-half-up(256 (T_k - p0) / (p1 - p0)) on the exact T_k = t0 + k D / N */
static int blend_weight(const mi355enc_rate_plan_t *pl, i128 k, int64_t p0, int64_t p1) {
    const i128 N = pl->fps_num, den = N * ((i128)p1 - p0);
    if (den <= 0) return 256;
    const i128 num = 256 * (((i128)pl->t0 - p0) * N + k * plan_d(pl));
    const i128 w = floordiv(2 * num + den, 2 * den);
    return w < 0 ? 0 : w > 256 ? 256 : (int)w;
}

int mi355enc_rate_plan_step(mi355enc_rate_plan_t *pl, int64_t pts, int *n, int64_t out_pts[], int weight[], int *resync) {
    if (!pl || !n || !out_pts || !weight || !resync || pl->fps_num <= 0 || pl->fps_den <= 0 || pl->pps <= 0 || pl->max_fill < 0 ||
        pl->max_fill >= MI355ENC_RATE_MAX_OUT || pl->mode < 0 || pl->mode > 2) return MI355ENC_ERR_ARG;
    *resync = 0;
    int anchor = !pl->started;
    if (pl->mode == 0) { *n = 1; out_pts[0] = pts; weight[0] = 256; return MI355ENC_OK; }
    if (!anchor && pts < pl->prev_pts) anchor = *resync = 1;
    if (!anchor) {
        const i128 N = pl->fps_num, D = plan_d(pl), tol = pl->mode == 1 ? 2 : 16;
        const i128 k_max = floordiv(tol * N * ((i128)pts - pl->t0) + D, tol * D);
        const i128 cnt = k_max - pl->k_next + 1;
        if (cnt <= 0) { *n = 0; pl->prev_pts = pts; return MI355ENC_OK; } /* hold: dropped; blend: kept, it is the next pair's p0 */
        if (cnt - 1 > pl->max_fill) anchor = *resync = 1;
        else {
            for (int i = 0; i < (int)cnt; i++) {
                out_pts[i] = rate_tick_pts(pl, pl->k_next + i);
                weight[i] = pl->mode == 1 ? (i == (int)cnt - 1 ? 256 : 0) : blend_weight(pl, (i128)pl->k_next + i, pl->prev_pts, pts);
            }
            *n = (int)cnt;
            pl->k_next = (int64_t)(k_max + 1);
        }
    }
    if (anchor) { pl->started = 1; pl->t0 = pts; pl->k_next = 1; *n = 1; out_pts[0] = pts; weight[0] = 256; }
    pl->prev_pts = pts;
    return MI355ENC_OK;
}
