/* stab_host.c -- the stabiliser's rule on the host: setting, projections, vote, motion and trajectory step as the ABI exposes them
 * (mi355enc_stabilize_*).  The kernels of k_stab.hip compute the same numbers; tests/stabref.py restates them in numpy. */
#include "stab_host.h"

#include <stddef.h>
#include <string.h>

#include "../../include/mi355enc.h"

void mi355enc_stabilize_default(mi355enc_stabilize_t *s) {
    if (!s) return;
    s->range = 0; s->leak = 16; s->margin_x = 0; s->margin_y = 0; /* off; a caller that turns it on sets the range (16 by convention) */
}

int mi355enc_stabilize_check(const mi355enc_stabilize_t *s) {
    if (!s || s->range < 0 || s->range > MI355ENC_STABILIZE_RANGE_MAX || s->leak < 0 || s->leak > 255) return MI355ENC_ERR_ARG;
    if (s->margin_x < 0 || s->margin_x > MI355ENC_STABILIZE_MARGIN_MAX || s->margin_y < 0 || s->margin_y > MI355ENC_STABILIZE_MARGIN_MAX || ((s->margin_x | s->margin_y) & 1)) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

int mi355enc_stabilize_project(const uint8_t *luma, int stride, int step, int w, int h, uint32_t *sums) {
    if (!luma || !sums || w < 1 || h < 1 || w > 8192 || h > 8192 || (step != 1 && step != 2) || stride < (w - 1) * step + 1) return MI355ENC_ERR_ARG;
    uint32_t *col = sums, *row = sums + (size_t)STAB_BANDS * w;
    memset(sums, 0, (size_t)STAB_BANDS * ((size_t)w + h) * sizeof *sums);
    for (int k = 0; k < STAB_BANDS; k++)
        for (int y = stab_band(k, h); y < stab_band(k + 1, h); y++) {
            const uint8_t *p = luma + (size_t)y * stride;
            for (int x = 0; x < w; x++) col[(size_t)k * w + x] += p[(size_t)x * step];
        }
    for (int k = 0; k < STAB_BANDS; k++)
        for (int y = 0; y < h; y++) {
            const uint8_t *p = luma + (size_t)y * stride;
            uint32_t s = 0;
            for (int x = stab_band(k, w); x < stab_band(k + 1, w); x++) s += p[(size_t)x * step];
            row[(size_t)k * h + y] = s;
        }
    return MI355ENC_OK;
}

int mi355enc_stabilize_vote(const uint32_t *p, const uint32_t *q, int n, int range, int *d_out) {
    if (!p || !q || !d_out || range < 1 || range > MI355ENC_STABILIZE_RANGE_MAX || n < 4 * range || n > 8192) return MI355ENC_ERR_ARG;
    uint64_t best = 0;
    int at = 0, ties = 0;
    for (int d = -range; d <= range; d++) {
        uint64_t c = 0; /* exact: up to 8192 terms of up to 2048 * 255 */
        for (int x = range; x < n - range; x++) { const uint32_t a = p[x], b = q[x - d]; c += a > b ? a - b : b - a; }
        if (d == -range || c < best) { best = c; at = d; ties = 0; }
        else if (c == best) ties++;
    }
    *d_out = at;
    return !ties && at > -range && at < range ? 1 : 0;
}

int mi355enc_stabilize_motion(const int *votes, int count, int *m) {
    if (!m || count < 0 || count > STAB_BANDS || (count && !votes)) return MI355ENC_ERR_ARG;
    int v[STAB_BANDS];
    for (int i = 0; i < count; i++) v[i] = votes[i];
    *m = stab_median(v, count);
    return MI355ENC_OK;
}

int mi355enc_stabilize_step(int S, int m, int leak, int lo, int hi, int *S_out, int *o) {
    if (!S_out || !o || leak < 0 || leak > 255 || lo > 0 || hi < 0 || lo < -MI355ENC_STABILIZE_MARGIN_MAX || hi > MI355ENC_STABILIZE_MARGIN_MAX || ((lo | hi) & 1)) return MI355ENC_ERR_ARG;
    if (m < -MI355ENC_STABILIZE_RANGE_MAX || m > MI355ENC_STABILIZE_RANGE_MAX || S < -256 * MI355ENC_STABILIZE_MARGIN_MAX || S > 256 * MI355ENC_STABILIZE_MARGIN_MAX) return MI355ENC_ERR_ARG;
    stab_step(S, m, leak, lo, hi, S_out, o);
    return MI355ENC_OK;
}
