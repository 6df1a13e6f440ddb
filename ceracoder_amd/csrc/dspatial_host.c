/* dspatial_host.c -- the rule of the spatial noise filter on the host: setting, tables, filter, noise measurement and decision as the
 * ABI exposes them (mi355enc_denoise_spatial_*).  The kernels of k_dspatial.hip compute the same numbers; tests/dspatialref.py restates them in numpy. */
#include "dspatial_host.h"

#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355enc.h"

void mi355enc_denoise_spatial_default(mi355enc_denoise_spatial_t *a) {
    if (!a) return;
    a->luma = 0; a->chroma = 0; a->auto_gain = 0; a->percentile = 25; a->speed = 32;
}

int mi355enc_denoise_spatial_check(const mi355enc_denoise_spatial_t *a) {
    if (!a || a->luma < 0 || a->luma > DS_MAX || a->chroma < 0 || a->chroma > DS_MAX) return MI355ENC_ERR_ARG;
    if (a->auto_gain != 0 && (a->auto_gain < 250 || a->auto_gain > 8000)) return MI355ENC_ERR_ARG;
    if (a->percentile < 1 || a->percentile > 50 || a->speed < 1 || a->speed > 256) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

int mi355enc_denoise_spatial_tables(int s, uint8_t weight[256], uint16_t filter[256]) {
    if (s < 0 || s > DS_MAX || (!weight && !filter)) return MI355ENC_ERR_ARG;
    for (int a = 0; a < 256; a++) {
        const int r = ds_weight(s, a);
        if (weight) weight[a] = (uint8_t)r;
        if (filter) filter[a] = (uint16_t)(a * r);
    }
    return MI355ENC_OK;
}

static int rect_ok(int W, int H, const int rect[4], int vw, int vh) {
    if (W < 16 || H < 2 || W > 8192 || H > 8192 || (W & 15) || (H & 1) || !rect) return 0;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return 0;
    return vw >= 1 && vh >= 1 && vw <= W && vh <= H && rect[0] < vw && rect[2] < vh;
}

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

/* one plane of the filter: src -> dst over rows y0 .. y1 - 1 and bytes x0 .. x1 - 1 at stride W, visible up to (vx1, vy1) exclusive; step 1 / radius 2 (luma) or
 * step 2 / radius 1 (the interleaved chroma plane: Cb and Cr each for itself) */
static void filter_plane(const uint8_t *src, uint8_t *dst, int W, int x0, int x1, int y0, int y1, int vx1, int vy1, int s, int step, int rad) {
    static const int w5[5] = {1, 4, 6, 4, 1}, w3[3] = {1, 2, 1};
    const int *w = rad == 2 ? w5 : w3, shift = rad == 2 ? 12 : 8;
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) {
            const int p = x & (step - 1), yc = clampi(y, y0, vy1 - 1), xc = clampi(x - p, x0, vx1 - step) + p;
            const int c = src[(size_t)yc * W + xc];
            int sum = 0;
            for (int dy = -rad; dy <= rad; dy++)
                for (int dx = -rad; dx <= rad; dx++) {
                    const int yy = clampi(yc + dy, y0, vy1 - 1), xx = clampi(xc - p + step * dx, x0, vx1 - step) + p;
                    const int d = (int)src[(size_t)yy * W + xx] - c, a = d < 0 ? -d : d, f = a * ds_weight(s, a);
                    sum += w[dy + rad] * w[dx + rad] * (d < 0 ? -f : f);
                }
            dst[(size_t)y * W + x] = (uint8_t)(c + ds_floor_shr(sum + (1 << (shift - 1)), shift));
        }
}

int mi355enc_denoise_spatial_apply_host(uint8_t *y, uint8_t *uv, int W, int H, const int rect[4], int vw, int vh, int s_luma, int s_chroma) {
    if (!y || !uv || !rect_ok(W, H, rect, vw, vh) || s_luma < -1 || s_luma > DS_MAX || s_chroma < -1 || s_chroma > DS_MAX) return MI355ENC_ERR_ARG;
    const size_t ysz = (size_t)W * H;
    uint8_t *tmp = (uint8_t *)malloc(ysz);
    if (!tmp) return MI355ENC_ERR_NOMEM;
    const int vx1 = rect[1] < vw ? rect[1] : vw, vy1 = rect[3] < vh ? rect[3] : vh;
    if (s_luma >= 0) {
        memcpy(tmp, y, ysz);
        filter_plane(tmp, y, W, rect[0], rect[1], rect[2], rect[3], vx1, vy1, s_luma, 1, 2);
    }
    if (s_chroma >= 0) {
        memcpy(tmp, uv, ysz / 2);
        filter_plane(tmp, uv, W, rect[0], rect[1], rect[2] >> 1, rect[3] >> 1, (vx1 + 1) & ~1, (vy1 + 1) >> 1, s_chroma, 2, 1);
    }
    free(tmp);
    return MI355ENC_OK;
}

int mi355enc_denoise_spatial_measure_host(const uint8_t *y, int W, int H, const int rect[4], int vw, int vh, int full_range, mi355enc_denoise_spatial_meas_t *m) {
    if (!y || !m || !rect_ok(W, H, rect, vw, vh)) return MI355ENC_ERR_ARG;
    int bx0, bcols, by0, brows;
    ds_blocks(rect, vw, vh, &bx0, &bcols, &by0, &brows);
    const int B = ds_black(full_range), S = ds_scale(full_range), lo = ds_vote_lo(B, S), hi = ds_vote_hi(B, S);
    memset(m, 0, sizeof *m);
    m->candidates = (uint32_t)bcols * (uint32_t)brows;
    for (int by = by0; by < by0 + brows; by++)
        for (int bx = bx0; bx < bx0 + bcols; bx++) {
            const uint8_t *p = y + (size_t)(8 * by) * W + 8 * bx;
            int sum = 0, A = 0;
            for (int r = 0; r < 8; r++)
                for (int c = 0; c < 8; c++) sum += p[(size_t)r * W + c];
            for (int r = 1; r < 7; r++)
                for (int c = 1; c < 7; c++) {
                    const uint8_t *q = p + (size_t)r * W + c;
                    const int L = (q[-W - 1] - 2 * q[-W] + q[-W + 1]) - 2 * (q[-1] - 2 * q[0] + q[1]) + (q[W - 1] - 2 * q[W] + q[W + 1]);
                    A += L < 0 ? -L : L;
                }
            if (sum >= lo && sum <= hi) { m->hist[ds_bin(A)]++; m->voters++; }
        }
    return MI355ENC_OK;
}

int mi355enc_denoise_spatial_decide(const mi355enc_denoise_spatial_meas_t *m, const mi355enc_denoise_spatial_t *a, int prime, int32_t *x, mi355enc_denoise_spatial_info_t *info) {
    if (!m || !x || !info || mi355enc_denoise_spatial_check(a) || a->auto_gain == 0) return MI355ENC_ERR_ARG;
    if (m->candidates > (1u << 20) || m->voters > m->candidates || (!prime && (*x < 0 || *x > DS_X_MAX))) return MI355ENC_ERR_ARG;
    uint64_t N = 0, cum = 0;
    for (int v = 0; v < 256; v++) N += m->hist[v];
    if (N != m->voters) return MI355ENC_ERR_ARG;
    int v = 0;
    for (; v < 255; v++) {
        cum += m->hist[v];
        if (ds_is_v(cum, N, a->percentile)) break;
    }
    const int set[5] = {a->luma, a->chroma, a->auto_gain, a->percentile, a->speed};
    int X = *x, rec[DS_REC_WORDS];
    ds_decide(m->candidates, m->voters, v, set, prime ? 1 : 0, &X, rec);
    *x = X;
    info->candidates = rec[0]; info->voters = rec[1]; info->v = rec[2]; info->valid = rec[3]; info->x = rec[4]; info->s_luma = rec[5]; info->s_chroma = rec[6]; info->reserved = 0;
    return MI355ENC_OK;
}
