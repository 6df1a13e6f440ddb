/* warp_host.c -- the mesh warp's rule (warp_host.h) as the ABI's host entry points: the coefficient table, the mesh's size and check,
 * the builder (seven Q16 integers -> a mesh, in 64-bit arithmetic) and the scalar form of the whole warp.  No device needed. */
#include "warp_host.h"

#include <stddef.h>

#include "../../include/mi355enc.h"

/* a / b rounded towards minus infinity, b > 0 */
static int64_t fdiv(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b) < 0 ? q - 1 : q; }

void mi355enc_warp_params_default(mi355enc_warp_params_t *p) {
    if (!p) return;
    p->k1 = p->k2 = 0; p->zoom = 65536; p->cos = 65536; p->sin = 0; p->kh = p->kv = 0;
}

int mi355enc_warp_coeff(int kind, int f, int16_t c[4]) {
    if ((kind != 0 && kind != 1) || f < 0 || f > 31 || !c) return MI355ENC_ERR_ARG;
    int t[4];
    warp_taps(kind, f, t);
    for (int k = 0; k < 4; k++) c[k] = (int16_t)t[k];
    return MI355ENC_OK;
}

int mi355enc_warp_mesh_size(int w, int h, int *nx, int *ny) {
    if (w < 2 || h < 2 || w > 8192 || h > 8192 || !nx || !ny) return MI355ENC_ERR_ARG;
    *nx = warp_nodes(w); *ny = warp_nodes(h);
    return MI355ENC_OK;
}

int mi355enc_warp_mesh_check(const int32_t *mesh, int nx, int ny) {
    if (!mesh || nx < 2 || ny < 2) return MI355ENC_ERR_ARG;
    for (size_t k = 0; k < (size_t)2 * nx * ny; k++)
        if (mesh[k] < WARP_NODE_MIN || mesh[k] > WARP_NODE_MAX) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

static int in_range(int v, int lo, int hi) { return v >= lo && v <= hi; }

int mi355enc_warp_build(const mi355enc_warp_params_t *p, int w, int h, int32_t *mesh, size_t cap) {
    int nx, ny;
    if (!p || !mesh || mi355enc_warp_mesh_size(w, h, &nx, &ny) || cap < (size_t)2 * nx * ny) return MI355ENC_ERR_ARG;
    if (!in_range(p->k1, -65536, 65536) || !in_range(p->k2, -65536, 65536) || !in_range(p->zoom, 16384, 262144) || !in_range(p->cos, -65536, 65536) ||
        !in_range(p->sin, -65536, 65536) || !in_range(p->kh, -32768, 32768) || !in_range(p->kv, -32768, 32768))
        return MI355ENC_ERR_ARG;
    const int64_t R2 = (int64_t)(w - 1) * (w - 1) + (int64_t)(h - 1) * (h - 1);
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            const int64_t u = 32 * i - (w - 1), v = 32 * j - (h - 1); /* half samples from the centre */
            int64_t U = (p->zoom * (p->cos * u - p->sin * v)) >> 16, V = (p->zoom * (p->sin * u + p->cos * v)) >> 16;
            const int64_t d = 65536 + fdiv(p->kh * U, (int64_t)(w - 1) * 65536) + fdiv(p->kv * V, (int64_t)(h - 1) * 65536);
            if (d < 16384) return MI355ENC_ERR_ARG;
            U = fdiv(U * 65536, d); V = fdiv(V * 65536, d);
            const int64_t r2 = ((U >> 8) * (U >> 8) + (V >> 8) * (V >> 8)) >> 16, q = fdiv(r2 * 65536, R2);
            if (q > WARP_Q_MAX) return MI355ENC_ERR_ARG; /* (keeps U g inside 64 bits) */
            const int64_t g = 65536 + ((p->k1 * q) >> 16) + ((p->k2 * ((q * q) >> 16)) >> 16);
            const int64_t sx = ((int64_t)(w - 1) * 65536 + ((U * g) >> 16) + 256) >> 9, sy = ((int64_t)(h - 1) * 65536 + ((V * g) >> 16) + 256) >> 9;
            if (sx < WARP_NODE_MIN || sx > WARP_NODE_MAX || sy < WARP_NODE_MIN || sy > WARP_NODE_MAX) return MI355ENC_ERR_ARG;
            mesh[2 * ((size_t)j * nx + i)] = (int32_t)sx;
            mesh[2 * ((size_t)j * nx + i) + 1] = (int32_t)sy;
        }
    return MI355ENC_OK;
}

int mi355enc_warp_plan(const int32_t *mesh, int nx, int ny, int w, int h, int *staged, int *direct) {
    int mx, my;
    if (!staged || !direct || mi355enc_warp_mesh_size(w, h, &mx, &my) || ((w | h) & 1) || nx != mx || ny != my || mi355enc_warp_mesh_check(mesh, nx, ny)) return MI355ENC_ERR_ARG;
    *staged = *direct = 0;
    for (int ty = 0; ty < (((h + 15) & ~15) + WARP_TILE - 1) / WARP_TILE; ty++)
        for (int tx = 0; tx < (((w + 15) & ~15) + WARP_TILE - 1) / WARP_TILE; tx++) {
            warp_window_t win;
            warp_window(mesh, nx, w, h, tx, ty, &win);
            if (win.staged) (*staged)++; else (*direct)++;
        }
    return MI355ENC_OK;
}

int mi355enc_warp_apply_host(const mi355enc_warp_t *s, const int32_t *mesh, int w, int h, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride,
                             uint8_t *out_y, int out_y_stride, uint8_t *out_uv, int out_uv_stride) {
    int nx, ny;
    if (!s || (s->kind != 0 && s->kind != 1) || !y || !uv || !out_y || !out_uv || mi355enc_warp_mesh_size(w, h, &nx, &ny) || ((w | h) & 1) ||
        y_stride < w || uv_stride < w || out_y_stride < w || out_uv_stride < w || mi355enc_warp_mesh_check(mesh, nx, ny))
        return MI355ENC_ERR_ARG;
    for (int py = 0; py < h; py++)
        for (int px = 0; px < w; px++) {
            const int X = warp_round_luma(warp_point(mesh, nx, px, py, 0, NULL)), Y = warp_round_luma(warp_point(mesh, nx, px, py, 1, NULL));
            out_y[(size_t)py * out_y_stride + px] = warp_outside(X, Y, w, h) ? s->fill[0] : (uint8_t)warp_filter(y, y_stride, w, h, 1, 0, X, Y, s->kind);
        }
    for (int cy = 0; cy < h / 2; cy++)
        for (int cx = 0; cx < w / 2; cx++) {
            const int X = warp_round_chroma(warp_point(mesh, nx, 2 * cx, 2 * cy, 0, NULL)), Y = warp_round_chroma(warp_point(mesh, nx, 2 * cx, 2 * cy, 1, NULL));
            uint8_t *o = out_uv + (size_t)cy * out_uv_stride + 2 * cx;
            const int out = warp_outside(X, Y, w / 2, h / 2);
            for (int c = 0; c < 2; c++) o[c] = out ? s->fill[1 + c] : (uint8_t)warp_filter(uv, uv_stride, w / 2, h / 2, 2, c, X, Y, s->kind);
        }
    return MI355ENC_OK;
}
