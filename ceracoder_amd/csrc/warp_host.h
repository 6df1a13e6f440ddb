/* warp_host.h -- the mesh warp's rule in plain C, all integers: what the host entry points of the ABI (mi355enc_warp_*, warp_host.c),
 * the handle (enc_warp.cpp) and the kernel (k_warp.hip) share.  No device needed.
 *   mesh       nx = (w + 15) / 16 + 1 by ny = (h + 15) / 16 + 1 nodes, node (i, j) at int32 index 2 (j nx + i): the source position {sx, sy} of the output luma
 *              sample (16 i, 16 j) in 1/256 luma sample, each inside [WARP_NODE_MIN, WARP_NODE_MAX]
 *   position   bilinear inside a cell, in 1/65536 sample (below 2^31 by the node range), rounded to 1/32 sample of the plane
 *   filter     four taps per axis, weights over 128, separable with no rounding in between; tap positions clamp to the visible plane
 *   outside    a sample whose first whole position is below -1 or behind the last column / row takes the fill value */
#ifndef MI355_WARP_HOST_H
#define MI355_WARP_HOST_H
#include <stdint.h>

#define WARP_NODE_MIN (-2048 * 256)
#define WARP_NODE_MAX (10240 * 256)
/* the builder's bound on q (the squared radius over the squared half diagonal, Q16): 64, a radius of eight half diagonals.  With it, for sizes up to 8192,
 * |U| <= 2^19 sqrt(R2) < 2^33, g < 2^16 + 2^22 + 2^28 < 2^29, and U g stays below 2^62 */
#define WARP_Q_MAX 4194304

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WARP_FN static __host__ __device__ inline
#else
#define WARP_FN static inline
#endif

/* every >> of a negative value below is meant as a floor: so the compilers this builds with make it */
#if defined(__cplusplus)
static_assert((-1 >> 1) == -1, "arithmetic right shift");
#else
_Static_assert((-1 >> 1) == -1, "arithmetic right shift");
#endif

WARP_FN int warp_nodes(int n) { return (n + 15) / 16 + 1; }
WARP_FN int warp_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

/* the four taps of fraction f (0 .. 31): kind 0 bilinear, otherwise Catmull-Rom; they add up to 128 */
WARP_FN void warp_taps(int kind, int f, int c[4]) {
    if (!kind) { c[0] = 0; c[1] = 4 * (32 - f); c[2] = 4 * f; c[3] = 0; return; }
    const int f2 = f * f, f3 = f2 * f;
    c[0] = (-f3 + 64 * f2 - 1024 * f + 256) >> 9;
    c[2] = (-3 * f3 + 128 * f2 + 1024 * f + 256) >> 9;
    c[3] = (f3 - 32 * f2 + 256) >> 9;
    c[1] = 128 - c[0] - c[2] - c[3];
}

/* one coordinate (comp 0: x, 1: y) at the luma point (x, y), in 1/65536 sample; *dx: what it changes by from x to x + 1 inside the cell */
WARP_FN int warp_point(const int32_t *mesh, int nx, int x, int y, int comp, int *dx) {
    const int i = x >> 4, j = y >> 4, xf = x & 15, yf = y & 15;
    const int32_t *n = mesh + 2 * ((long)j * nx + i) + comp;
    const int n00 = n[0], n01 = n[2], n10 = n[2 * nx], n11 = n[2 * nx + 2];
    if (dx) *dx = (16 - yf) * (n01 - n00) + yf * (n11 - n10);
    return (16 - yf) * ((16 - xf) * n00 + xf * n01) + yf * ((16 - xf) * n10 + xf * n11);
}
/* ... rounded to 1/32 sample of the luma / of the chroma plane */
WARP_FN int warp_round_luma(int P) { return (P + 1024) >> 11; }
WARP_FN int warp_round_chroma(int P) { return (P + 2048) >> 12; }

/* The source window of a 32 x 32 output tile (tx, ty): the position inside a cell is a convex combination of the cell's four nodes, so with lo / hi the smallest
 * and largest node value over the tile's visible cells, 65536 (lo >> 8) <= P <= 65536 ((hi >> 8) + 1) - 256, the rounded position's whole part lies in
 * [lo >> 8, (hi >> 8) + 1] (at the upper end only with f = 0, where the two taps behind it weigh nothing), and every tap that weighs lies in
 * [(lo >> 8) - 1, (hi >> 8) + 2]; the chroma plane likewise with >> 9.  Clamped to the visible plane.  staged: both windows fit the kernel's LDS room */
#define WARP_TILE 32
#define WARP_ROOM_Y 64 /* luma window: rows and columns */
#define WARP_ROOM_C 36 /* chroma window: rows and pairs (half the luma span, plus the same four) */
typedef struct { int x0, x1, y0, y1, cx0, cx1, cy0, cy1, staged; } warp_window_t;
WARP_FN void warp_window(const int32_t *mesh, int nx, int w, int h, int tx, int ty, warp_window_t *o) {
    const int xe = WARP_TILE * tx + WARP_TILE - 1 < w - 1 ? WARP_TILE * tx + WARP_TILE - 1 : w - 1, ye = WARP_TILE * ty + WARP_TILE - 1 < h - 1 ? WARP_TILE * ty + WARP_TILE - 1 : h - 1;
    int lo[2] = {WARP_NODE_MAX, WARP_NODE_MAX}, hi[2] = {WARP_NODE_MIN, WARP_NODE_MIN};
    for (int j = 2 * ty; j <= (ye >> 4) + 1; j++)
        for (int i = 2 * tx; i <= (xe >> 4) + 1; i++)
            for (int c = 0; c < 2; c++) {
                const int v = mesh[2 * ((long)j * nx + i) + c];
                lo[c] = v < lo[c] ? v : lo[c]; hi[c] = v > hi[c] ? v : hi[c];
            }
    o->x0 = warp_clampi((lo[0] >> 8) - 1, 0, w - 1); o->x1 = warp_clampi((hi[0] >> 8) + 2, 0, w - 1);
    o->y0 = warp_clampi((lo[1] >> 8) - 1, 0, h - 1); o->y1 = warp_clampi((hi[1] >> 8) + 2, 0, h - 1);
    o->cx0 = warp_clampi((lo[0] >> 9) - 1, 0, w / 2 - 1); o->cx1 = warp_clampi((hi[0] >> 9) + 2, 0, w / 2 - 1);
    o->cy0 = warp_clampi((lo[1] >> 9) - 1, 0, h / 2 - 1); o->cy1 = warp_clampi((hi[1] >> 9) + 2, 0, h / 2 - 1);
    o->staged = o->x1 - o->x0 < WARP_ROOM_Y && o->y1 - o->y0 < WARP_ROOM_Y && o->cx1 - o->cx0 < WARP_ROOM_C && o->cy1 - o->cy0 < WARP_ROOM_C;
}

/* whether the sample at (px, py) (1/32 sample) of a pw x ph plane takes the fill value */
WARP_FN int warp_outside(int px, int py, int pw, int ph) {
    const int ix = px >> 5, iy = py >> 5;
    return ix < -1 || ix > pw - 1 || iy < -1 || iy > ph - 1;
}
/* the filtered value of component `c` of a plane whose elements are `es` bytes (1 luma, 2 a chroma pair) at (px, py), not outside */
WARP_FN int warp_filter(const uint8_t *src, long stride, int pw, int ph, int es, int c, int px, int py, int kind) {
    const int ix = px >> 5, iy = py >> 5;
    int cx[4], cy[4], a = 0;
    warp_taps(kind, px & 31, cx);
    warp_taps(kind, py & 31, cy);
    const int lo = kind ? 0 : 1, hi = kind ? 4 : 3; /* (the bilinear filter's outer taps weigh nothing) */
    for (int r = lo; r < hi; r++) {
        const uint8_t *row = src + (long)warp_clampi(iy - 1 + r, 0, ph - 1) * stride + c;
        int t = 0;
        for (int k = lo; k < hi; k++) t += cx[k] * row[(long)warp_clampi(ix - 1 + k, 0, pw - 1) * es];
        a += cy[r] * t;
    }
    return warp_clampi((a + 8192) >> 14, 0, 255);
}
#endif
