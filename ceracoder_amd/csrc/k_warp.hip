// k_warp.hip -- lens, roll and keystone correction: the coded NV12 picture resampled through a coarse mesh of source positions, bilinear
// or bicubic, in integers.  The rule is warp_host.h's (mesh interpolation, rounding, taps, the outside test, the filter), shared with the host statement
// warp_host.c: this file only decides which lane computes which sample.  One launch per picture, both planes.
//
// A workgroup of 256 owns a 32 x 32 luma tile of the coded surface and its 16 x 16 chroma pairs.  A lane takes four luma samples of one row (one aligned
// dword store) and one chroma pair (one 16-bit store).  The four luma samples lie in one mesh cell, so the position is interpolated once and stepped by the
// row's constant from sample to sample.
// Two forms, chosen per workgroup by warp_window's test (uniform; mi355enc_warp_plan states the same test on the host), both computing the same result:
//   staged   the tile's source window (warp_host.h: from the smallest and largest node over the tile's cells) fits the LDS room -- 64 x 64 luma, 36 x 36 pairs --
//            and is loaded once, whole dwords at natural alignment and the dwords that reach behind the visible width byte by byte (pair by pair); every tap is
//            then an LDS read.  Luma rows are 17 dwords apart, chroma rows 19: odd, so the rows a lane's four tap rows touch fall on different banks
//   direct   the window does not fit (a strong shrink, a folded mesh): the taps come from global memory
// Tap positions clamp to the visible picture in both; nothing outside it is ever read.
// Margin up to W x H (pad_kernel's rule: the last visible column / row, chroma the last pair): a margin sample is computed at the clamped output position, so
// the launch writes every byte of both surfaces and the caller may exchange them for the source's.  No workgroup waits for another, no atomic.
#include "kernels_common.hpp"
#include "warp_host.h"

#define WT WARP_TILE /* luma tile edge */
#define LY_PITCH 17    /* dwords per LDS luma row: 64 columns and up to 3 in front of them (the window starts at a dword) */
#define LC_PITCH 19    /* dwords per LDS chroma row: 36 pairs and one in front */

struct warp_args {
    const uint8_t *sy, *suv; // source surfaces, stride W
    uint8_t *dy, *duv;       // destination surfaces, stride W
    const int32_t *mesh;     // nx x ny nodes {sx, sy}
    int w, h, W, H, nx, kind, staging; // staging 0: every workgroup takes the direct form (measurements)
    unsigned fill_y, fill_uv; // Y; Cb | Cr << 8
};

// where a form's taps come from: global memory, or the window in LDS (its first row wy0, first column wa -- the window's own rounded down to a dword -- and
// its extent [wx0, wx1] x [wy0, wy1], which a tap that weighs nothing may leave: it reads the nearest element inside)
struct warp_src { const uint8_t *g; int stride; const unsigned *lds; int wa, wx0, wx1, wy0, wy1; };

// the pair (or, es 1, the sample) at (px, py) of a pw x ph plane, taps clamped; the same sums as warp_filter, both components of a pair from one pass.  o0 / o1:
// the values before the clip to a byte (they fit 16 bits: at most 160 * 160 * 255 >> 14), which the caller packs through csc_pack4
template <int ES, bool STAGED> DEV void warp_sample(const warp_src &s, int pw, int ph, int px, int py, int kind, unsigned fill, int &o0, int &o1) {
    if (warp_outside(px, py, pw, ph)) { o0 = (int)(fill & 255u); o1 = (int)(fill >> 8); return; }
    const int ix = px >> 5, iy = py >> 5;
    int cx[4], cy[4], a0 = 0, a1 = 0;
    warp_taps(kind, px & 31, cx);
    warp_taps(kind, py & 31, cy);
    const int lo = kind ? 0 : 1, hi = kind ? 4 : 3;
    for (int r = lo; r < hi; r++) {
        int yy = warp_clampi(iy - 1 + r, 0, ph - 1), t0 = 0, t1 = 0;
        if (STAGED) yy = warp_clampi(yy, s.wy0, s.wy1);
        const uint8_t *row = STAGED ? (const uint8_t *)(s.lds + (yy - s.wy0) * (ES == 1 ? LY_PITCH : LC_PITCH)) : s.g + (size_t)yy * s.stride;
        for (int k = lo; k < hi; k++) {
            int xx = warp_clampi(ix - 1 + k, 0, pw - 1);
            if (STAGED) xx = warp_clampi(xx, s.wx0, s.wx1) - s.wa;
            if (ES == 1) t0 += cx[k] * (STAGED ? (int)row[xx] : (int)ldg8(row + xx));
            else {
                const unsigned v = STAGED ? (unsigned)((const uint16_t *)row)[xx] : (unsigned)ldg16(row + 2 * (size_t)xx) & 0xffffu;
                t0 += cx[k] * (int)(v & 255u); t1 += cx[k] * (int)(v >> 8);
            }
        }
        a0 += cy[r] * t0; a1 += cy[r] * t1;
    }
    o0 = (a0 + 8192) >> 14; o1 = (a1 + 8192) >> 14;
}

// rows x nd dwords of a plane's window into LDS (pitch dwords per row): the dword at byte xb of a row whole where all of it is visible (below vis bytes), else
// its visible bytes alone -- es at a time -- and zeros behind them
template <int ES> DEV void warp_stage(const uint8_t *src, int stride, int vis, int row0, int rows, int xb0, int nd, int pitch, unsigned *lds) {
    for (int idx = threadIdx.x; idx < rows * nd; idx += 256) {
        const int r = idx / nd, c = idx - r * nd, xb = xb0 + 4 * c;
        const uint8_t *p = src + (size_t)(row0 + r) * stride + xb;
        unsigned v = 0;
        if (xb + 4 <= vis) v = ldg32(p);
        else if (ES == 1) { for (int b = 0; b < 4; b++) if (xb + b < vis) v |= ldg8(p + b) << (8 * b); }
        else if (xb + 2 <= vis) v = (unsigned)ldg16(p) & 0xffffu;
        lds[r * pitch + c] = v;
    }
}

template <bool STAGED> DEV void warp_tile(const warp_args &a, const warp_src &ly, const warp_src &lc) {
    const int t = threadIdx.x, bx = blockIdx.x * WT, by = blockIdx.y * WT;
    { // luma: four samples of a row
        const int x0 = bx + 4 * (t & 7), y = by + (t >> 3);
        if (x0 < a.W && y < a.H) { // (W is a multiple of 16: a dword is all inside or all outside)
            const int yc = y < a.h ? y : a.h - 1, xs = x0 < a.w ? x0 : a.w - 1; // (margin: the clamped output position)
            int dX, dY;
            int X = warp_point(a.mesh, a.nx, xs, yc, 0, &dX), Y = warp_point(a.mesh, a.nx, xs, yc, 1, &dY);
            int v[4], unused;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (k && x0 + k < a.w) { X += dX; Y += dY; } // (x0 .. x0 + 3 share a cell; behind the last visible column the position stays)
                warp_sample<1, STAGED>(ly, a.w, a.h, warp_round_luma(X), warp_round_luma(Y), a.kind, a.fill_y, v[k], unused);
            }
            stg32(a.dy + (size_t)y * a.W + x0, csc_pack4(v[0], v[1], v[2], v[3]));
        }
    }
    { // chroma: one pair
        const int cx = (bx >> 1) + (t & 15), cy = (by >> 1) + (t >> 4);
        if (cx < (a.W >> 1) && cy < (a.H >> 1)) {
            const int cw = a.w >> 1, ch = a.h >> 1, xc = cx < cw ? cx : cw - 1, yc = cy < ch ? cy : ch - 1;
            const int X = warp_point(a.mesh, a.nx, 2 * xc, 2 * yc, 0, nullptr), Y = warp_point(a.mesh, a.nx, 2 * xc, 2 * yc, 1, nullptr);
            int cb, cr;
            warp_sample<2, STAGED>(lc, cw, ch, warp_round_chroma(X), warp_round_chroma(Y), a.kind, a.fill_uv, cb, cr);
            stg16(a.duv + (size_t)cy * a.W + 2 * cx, (int)(csc_pack4(cb, cr, 0, 0) & 0xffffu));
        }
    }
}

__global__ __launch_bounds__(256) void warp_kernel(const warp_args a) {
    __shared__ unsigned lds_y[WARP_ROOM_Y * LY_PITCH], lds_c[WARP_ROOM_C * LC_PITCH];
    warp_src ly = {a.sy, a.W, lds_y, 0, 0, 0, 0, 0}, lc = {a.suv, a.W, lds_c, 0, 0, 0, 0, 0};
    warp_window_t win;
    warp_window(a.mesh, a.nx, a.w, a.h, blockIdx.x, blockIdx.y, &win); // (from the block's index and uniform loads: the branch is the workgroup's)
    if (a.staging && win.staged) {
        ly.wa = win.x0 & ~3; ly.wx0 = win.x0; ly.wx1 = win.x1; ly.wy0 = win.y0; ly.wy1 = win.y1;
        lc.wa = win.cx0 & ~1; lc.wx0 = win.cx0; lc.wx1 = win.cx1; lc.wy0 = win.cy0; lc.wy1 = win.cy1;
        warp_stage<1>(a.sy, a.W, a.w, win.y0, win.y1 - win.y0 + 1, ly.wa, ((win.x1 - ly.wa) >> 2) + 1, LY_PITCH, lds_y);
        warp_stage<2>(a.suv, a.W, a.w, win.cy0, win.cy1 - win.cy0 + 1, 2 * lc.wa, ((win.cx1 - lc.wa) >> 1) + 1, LC_PITCH, lds_c);
        __syncthreads();
        warp_tile<true>(a, ly, lc);
    } else
        warp_tile<false>(a, ly, lc);
}

// w x h (even, >= 2): the coded visible size; W x H: the coded size; mesh: warp_nodes(w) x warp_nodes(h) valid nodes on the device; the surfaces are 4-byte
// aligned and dy / duv are not sy / suv; staging 0: the direct form everywhere.  -1: arguments outside that
int k_launch_warp(const uint8_t *sy, const uint8_t *suv, uint8_t *dy, uint8_t *duv, int w, int h, int W, int H, const int32_t *mesh, int kind, const uint8_t fill[3], hipStream_t s, int staging) {
    if (!sy || !suv || !dy || !duv || !mesh || !fill || w < 2 || h < 2 || ((w | h) & 1) || ((W | H) & 15) || w > W || h > H || W > 8192 + 15 || H > 8192 + 15 || (kind != 0 && kind != 1) ||
        sy == dy || suv == duv || (((uintptr_t)dy | (uintptr_t)duv | (uintptr_t)sy | (uintptr_t)suv) & 3))
        return -1;
    warp_args a;
    a.sy = sy; a.suv = suv; a.dy = dy; a.duv = duv; a.mesh = mesh; a.w = w; a.h = h; a.W = W; a.H = H; a.nx = warp_nodes(w); a.kind = kind; a.staging = staging;
    a.fill_y = fill[0]; a.fill_uv = (unsigned)fill[1] | (unsigned)fill[2] << 8;
    hipLaunchKernelGGL(warp_kernel, dim3((unsigned)((W + WT - 1) / WT), (unsigned)((H + WT - 1) / WT)), dim3(256), 0, s, a);
    return 0;
}
