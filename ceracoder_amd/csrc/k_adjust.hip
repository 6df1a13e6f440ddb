// k_adjust.hip -- picture controls on the coded NV12 surfaces of a slot: a luma table (brightness, contrast, gamma), a chroma rotation
// (saturation, hue) and a 3 x 3 unsharp mask on the luma behind the table.  Two forms, chosen by the host:
//
//   pointwise (sharpen = 0)   in place, with yuv_convert_kernel's ownership: a thread owns an 8 x 2 luma patch and its four chroma pairs, reads all of them before
//                             it writes any, and no other thread touches them.  LUMA / CHROMA say which planes are not neutral: the other one is not touched.
//   stencil (sharpen != 0)    luma only, from the slot's plane into a scratch plane (a halo sample belongs to a neighbouring workgroup, which may have written it
//                             already: not in place).  A workgroup stages a 64 x 16 tile and a one-sample halo in LDS, the table applied on the way in, every
//                             coordinate clamped to the visible part of the picture rectangle; a lane then computes four horizontally adjacent outputs from LDS and
//                             stores them as one dword.  The host then takes the scratch plane for the slot's (ping-pong), or under a geometry copies the rectangle back.
//
// The 256-byte table travels by value as 64 dwords; the first wave copies it into LDS, one dword per lane (a by-value array indexed per lane by a sample would
// live in scratch), and a look-up is one ds_read_u8.  Byte look-ups bank by their dword, (v / 4) mod 32: two samples within the same four codes share a read,
// others may meet on a bank; on noise that is a few cycles per look-up wave, beside one global load and store per 16 (8) look-ups.  No scratch, no atomics, no wait.
#include "kernels_common.hpp"

#include <cstring>

struct adj_tab { unsigned w[64]; };

struct adj_args {
    uint8_t *y, *uv;
    int W, H, x0, x1, y0, y1; // the picture rectangle (even)
    int cu, su;
    adj_tab tab;
};

DEV int adj_clip(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
DEV unsigned adj_lut4(const uint8_t *t, unsigned w) { return (unsigned)t[w & 255u] | ((unsigned)t[(w >> 8) & 255u] << 8) | ((unsigned)t[(w >> 16) & 255u] << 16) | ((unsigned)t[w >> 24] << 24); }

template <bool LUMA, bool CHROMA>
__global__ __launch_bounds__(256) void adjust_point_kernel(adj_args a) {
    __shared__ unsigned tab[64];
    if (LUMA) {
        if (threadIdx.x < 64) tab[threadIdx.x] = a.tab.w[threadIdx.x];
        __syncthreads();
    }
    const int tx = blockIdx.x * 256 + threadIdx.x, per_row = a.W >> 3, rows2 = a.H >> 1;
    if (tx >= per_row * rows2) return;
    const int ry = tx / per_row, cx = tx - ry * per_row, x0 = cx * 8;
    if (2 * ry < a.y0 || 2 * ry >= a.y1 || x0 + 8 <= a.x0 || x0 >= a.x1) return;
    uint8_t *py = a.y + (size_t)(2 * ry) * a.W + x0, *puv = a.uv + (size_t)ry * a.W + x0;
    uint2 s0 = make_uint2(0, 0), s1 = s0, sc = s0;
    if (LUMA) { s0 = ldg64(py); s1 = ldg64(py + a.W); }
    if (CHROMA) sc = ldg64(puv);
    uint2 o0 = s0, o1 = s1, ouv = sc;
    if (LUMA) {
        const uint8_t *t = (const uint8_t *)tab;
        o0 = make_uint2(adj_lut4(t, s0.x), adj_lut4(t, s0.y));
        o1 = make_uint2(adj_lut4(t, s1.x), adj_lut4(t, s1.y));
    }
    if (CHROMA) {
        const unsigned cw[2] = {sc.x, sc.y};
        int nb[4], nr[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int cb = byte_of(cw[i >> 1], 2 * (i & 1)) - 128, cr = byte_of(cw[i >> 1], 2 * (i & 1) + 1) - 128;
            nb[i] = adj_clip(128 + ((a.cu * cb + a.su * cr + 2048) >> 12));
            nr[i] = adj_clip(128 + ((a.cu * cr - a.su * cb + 2048) >> 12));
        }
        ouv = make_uint2((unsigned)nb[0] | (nr[0] << 8) | (nb[1] << 16) | ((unsigned)nr[1] << 24), (unsigned)nb[2] | (nr[2] << 8) | (nb[3] << 16) | ((unsigned)nr[3] << 24));
    }
    if (x0 < a.x0 || x0 + 8 > a.x1) { // straddles an edge of the picture rectangle: per column pair, adjusted inside, the original bytes outside
        unsigned m[2];
#pragma unroll
        for (int k = 0; k < 2; k++) m[k] = (x0 + 4 * k >= a.x0 && x0 + 4 * k < a.x1 ? 0x0000ffffu : 0u) | (x0 + 4 * k + 2 >= a.x0 && x0 + 4 * k + 2 < a.x1 ? 0xffff0000u : 0u);
        o0 = make_uint2((o0.x & m[0]) | (s0.x & ~m[0]), (o0.y & m[1]) | (s0.y & ~m[1]));
        o1 = make_uint2((o1.x & m[0]) | (s1.x & ~m[0]), (o1.y & m[1]) | (s1.y & ~m[1]));
        ouv = make_uint2((ouv.x & m[0]) | (sc.x & ~m[0]), (ouv.y & m[1]) | (sc.y & ~m[1]));
    }
    if (LUMA) { stg64(py, o0); stg64(py + a.W, o1); }
    if (CHROMA) stg64(puv, ouv);
}

// y, uv: NV12 surfaces of W x H (multiples of 8 / 2) at stride W, 8-byte aligned; rect: x0, x1, y0, y1 (even, inside the surfaces); luma: the 256 bytes of the
// table, or null (the luma plane is not touched); chroma: {cu, su}, or null (the chroma plane is not touched).  -1: arguments outside that, or both null.
int k_launch_adjust(uint8_t *y, uint8_t *uv, int W, int H, const int rect[4], const uint8_t *luma, const int *chroma, hipStream_t s) {
    if (!y || !uv || !rect || (!luma && !chroma) || W <= 0 || H <= 0 || (W & 7) || (H & 1) || ((((uintptr_t)y) | ((uintptr_t)uv)) & 7)) return -1;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return -1;
    adj_args a;
    a.y = y; a.uv = uv; a.W = W; a.H = H; a.x0 = rect[0]; a.x1 = rect[1]; a.y0 = rect[2]; a.y1 = rect[3];
    a.cu = chroma ? chroma[0] : 4096; a.su = chroma ? chroma[1] : 0;
    if (luma) memcpy(a.tab.w, luma, 256); else memset(a.tab.w, 0, 256);
    const dim3 g(((W >> 3) * (H >> 1) + 255) / 256), b(256);
    if (luma && chroma) hipLaunchKernelGGL((adjust_point_kernel<true, true>), g, b, 0, s, a);
    else if (luma) hipLaunchKernelGGL((adjust_point_kernel<true, false>), g, b, 0, s, a);
    else hipLaunchKernelGGL((adjust_point_kernel<false, true>), g, b, 0, s, a);
    return 0;
}

// =================================================================== the stencil form
#define ADJ_TW 64                    /* a tile's outputs per row: four per lane, sixteen lanes */
#define ADJ_TH 16                    /* ... and its rows: sixteen lanes x sixteen rows = 256 threads */
#define ADJ_PITCH (ADJ_TW / 4 + 2)   /* dwords of an LDS row: the sample at x lies at byte x - tx0 + 4, so a lane's four centres are one aligned dword; the left halo
                                        is byte 3 of dword 0, the right one byte 0 of the last */
struct sharp_args {
    const uint8_t *y;
    uint8_t *out;
    int W, x0, x1, y0, y1; // the picture rectangle (even): what is written (whole dwords: up to two bytes beyond its left and right edge, inside the row)
    int vx1, vy1;          // the end of its visible part: min(x1, visible width), min(y1, visible height)
    int amount, thr16;     // sharpen; 16 threshold for sharpen > 0, -1 otherwise (no sample stays)
    adj_tab tab;
};

DEV int sharp_one(int c, int sum, int amount, int thr16) {
    const int d = 16 * c - sum, ad = d < 0 ? -d : d;
    return ad <= thr16 ? c : adj_clip(c + ((amount * d + 128) >> 8));
}

// LUT: the luma table is not the identity (otherwise nothing of it is staged or looked up)
template <bool LUT>
__global__ __launch_bounds__(256) void adjust_sharpen_kernel(sharp_args a) {
    __shared__ unsigned tab[LUT ? 64 : 1];
    __shared__ unsigned tile[(ADJ_TH + 2) * ADJ_PITCH];
    const int tid = threadIdx.x;
    if (LUT) {
        if (tid < 64) tab[tid] = a.tab.w[tid];
        __syncthreads();
    }
    const uint8_t *t = (const uint8_t *)tab;
    const int tx0 = (a.x0 & ~(ADJ_TW - 1)) + ADJ_TW * (int)blockIdx.x, ty0 = (a.y0 & ~(ADJ_TH - 1)) + ADJ_TH * (int)blockIdx.y;
    // stage: LDS row r is the picture's row clamp(ty0 - 1 + r), LDS byte i its column clamp(tx0 - 4 + i), both clamped to the visible part of the rectangle
    for (int i = tid; i < (ADJ_TH + 2) * ADJ_PITCH; i += 256) {
        const int r = i / ADJ_PITCH, j = i - r * ADJ_PITCH;
        int yy = ty0 - 1 + r;
        yy = yy < a.y0 ? a.y0 : yy > a.vy1 - 1 ? a.vy1 - 1 : yy;
        const uint8_t *row = a.y + (size_t)yy * a.W;
        const int xb = tx0 - 4 + 4 * j;
        unsigned w;
        if (xb >= a.x0 && xb + 4 <= a.vx1) w = ldg32(row + xb); // (an aligned dword inside the row)
        else {
            w = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int xx = xb + k;
                xx = xx < a.x0 ? a.x0 : xx > a.vx1 - 1 ? a.vx1 - 1 : xx;
                w |= (unsigned)row[xx] << (8 * k);
            }
        }
        tile[i] = LUT ? adj_lut4(t, w) : w;
    }
    __syncthreads();
    const int r = tid >> 4, c = tid & 15, x = tx0 + 4 * c, y = ty0 + r;
    if (y < a.y0 || y >= a.y1 || x + 4 <= a.x0 || x >= a.x1) return;
    // a margin sample is the result of its clamped visible position: the centre's row and column are clamped, the neighbours' by the staging
    int yc = y > a.vy1 - 1 ? a.vy1 - 1 : y;
    yc = yc < ty0 ? ty0 : yc; // (never: a tile that meets the rectangle holds one of its visible rows and columns; k_launch_adjust_sharpen's contract)
    const unsigned *l0 = tile + (yc - ty0) * ADJ_PITCH, *l1 = l0 + ADJ_PITCH, *l2 = l1 + ADJ_PITCH;
    int v[4];
    if (x + 4 <= a.vx1) { // four centres in one dword, their neighbours in the dwords beside it
        int h[3][6];
        const unsigned *l[3] = {l0, l1, l2};
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const unsigned p = l[q][c], m = l[q][c + 1], n = l[q][c + 2];
            h[q][0] = (int)(p >> 24); h[q][1] = byte_of(m, 0); h[q][2] = byte_of(m, 1); h[q][3] = byte_of(m, 2); h[q][4] = byte_of(m, 3); h[q][5] = byte_of(n, 0);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int sum = (h[0][k] + 2 * h[0][k + 1] + h[0][k + 2]) + 2 * (h[1][k] + 2 * h[1][k + 1] + h[1][k + 2]) + (h[2][k] + 2 * h[2][k + 1] + h[2][k + 2]);
            v[k] = sharp_one(h[1][k + 1], sum, a.amount, a.thr16);
        }
    } else { // the dword reaches into the margin (or past the rectangle's right edge): sample by sample
        const uint8_t *b0 = (const uint8_t *)l0, *b1 = (const uint8_t *)l1, *b2 = (const uint8_t *)l2;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int xc = x + k > a.vx1 - 1 ? a.vx1 - 1 : x + k;
            xc = xc < tx0 ? tx0 : xc; // (never, as above)
            const int ci = xc - tx0 + 4;
            const int sum = (b0[ci - 1] + 2 * b0[ci] + b0[ci + 1]) + 2 * (b1[ci - 1] + 2 * b1[ci] + b1[ci + 1]) + (b2[ci - 1] + 2 * b2[ci] + b2[ci + 1]);
            v[k] = sharp_one(b1[ci], sum, a.amount, a.thr16);
        }
    }
    stg32(a.out + (size_t)y * a.W + x, (unsigned)v[0] | (v[1] << 8) | (v[2] << 16) | ((unsigned)v[3] << 24));
}

// y -> out: luma planes of W x H (multiples of 16) at stride W, 4-byte aligned, not the same plane; vw x vh: the visible size, less than 16 short of W x H; rect as
// k_launch_adjust's; luma: the 256 bytes of the table, or null (the luma is neutral: the stencil alone); amount -16 .. 64 except 0, thr 0 .. 32.  Writes the rectangle's
// samples of `out` (and up to two bytes beside its left and right edge).  -1: arguments outside that.
int k_launch_adjust_sharpen(const uint8_t *y, uint8_t *out, int W, int H, int vw, int vh, const int rect[4], const uint8_t *luma, int amount, int thr, hipStream_t s) {
    if (!y || !out || y == out || !rect || W <= 0 || H <= 0 || (W & 15) || (H & 15) || vw > W || vw <= W - 16 || vh > H || vh <= H - 16 || ((((uintptr_t)y) | ((uintptr_t)out)) & 3)) return -1;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return -1;
    if (rect[0] >= vw || rect[2] >= vh || amount < -16 || amount > 64 || amount == 0 || thr < 0 || thr > 32) return -1;
    sharp_args a;
    a.y = y; a.out = out; a.W = W; a.x0 = rect[0]; a.x1 = rect[1]; a.y0 = rect[2]; a.y1 = rect[3];
    a.vx1 = rect[1] < vw ? rect[1] : vw; a.vy1 = rect[3] < vh ? rect[3] : vh;
    a.amount = amount; a.thr16 = amount > 0 ? 16 * thr : -1;
    if (luma) memcpy(a.tab.w, luma, 256); else memset(a.tab.w, 0, 256);
    const int gx0 = rect[0] & ~(ADJ_TW - 1), gy0 = rect[2] & ~(ADJ_TH - 1);
    const dim3 g((rect[1] - gx0 + ADJ_TW - 1) / ADJ_TW, (rect[3] - gy0 + ADJ_TH - 1) / ADJ_TH), b(256);
    if (luma) hipLaunchKernelGGL(adjust_sharpen_kernel<true>, g, b, 0, s, a);
    else hipLaunchKernelGGL(adjust_sharpen_kernel<false>, g, b, 0, s, a);
    return 0;
}
