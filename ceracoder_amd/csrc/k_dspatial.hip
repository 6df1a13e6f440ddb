// k_dspatial.hip -- spatial noise reduction on the coded NV12 surfaces of a slot and its per-picture noise estimate (the rule:
// dspatial_host.h).  Three kernels, all launched on one stream:
//
//   filter    adjust_sharpen_kernel's shape, one launch per plane: from the slot's plane into a scratch plane (a halo sample belongs to a neighbouring workgroup:
//             not in place).  A workgroup stages a tile of 64 bytes x 16 rows and its halo in LDS -- two samples and two rows for the luma's 5 x 5 stencil, one
//             Cb / Cr pair and one row for the chroma's 3 x 3 on the interleaved plane, which is two bytes either way -- every coordinate clamped to the visible
//             part of the picture rectangle (the chroma's by pairs, so Cb meets Cb); a lane then computes four horizontally adjacent outputs from three aligned
//             LDS dwords per row and stores them as one dword.  A neighbour's term sgn(d) F_s[|d|] is one LDS word, looked up by d + 255 in a table of 511 that
//             the workgroup builds from the strength's 256 weights R_s: in manual mode those travel by value as 64 dwords, as k_adjust.hip's table does; in
//             automatic mode the launch takes its strength as one uniform load from the record the decide launch wrote and R_s from a device buffer of all 33
//             tables, so the strength never visits the host.  s = 0 there is the table of zeros: the plane is copied, margins replicated like any other.
//   measure   a thread owns an aligned 8 x 8 luma block: eight 8-byte loads, the Laplacian mask as two second differences with two rows of history in
//             registers, its bin and its vote.  At most DS_SLABS_MAX workgroups walk the candidates in a grid-stride loop; each keeps one histogram per wave
//             in LDS and stores their sum as a slab with plain stores: no global atomic, no clear in front of the launch.  Equal bins are folded across the
//             wave before they reach a counter (a flat picture puts every block into bin 0): the lanes that hold the first voting lane's bin are counted
//             with a ballot and added once, up to twice, and what is left adds for itself.
//   decide    one workgroup of 256: thread v sums bin v over the slabs in 64 bits, the prefix sum runs through LDS, the percentile's bin is an LDS minimum,
//             thread 0 takes the state step (ds_decide, the host's own function) and writes state and record.
// No scratch memory, no global atomics, no wait on another workgroup.
#include "kernels_common.hpp"
#include "dspatial_host.h"

#include <cstring>

// ------------------------------------------------------------------ filter
#define DSP_TW 64                    /* a tile's bytes per row: four per lane, sixteen lanes */
#define DSP_TH 16                    /* ... and its rows */
#define DSP_PITCH (DSP_TW / 4 + 2)   /* dwords of an LDS row: the byte at x lies at x - tx0 + 4; the left halo is bytes 2, 3 of dword 0, the right one bytes 0, 1 of the last */

struct dsp_tab { unsigned w[64]; };

struct dsp_args {
    const uint8_t *src;
    uint8_t *out;
    int W, x0, x1, y0, y1; // the picture rectangle in this plane's bytes and rows: what is written (whole dwords: up to two bytes beyond its left and right edge)
    int vx1, vy1;          // the end of its visible part
    const int *rec;        // automatic: the record's word that holds this plane's strength; null: manual
    const uint8_t *tabs;   // automatic: R_0 .. R_32, 256 bytes each
    dsp_tab tab;           // manual: R_s
};

// STEP, RAD: 1, 2 the luma plane; 2, 1 the interleaved chroma plane
template <int STEP, int RAD>
__global__ __launch_bounds__(256) void dspatial_filter_kernel(dsp_args a) {
    constexpr int TAPS = 2 * RAD + 1, ROWS = DSP_TH + 2 * RAD, SHIFT = RAD == 2 ? 12 : 8;
    __shared__ unsigned rtab[64];
    __shared__ int sF[512];
    __shared__ unsigned tile[ROWS * DSP_PITCH];
    const int tid = threadIdx.x;
    if (tid < 64) {
        if (a.rec) { // (uniform)
            int s = (int)ldg32(a.rec);
            s = s < 0 ? 0 : s > DS_MAX ? DS_MAX : s;
            rtab[tid] = ldg32(a.tabs + 256 * s + 4 * tid);
        } else rtab[tid] = a.tab.w[tid];
    }
    const int tx0 = (a.x0 & ~(DSP_TW - 1)) + DSP_TW * (int)blockIdx.x, ty0 = (a.y0 & ~(DSP_TH - 1)) + DSP_TH * (int)blockIdx.y;
    // stage: LDS row r is the plane's row clamp(ty0 - RAD + r), LDS byte i its byte clamp(tx0 - 4 + i), both clamped to the visible part of the rectangle
    for (int i = tid; i < ROWS * DSP_PITCH; i += 256) {
        const int r = i / DSP_PITCH, j = i - r * DSP_PITCH;
        int yy = ty0 - RAD + r;
        yy = yy < a.y0 ? a.y0 : yy > a.vy1 - 1 ? a.vy1 - 1 : yy;
        const uint8_t *row = a.src + (size_t)yy * a.W;
        const int xb = tx0 - 4 + 4 * j;
        unsigned w;
        if (xb >= a.x0 && xb + 4 <= a.vx1) w = ldg32(row + xb); // (an aligned dword inside the row)
        else {
            w = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int p = (xb + k) & (STEP - 1);
                int xx = xb + k - p;
                xx = (xx < a.x0 ? a.x0 : xx > a.vx1 - STEP ? a.vx1 - STEP : xx) + p;
                w |= (unsigned)row[xx] << (8 * k);
            }
        }
        tile[i] = w;
    }
    __syncthreads();
    for (int i = tid; i < 511; i += 256) { // sgn(d) F_s[|d|] at d + 255
        const int d = i - 255, ad = iabs(d), f = ad * (int)((const uint8_t *)rtab)[ad];
        sF[i] = d < 0 ? -f : f;
    }
    __syncthreads();
    const int r = tid >> 4, c = tid & 15, x = tx0 + 4 * c, y = ty0 + r;
    if (y < a.y0 || y >= a.y1 || x + 4 <= a.x0 || x >= a.x1) return;
    // a margin sample is the result of its clamped visible position: the centre's row and column are clamped, the neighbours' by the staging
    int yc = y > a.vy1 - 1 ? a.vy1 - 1 : y;
    yc = yc < ty0 ? ty0 : yc; // (never: a tile that meets the rectangle holds one of its visible rows and columns; k_launch_dspatial_filter's contract)
    const unsigned *l0 = tile + (yc - ty0) * DSP_PITCH; // (the LDS row of the plane's row yc - RAD)
    constexpr int wt[5] = {1, RAD == 2 ? 4 : 2, RAD == 2 ? 6 : 1, 4, 1};
    int v[4];
    if (x + 4 <= a.vx1) { // four centres in one dword, their neighbours in the dwords beside it
        int h[TAPS][8];
#pragma unroll
        for (int q = 0; q < TAPS; q++) {
            const unsigned p = l0[q * DSP_PITCH + c], m = l0[q * DSP_PITCH + c + 1], n = l0[q * DSP_PITCH + c + 2];
            h[q][0] = byte_of(p, 2); h[q][1] = byte_of(p, 3); h[q][2] = byte_of(m, 0); h[q][3] = byte_of(m, 1); h[q][4] = byte_of(m, 2); h[q][5] = byte_of(m, 3);
            h[q][6] = byte_of(n, 0); h[q][7] = byte_of(n, 1);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int cc = h[RAD][k + 2];
            int sum = 0;
#pragma unroll
            for (int dy = 0; dy < TAPS; dy++)
#pragma unroll
                for (int dx = 0; dx < TAPS; dx++)
                    if (dy != RAD || dx != RAD) sum += wt[dy] * wt[dx] * sF[h[dy][k + 2 + STEP * (dx - RAD)] - cc + 255];
            v[k] = cc + ((sum + (1 << (SHIFT - 1))) >> SHIFT);
        }
    } else { // the dword reaches into the margin (or past the rectangle's right edge): byte by byte
        const uint8_t *b = (const uint8_t *)l0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int p = (x + k) & (STEP - 1);
            int xc = x + k - p;
            xc = (xc > a.vx1 - STEP ? a.vx1 - STEP : xc) + p;
            xc = xc < tx0 ? tx0 : xc; // (never, as above)
            const int ci = xc - tx0 + 4, cc = b[RAD * DSP_PITCH * 4 + ci];
            int sum = 0;
#pragma unroll
            for (int dy = 0; dy < TAPS; dy++)
#pragma unroll
                for (int dx = 0; dx < TAPS; dx++)
                    if (dy != RAD || dx != RAD) sum += wt[dy] * wt[dx] * sF[(int)b[dy * DSP_PITCH * 4 + ci + STEP * (dx - RAD)] - cc + 255];
            v[k] = cc + ((sum + (1 << (SHIFT - 1))) >> SHIFT);
        }
    }
    stg32(a.out + (size_t)y * a.W + x, (unsigned)v[0] | (v[1] << 8) | (v[2] << 16) | ((unsigned)v[3] << 24));
}

// src -> out: one plane of NV12 surfaces of W x H (multiples of 16) at stride W -- chroma 0: the luma plane, 1: the interleaved chroma plane (H / 2 rows) --, 4-byte
// aligned, not the same plane; vw x vh: the visible size, less than 16 short of W x H; rect: x0, x1, y0, y1 in luma samples (even, inside the surfaces, meeting the
// visible part).  weight: the 256 bytes of R_s (manual), or null with rec, the device word that holds the strength, and tabs, the device's 33 tables (automatic).
// Writes the rectangle's bytes of `out` (and up to two bytes beside its left and right edge).  -1: arguments outside that.
int k_launch_dspatial_filter(const uint8_t *src, uint8_t *out, int W, int H, int vw, int vh, const int rect[4], int chroma, const uint8_t *weight, const int *rec, const uint8_t *tabs, hipStream_t s) {
    if (!src || !out || src == out || !rect || W <= 0 || H <= 0 || (W & 15) || (H & 15) || vw > W || vw <= W - 16 || vh > H || vh <= H - 16 || ((((uintptr_t)src) | ((uintptr_t)out)) & 3)) return -1;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return -1;
    if (rect[0] >= vw || rect[2] >= vh || (weight ? (rec || tabs) : (!rec || !tabs || (((uintptr_t)tabs) & 3)))) return -1;
    dsp_args a;
    const int vx1 = rect[1] < vw ? rect[1] : vw, vy1 = rect[3] < vh ? rect[3] : vh;
    a.src = src; a.out = out; a.W = W; a.x0 = rect[0]; a.x1 = rect[1];
    if (chroma) { a.y0 = rect[2] >> 1; a.y1 = rect[3] >> 1; a.vx1 = (vx1 + 1) & ~1; a.vy1 = (vy1 + 1) >> 1; }
    else { a.y0 = rect[2]; a.y1 = rect[3]; a.vx1 = vx1; a.vy1 = vy1; }
    a.rec = rec; a.tabs = tabs;
    if (weight) memcpy(a.tab.w, weight, 256); else memset(a.tab.w, 0, 256);
    const int gx0 = a.x0 & ~(DSP_TW - 1), gy0 = a.y0 & ~(DSP_TH - 1);
    const dim3 g((a.x1 - gx0 + DSP_TW - 1) / DSP_TW, (a.y1 - gy0 + DSP_TH - 1) / DSP_TH), b(256);
    if (chroma) hipLaunchKernelGGL((dspatial_filter_kernel<2, 1>), g, b, 0, s, a);
    else hipLaunchKernelGGL((dspatial_filter_kernel<1, 2>), g, b, 0, s, a);
    return 0;
}

// ------------------------------------------------------------------ measure
struct dsm_args {
    const uint8_t *y;
    int W;
    int bx0, bcols, by0, total; // the candidates: first block column, their count per row, first block row, their number
    int lo, hi;                 // the bounds of a voting block's sample sum
    unsigned *slabs;
};

// the lanes with `have` add one to hist[v]: up to two rounds of folding on the first such lane's bin, then lane by lane.  Every lane of the wave calls.
DEV void ds_flush(unsigned *hist, int lane, int v, bool have) {
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const unsigned long long pend = __ballot(have);
        if (!pend) return; // (uniform)
        const int leader = __ffsll((long long)pend) - 1, lv = __builtin_amdgcn_readlane(v, leader);
        const bool m = have && v == lv;
        const unsigned long long mm = __ballot(m);
        if (lane == leader) atomicAdd(&hist[lv], (unsigned)__popcll(mm));
        have = have && !m;
        if (4 * __popcll(mm) < __popcll(pend)) break; // (uniform) many bins: a second round folds little
    }
    if (have) atomicAdd(&hist[v], 1u);
}

__global__ __launch_bounds__(256) void dspatial_measure_kernel(dsm_args a) {
    __shared__ unsigned hist[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int w = 0; w < 4; w++) hist[w][tid] = 0;
    __syncthreads();
    const int step = (int)gridDim.x * 256;
    for (int base = (int)blockIdx.x * 256; base < a.total; base += step) { // (the same trips for every lane of a workgroup: ds_flush is the wave's)
        const int p = base + tid;
        const bool have = p < a.total;
        int bin = 0;
        bool vote = false;
        if (have) {
            const int br = p / a.bcols, bc = p - br * a.bcols;
            const uint8_t *q = a.y + (size_t)(8 * (a.by0 + br)) * a.W + 8 * (a.bx0 + bc);
            int sum = 0, A = 0, h0[6] = {0, 0, 0, 0, 0, 0}, h1[6] = {0, 0, 0, 0, 0, 0}; // the second differences of the two rows above
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint2 w = ldg64(q + (size_t)r * a.W);
                int px[8], hc[6];
#pragma unroll
                for (int i = 0; i < 8; i++) { px[i] = byte_of(i < 4 ? w.x : w.y, i & 3); sum += px[i]; }
#pragma unroll
                for (int i = 0; i < 6; i++) hc[i] = px[i] - 2 * px[i + 1] + px[i + 2];
                if (r >= 2) {
#pragma unroll
                    for (int i = 0; i < 6; i++) A += iabs(h0[i] - 2 * h1[i] + hc[i]);
                }
#pragma unroll
                for (int i = 0; i < 6; i++) { h0[i] = h1[i]; h1[i] = hc[i]; }
            }
            vote = sum >= a.lo && sum <= a.hi;
            bin = ds_bin(A);
        }
        ds_flush(hist[wave], lane, bin, vote);
    }
    __syncthreads();
    stg32(a.slabs + (size_t)blockIdx.x * DS_SLAB_WORDS + tid, hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid]);
}

// y: the luma plane of a surface of W x H (W a multiple of 8) at stride W, 8-byte aligned; rect: x0, x1, y0, y1 (even, inside the surface); vw x vh: the visible
// size, which the rectangle meets; slabs: room for DS_SLABS_MAX slabs.  Returns the number of slabs written (1 .. DS_SLABS_MAX; without a candidate: one slab of
// zeros), -1: arguments outside that.
int k_launch_dspatial_measure(const uint8_t *y, int W, int H, const int rect[4], int vw, int vh, int full_range, unsigned *slabs, hipStream_t s) {
    if (!y || !rect || !slabs || W <= 0 || H <= 0 || W > 8192 || H > 8192 || (W & 7) || (H & 1) || (((uintptr_t)y) & 7)) return -1;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return -1;
    if (vw < 1 || vh < 1 || vw > W || vh > H || rect[0] >= vw || rect[2] >= vh) return -1;
    dsm_args a;
    int brows;
    ds_blocks(rect, vw, vh, &a.bx0, &a.bcols, &a.by0, &brows);
    a.y = y; a.W = W; a.total = a.bcols * brows;
    if (a.total == 0) a.bcols = 1; // (nothing is divided by it then; kept away from 0 all the same)
    const int B = ds_black(full_range), S = ds_scale(full_range);
    a.lo = ds_vote_lo(B, S); a.hi = ds_vote_hi(B, S);
    a.slabs = slabs;
    int g = (a.total + 255) / 256;
    g = g > DS_SLABS_MAX ? DS_SLABS_MAX : g < 1 ? 1 : g;
    hipLaunchKernelGGL(dspatial_measure_kernel, dim3(g), dim3(256), 0, s, a);
    return g;
}

// ------------------------------------------------------------------ decide
struct dsd_args {
    const unsigned *slabs;
    int nslabs;
    unsigned NC;
    int set[5];
    int prime;
    int *state, *rec;
};

__global__ __launch_bounds__(256) void dspatial_decide_kernel(dsd_args a) {
    __shared__ unsigned long long cum[2][256];
    __shared__ int s_v;
    const int tid = threadIdx.x;
    unsigned long long c = 0;
    for (int g0 = 0; g0 < a.nslabs; g0 += 16) { // 16 loads in flight per round
        unsigned t[16];
#pragma unroll
        for (int k = 0; k < 16; k++) { const int g = g0 + k < a.nslabs ? g0 + k : a.nslabs - 1; t[k] = ldg32(a.slabs + (size_t)g * DS_SLAB_WORDS + tid); }
#pragma unroll
        for (int k = 0; k < 16; k++) c += g0 + k < a.nslabs ? t[k] : 0u;
    }
    cum[0][tid] = c;
    if (tid == 0) s_v = 255;
    __syncthreads();
    int src = 0;
    for (int d = 1; d < 256; d <<= 1) {
        unsigned long long x = cum[src][tid];
        if (tid >= d) x += cum[src][tid - d];
        cum[src ^ 1][tid] = x;
        __syncthreads();
        src ^= 1;
    }
    const unsigned long long N = cum[src][255];
    if (ds_is_v(cum[src][tid], N, a.set[3])) atomicMin(&s_v, tid);
    __syncthreads();
    if (tid == 0) {
        int X = (int)ldg32(a.state), rec[DS_REC_WORDS];
        ds_decide(a.NC, (uint32_t)N, s_v, a.set, a.prime, &X, rec);
        stg32(a.state, (unsigned)X);
#pragma unroll
        for (int i = 0; i < DS_REC_WORDS; i++) stg32(a.rec + i, (unsigned)rec[i]);
    }
}

// slabs: nslabs (1 .. DS_SLABS_MAX) slabs of a measure launch; NC: the candidates; set: the checked automatic setting's five fields; state: one word, read (unless
// prime) and written; rec: DS_REC_WORDS words.  -1: arguments outside that.
int k_launch_dspatial_decide(const unsigned *slabs, int nslabs, unsigned NC, const int set[5], int prime, int *state, int *rec, hipStream_t s) {
    if (!slabs || !set || !state || !rec || nslabs < 1 || nslabs > DS_SLABS_MAX) return -1;
    dsd_args a;
    a.slabs = slabs; a.nslabs = nslabs; a.NC = NC;
    for (int i = 0; i < 5; i++) a.set[i] = set[i];
    a.prime = prime ? 1 : 0; a.state = state; a.rec = rec;
    hipLaunchKernelGGL(dspatial_decide_kernel, dim3(1), dim3(256), 0, s, a);
    return 0;
}
