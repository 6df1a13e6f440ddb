// k_hdr.hip -- HDR input (PQ / HLG, BT.2020 non-constant luminance, 10 bits) tone-mapped to 8-bit SDR NV12 in the conversion launch (DESIGN.md section 22
// states the model and the rule).  Hand-written HIP for gfx950 (CDNA4, wave64); part of libmi355enc.
// Shape of csc_deep_kernel (k_csc.hip): one thread makes a PW x 2 luma patch and its PW / 2 chroma pairs, PW 8 (P010, I420_10) or 24 (v210); the fast path
// reads 16-byte words and writes aligned 8-byte ones; a patch that reaches past the visible width, margin rows and planes that are not suitably aligned go
// sample by sample with clamped source coordinates.  Integer arithmetic and table look-ups only: the parameter block (hdr_host.c) holds the matrices and the
// four tables; products that pass 32 bits are 32 x 32 -> 64 (v_mad_i64_i32).  The grid is one patch per thread.  Every workgroup stages the block (31 KB) into
// LDS for its 256 patches (4096 luma samples; v210: 12 288); with -DHDR_TABLES_GLOBAL the tables are gathered from global memory through the vector cache
// instead -- measured slower at every size and format, as were grids of fewer workgroups that walk several patches each to amortise the staging
// (profiles/hdr_price.md has all of them).
#include "kernels_common.hpp"
#include "hdr_host.h"

struct hdr_args {
    const uint8_t *p0, *p1, *p2; // P010: Y, CbCr; I420_10: Y, U, V; v210: p0 only
    int s0, s1, s2;              // their strides in bytes
    uint8_t *dy, *duv;           // NV12 destination, coded size W x H, stride W
    int vw, vh, W, H;            // visible and coded size
    const int *tab;              // the parameter block (HDR_WORDS words)
};
// the header's words a sample needs.  Words that follow from others are not kept (fewer scalar registers, fewer products; in integers the same numbers):
// lg = 2^16 - lr - lb, the gamut matrix's diagonal = 2^20 - the row's other two (m: the six others by rows), bg = -br - bb, rg = -rr - rb.
struct hdr_par {
    int oy, cy, rv, gu, gv, bu, lr, lb, m[6], yr, yg, yb, br, bb, rr, rb, oyo;
};
struct hdr_tab_global { const int *t; DEV int operator()(int i) const { return (int)ldg32(t + i); } };
struct hdr_tab_lds { const int *t; DEV int operator()(int i) const { return t[i]; } };

DEV hdr_par hdr_load_par(const int *t) {
    hdr_par P;
    P.oy = t[8]; P.cy = t[9]; P.rv = t[10]; P.gu = t[11]; P.gv = t[12]; P.bu = t[13];
    P.lr = t[14]; P.lb = t[16];
    P.m[0] = t[18]; P.m[1] = t[19]; P.m[2] = t[20]; P.m[3] = t[22]; P.m[4] = t[23]; P.m[5] = t[24];
    P.yr = t[26]; P.yg = t[27]; P.yb = t[28]; P.br = t[29]; P.bb = t[31]; P.rr = t[32]; P.rb = t[34]; P.oyo = t[35];
    return P;
}
DEV long long mul64(int a, int b) { return (long long)a * (long long)b; }
// a gain table, spaced by octaves: entry 64 o + m stands for s = (64 + m) << (o + 2); s in 0 .. 2^28 (below 256: the first entry)
template <class T> DEV int hdr_gain(const T &tab, int at, int s) {
    const int big = max(min(s, 1 << 28), 256);
    const int e = 31 - __clz(big), sh = e - 6, q = big >> sh, i = 64 * (e - 8) + q - 64, f = big - (q << sh);
    const int a = tab(at + i), b = tab(at + i + 1);
    return a + (int)((mul64(b - a, f) + (1ll << (sh - 1))) >> sh);
}
// one sample: its 10-bit luma and the chroma terms of its pair -> non-linear BT.709 R, G, B in 2^-16 units
template <bool HLG, class T> DEV void hdr_sample(const hdr_par &P, const T &tab, int y, int tr, int tg, int tb, int &R, int &G, int &B) {
    const int cyy = P.cy * (y - P.oy), t[3] = {cyy + tr, cyy + tg, cyy + tb};
    int l[3], w[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int x = clip3(0, 1 << 24, (t[i] + 8) >> 4), k = min(x >> 12, 4095), f = x - (k << 12);
        const int a = tab(HDR_LIN_AT + k), b = tab(HDR_LIN_AT + k + 1);
        l[i] = a + (int)((mul64(b - a, f) + 2048) >> 12);
    }
    if (HLG) { // the OOTF: scene light times Ys^(g - 1)
        const int ys = (int)((mul64(P.lr, l[0] - l[1]) + mul64(P.lb, l[2] - l[1]) + ((long long)l[1] << 16) + 32768) >> 16);
        const int g1 = hdr_gain(tab, HDR_GA_AT, ys);
#pragma unroll
        for (int i = 0; i < 3; i++) l[i] = (int)((mul64(l[i], g1) + (1 << 29)) >> 30);
    }
    const int g2 = hdr_gain(tab, HDR_GB_AT, max(max(l[0], l[1]), l[2])); // the tone curve on the largest component, as a gain on all three
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = (int)((mul64(l[i], g2) + (1 << 23)) >> 24);
    int o[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int j0 = i == 0 ? 1 : 0, j1 = i == 2 ? 1 : 2; // the row's two off-diagonal columns
        const int u = clip3(0, 1 << 28, (int)((mul64(P.m[2 * i], w[j0] - w[i]) + mul64(P.m[2 * i + 1], w[j1] - w[i]) + ((long long)w[i] << 20) + (1 << 19)) >> 20));
        const int k = min(u >> 18, 1023), f = u - (k << 18);
        const int a = tab(HDR_OE_AT + k), b = tab(HDR_OE_AT + k + 1);
        o[i] = a + (((b - a) * f + (1 << 17)) >> 18);
    }
    R = o[0]; G = o[1]; B = o[2];
}
// an 8 x 2 piece: yv its 10-bit luma (rows base, base + 1), c its four chroma pairs (Cb0 Cr0 Cb1 Cr1 ...); dup: bit i set -- pair i lies in the margin right of
// the picture, where both luma columns repeat the picture's last one (the pair's chroma is the last visible pair's either way)
template <bool HLG, class T> DEV void hdr_piece(const hdr_par &P, const T &tab, const int (&yv)[2][8], const int (&c)[8], unsigned dup, uint2 (&yrow)[2], unsigned (&uvw)[2]) {
    int o[2][8], cb[4], cr[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = c[2 * i] - 512, v = c[2 * i + 1] - 512;
        const int tr = P.rv * v, tg = P.gu * u + P.gv * v, tb = P.bu * u;
        int sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int r = 0; r < 2; r++) {
#pragma unroll
            for (int k = 0; k < 2; k++) {
                int R, G, B;
                hdr_sample<HLG>(P, tab, yv[r][2 * i + k], tr, tg, tb, R, G, B);
                o[r][2 * i + k] = (int)((mul64(P.yr, R) + mul64(P.yg, G) + mul64(P.yb, B) + ((long long)P.oyo << 30) + (1 << 29)) >> 30);
                sr += R; sg += G; sb += B;
            }
            if ((dup >> i) & 1) o[r][2 * i] = o[r][2 * i + 1];
        }
        cb[i] = (int)((mul64(P.br, sr - sg) + mul64(P.bb, sb - sg) + (128ll << 32) + (1ll << 31)) >> 32);
        cr[i] = (int)((mul64(P.rr, sr - sg) + mul64(P.rb, sb - sg) + (128ll << 32) + (1ll << 31)) >> 32);
    }
#pragma unroll
    for (int r = 0; r < 2; r++) yrow[r] = make_uint2(csc_pack4(o[r][0], o[r][1], o[r][2], o[r][3]), csc_pack4(o[r][4], o[r][5], o[r][6], o[r][7]));
    uvw[0] = csc_pack4(cb[0], cr[0], cb[1], cr[1]);
    uvw[1] = csc_pack4(cb[2], cr[2], cb[3], cr[3]);
}
// (margin rows: both luma rows are the picture's last, the chroma row that of its last two rows)
DEV void hdr_store(const hdr_args &a, int ry, int x, bool margin, const uint2 (&yrow)[2], const unsigned (&uvw)[2]) {
    stg64(a.dy + (size_t)(2 * ry) * a.W + x, margin ? yrow[1] : yrow[0]);
    stg64(a.dy + (size_t)(2 * ry + 1) * a.W + x, yrow[1]);
    stg64(a.duv + (size_t)ry * a.W + x, make_uint2(uvw[0], uvw[1]));
}
// luma sample (sx, sy), 10 bits, byte by byte
template <int FMT> DEV int hdr_luma10(const hdr_args &a, int sx, int sy) {
    const uint8_t *row = a.p0 + (size_t)sy * a.s0;
    if (FMT == 14) return deep_word(row + 2 * sx) >> 6;
    if (FMT == 15) return deep_word(row + 2 * sx) & 1023;
    const int g = sx / 6, k = sx - 6 * g;
    return (int)v210_field(row, 4 * g + v210_yw(k), v210_ys(k));
}
// chroma sample c (comp 0 Cb, 1 Cr) of the pair row made from luma rows base, base + 1; v210: the rounded mean of its two rows
template <int FMT> DEV int hdr_chroma10(const hdr_args &a, int c, int base, int comp) {
    if (FMT == 14) return deep_word(a.p1 + (size_t)(base >> 1) * a.s1 + 4 * c + 2 * comp) >> 6;
    if (FMT == 15) return deep_word((comp ? a.p2 + (size_t)(base >> 1) * a.s2 : a.p1 + (size_t)(base >> 1) * a.s1) + 2 * c) & 1023;
    const int g = c / 3, k = 2 * (c - 3 * g) + comp;
    return ((int)v210_field(a.p0 + (size_t)base * a.s0, 4 * g + v210_cw(k), v210_cs(k)) + (int)v210_field(a.p0 + (size_t)(base + 1) * a.s0, 4 * g + v210_cw(k), v210_cs(k)) + 1) >> 1;
}

// piece J (luma columns 8 J .. 8 J + 7, pairs 4 J .. 4 J + 3) of the 24 x 2 patch whose words are q: 10-bit luma, and chroma as the rounded mean of the two rows
template <int J> DEV void v210_piece(const uint4 (&q)[2][4], int (&y8)[2][8], int (&c8)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int s = 8 * J + i, g = s / 6, k = s - 6 * g;
        y8[0][i] = v210_get(q[0][g], v210_yw(k), v210_ys(k));
        y8[1][i] = v210_get(q[1][g], v210_yw(k), v210_ys(k));
        c8[i] = (v210_get(q[0][g], v210_cw(k), v210_cs(k)) + v210_get(q[1][g], v210_cw(k), v210_cs(k)) + 1) >> 1;
    }
}
template <int FMT, bool HLG, class T> DEV void hdr_patch(const hdr_args &a, const hdr_par &P, const T &tab, int tx, int per_row) {
    constexpr int PW = FMT == 16 ? 24 : 8;
    const int ry = tx / per_row, cx = tx - ry * per_row, x0 = cx * PW;
    const bool margin = 2 * ry >= a.vh;
    const int base = margin ? a.vh - 2 : 2 * ry;
    const bool vis = x0 + PW <= a.vw; // visible width is even: a patch is fully visible, or clamped per sample
    bool fast = vis && (a.s0 & 15) == 0 && (((uintptr_t)a.p0) & 15) == 0;
    if (FMT == 14) fast = fast && (a.s1 & 15) == 0 && (((uintptr_t)a.p1) & 15) == 0;
    if (FMT == 15) fast = fast && ((a.s1 | a.s2) & 7) == 0 && ((((uintptr_t)a.p1) | ((uintptr_t)a.p2)) & 7) == 0;
    uint2 yrow[2];
    unsigned uvw[2];
    if (!fast) { // sample by sample, in pieces of 8 luma columns
        const int cw = a.vw >> 1;
        for (int j = 0; j < PW / 8 && x0 + 8 * j < a.W; j++) {
            const int xp = x0 + 8 * j;
            int yv[2][8], c[8];
            unsigned dup = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const bool out = xp + 2 * i >= a.vw;
                const int cc = out ? cw - 1 : (xp >> 1) + i;
                dup |= (out ? 1u : 0u) << i;
                c[2 * i] = hdr_chroma10<FMT>(a, cc, base, 0);
                c[2 * i + 1] = hdr_chroma10<FMT>(a, cc, base, 1);
#pragma unroll
                for (int r = 0; r < 2; r++) { yv[r][2 * i] = hdr_luma10<FMT>(a, 2 * cc, base + r); yv[r][2 * i + 1] = hdr_luma10<FMT>(a, 2 * cc + 1, base + r); }
            }
            hdr_piece<HLG>(P, tab, yv, c, dup, yrow, uvw);
            hdr_store(a, ry, xp, margin, yrow, uvw);
        }
        return;
    }
    if (FMT == 16) { // the sixteen words of both rows stay in registers; the three pieces follow each other in a loop that is not unrolled, each picking its samples
        uint4 q[2][4];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint8_t *sp = a.p0 + (size_t)(base + r) * a.s0 + (size_t)cx * 64;
#pragma unroll
            for (int g = 0; g < 4; g++) q[r][g] = ldg128(sp + 16 * g);
        }
#pragma unroll 1
        for (int j = 0; j < 3; j++) {
            int y8[2][8], c8[8];
            if (j == 0) v210_piece<0>(q, y8, c8);
            else if (j == 1) v210_piece<1>(q, y8, c8);
            else v210_piece<2>(q, y8, c8);
            hdr_piece<HLG>(P, tab, y8, c8, 0u, yrow, uvw);
            hdr_store(a, ry, x0 + 8 * j, margin, yrow, uvw);
        }
        return;
    }
    constexpr int SH = FMT == 14 ? 6 : 0; // (v >> 6, or v & 1023: one shift and one mask serve both)
    int yv[2][8], c[8];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint4 q = ldg128(a.p0 + (size_t)(base + r) * a.s0 + 2 * x0);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; i++) yv[r][i] = (int)(((w[i >> 1] >> (16 * (i & 1))) & 0xffffu) >> SH & 1023u);
    }
    if (FMT == 14) {
        const uint4 q = ldg128(a.p1 + (size_t)(base >> 1) * a.s1 + 2 * x0);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; i++) c[i] = (int)(((w[i >> 1] >> (16 * (i & 1))) & 0xffffu) >> 6);
    } else {
        const uint2 u = ldg64(a.p1 + (size_t)(base >> 1) * a.s1 + x0), v = ldg64(a.p2 + (size_t)(base >> 1) * a.s2 + x0);
        const unsigned uw[2] = {u.x, u.y}, vw[2] = {v.x, v.y};
#pragma unroll
        for (int i = 0; i < 4; i++) { c[2 * i] = (int)((uw[i >> 1] >> (16 * (i & 1))) & 1023u); c[2 * i + 1] = (int)((vw[i >> 1] >> (16 * (i & 1))) & 1023u); }
    }
    hdr_piece<HLG>(P, tab, yv, c, 0u, yrow, uvw);
    hdr_store(a, ry, x0, margin, yrow, uvw);
}

// every workgroup stages the block (unless -DHDR_TABLES_GLOBAL), then converts its patches: one per thread, or under a capped grid (-DHDR_WG_QUARTERS) blockIdx.x, blockIdx.x + gridDim.x, ...
template <int FMT, bool HLG>
__global__ __launch_bounds__(256) void hdr_kernel(hdr_args a) {
    constexpr int PW = FMT == 16 ? 24 : 8;
    const int per_row = (a.W + PW - 1) / PW, total = per_row * (a.H >> 1);
    const hdr_par P = hdr_load_par(a.tab);
#ifndef HDR_TABLES_GLOBAL
    __shared__ int lds[HDR_WORDS];
    for (int i = threadIdx.x; i < HDR_WORDS; i += 256) lds[i] = (int)ldg32(a.tab + i);
    __syncthreads();
    const hdr_tab_lds tab = {lds};
#else
    const hdr_tab_global tab = {a.tab};
#endif
    for (int tx = blockIdx.x * 256 + threadIdx.x; tx < total; tx += gridDim.x * 256) hdr_patch<FMT, HLG>(a, P, tab, tx, per_row);
}

// -DHDR_WG_QUARTERS=q caps the grid at q / 4 workgroups per compute unit, each then walking several rounds of patches (what profiles/hdr_price.md measured
// the amortised grids with); the library is built without a cap
#ifdef HDR_WG_QUARTERS
// compute units of the current device (asked once per device; 256 where the runtime does not say)
static int hdr_compute_units() {
    static int units[16];
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    if (units[dev]) return units[dev];
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return units[dev] = n;
}
#endif
// fmt: 14 P010, 15 I420_10, 16 V210; hlg: the block's transfer is 18 (the OOTF step is compiled in), else PQ; planes / strides as k_launch_csc2's; d_tables: the HDR_WORDS words of mi355enc_hdr_tables on the device.
// -1: not a format of this file, or arguments outside what the kernel's addressing holds for.
int k_launch_hdr(int fmt, int hlg, const uint8_t *const planes[3], const int strides[3], uint8_t *dy, uint8_t *duv, int vw, int vh, int W, int H, const int *d_tables, hipStream_t s) {
    if (!planes || !strides || !planes[0] || !dy || !duv || !d_tables || vw < 2 || vh < 2 || ((vw | vh) & 1) || W < vw || H < vh || (W & 7) || (H & 1)) return -1;
    if ((((uintptr_t)dy) | ((uintptr_t)duv)) & 7) return -1;
    if ((fmt == 14 && !planes[1]) || (fmt == 15 && (!planes[1] || !planes[2]))) return -1;
    hdr_args a;
    a.p0 = planes[0]; a.p1 = planes[1]; a.p2 = planes[2]; a.s0 = strides[0]; a.s1 = strides[1]; a.s2 = strides[2];
    a.dy = dy; a.duv = duv; a.vw = vw; a.vh = vh; a.W = W; a.H = H; a.tab = d_tables;
    const int pw = fmt == 16 ? 24 : 8, need = (((W + pw - 1) / pw) * (H >> 1) + 255) / 256;
#ifdef HDR_WG_QUARTERS
    const int cap = hdr_compute_units() * HDR_WG_QUARTERS / 4;
    const dim3 g(need < cap ? need : cap > 0 ? cap : 1), b(256);
#else
    const dim3 g(need), b(256); // one patch per thread: every workgroup stages the block for its 256 patches (fewer, longer-walking workgroups measured slower)
#endif
    switch (fmt) {
    case 14: if (hlg) hipLaunchKernelGGL((hdr_kernel<14, true>), g, b, 0, s, a); else hipLaunchKernelGGL((hdr_kernel<14, false>), g, b, 0, s, a); break;
    case 15: if (hlg) hipLaunchKernelGGL((hdr_kernel<15, true>), g, b, 0, s, a); else hipLaunchKernelGGL((hdr_kernel<15, false>), g, b, 0, s, a); break;
    case 16: if (hlg) hipLaunchKernelGGL((hdr_kernel<16, true>), g, b, 0, s, a); else hipLaunchKernelGGL((hdr_kernel<16, false>), g, b, 0, s, a); break;
    default: return -1;
    }
    return 0;
}
