// k_denoise.hip -- temporal noise reduction on the coded NV12 surfaces of a slot: a motion-adaptive recursive filter against a history
// of one uint16 per sample in sixteenths of a code, in place on both.
//
// Ownership is yuv_convert_kernel's and adjust_point_kernel's: a thread owns an 8 x 2 luma patch, its four chroma pairs and the history of both, loads all of it
// (8- and 16-byte loads) before it stores any of it, and no other thread reads or writes it -- which is what makes one history buffer and no scratch plane
// enough.  The four threads of an aligned 8 x 8 block are four adjacent lanes (a quad) of one wave and exchange only their partial sums of the block measure M,
// by two quad permutes (DPP): no LDS, no barrier for it.
//
// An 8 x 8 block without a visible sample (rows 1080 .. 1087 of a 1080-line picture) takes out and H' of its clamped visible position.  Its threads do nothing:
// reading the clamped block's samples would race with their owner's stores.  Instead the owner of the last visible column / row of the block beside / above it
// stores its own result there too, replicated -- only those threads pay the extra stores, and the ownership stays strict.
//
// LM 1: the luma is filtered; 0: it primes or only follows (out = c: the slot's luma is not written; H' = 16 c).  CM 2: the chroma is filtered; 1: it primes (the
// slot's chroma is read, not written); 0: off, neither read nor written.  With nothing filtered there is no measure: no table, no history read.
//
// The three 256-byte tables travel by value as 192 dwords; the first wave copies them into LDS (a by-value array indexed per lane by a sample would live in
// scratch), and a look-up is one ds_read_u8.  No scratch, no atomics, no wait.
#include "kernels_common.hpp"

#include <cstring>

struct dn_tab { unsigned w[192]; }; // B, the luma's P, the chroma's P

struct dn_args {
    uint8_t *y, *uv;
    uint16_t *hy, *huv;
    int W, H, vw, vh;
    dn_tab tab;
};

DEV unsigned dn_pick2(uint2 v, int i) { return i ? v.y : v.x; }
DEV unsigned dn_pick4(uint4 v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
DEV int dn_abs(int v) { return v < 0 ? -v : v; }
DEV int dn_quad_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false); // quad_perm:[1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false); // quad_perm:[2,3,0,1]
    return v;
}
// one sample: c the input code, h its history; b the block's weight, p the table of its plane.  Returns H' (out = (H' + 8) >> 4)
DEV int dn_one(int c, int h, int b, const uint8_t *p) {
    const int d = dn_abs(c - ((h + 8) >> 4)), k = (b * (int)p[d] + 128) >> 8;
    return 16 * c + ((k * (h - 16 * c) + 128) >> 8);
}
// four samples of the word c against the history words h0 (samples 0, 1), h1 (2, 3): the new history words, and the output word
template <bool FILTER> DEV unsigned dn_four(unsigned c, unsigned h0, unsigned h1, int b, const uint8_t *p, unsigned &n0, unsigned &n1) {
    if (!FILTER) {
        n0 = (byte_of(c, 0) << 4) | (byte_of(c, 1) << 20);
        n1 = (byte_of(c, 2) << 4) | (byte_of(c, 3) << 20);
        return c;
    }
    const int a0 = dn_one(byte_of(c, 0), (int)(h0 & 0xffffu), b, p), a1 = dn_one(byte_of(c, 1), (int)(h0 >> 16), b, p);
    const int a2 = dn_one(byte_of(c, 2), (int)(h1 & 0xffffu), b, p), a3 = dn_one(byte_of(c, 3), (int)(h1 >> 16), b, p);
    n0 = (unsigned)a0 | ((unsigned)a1 << 16);
    n1 = (unsigned)a2 | ((unsigned)a3 << 16);
    return (unsigned)((a0 + 8) >> 4) | ((unsigned)((a1 + 8) >> 4) << 8) | ((unsigned)((a2 + 8) >> 4) << 16) | ((unsigned)((a3 + 8) >> 4) << 24);
}
// sum |c - ((H + 8) >> 4)| over the four samples of a word
DEV int dn_measure4(unsigned c, unsigned h0, unsigned h1) {
    return dn_abs(byte_of(c, 0) - (int)(((h0 & 0xffffu) + 8) >> 4)) + dn_abs(byte_of(c, 1) - (int)(((h0 >> 16) + 8) >> 4)) +
           dn_abs(byte_of(c, 2) - (int)(((h1 & 0xffffu) + 8) >> 4)) + dn_abs(byte_of(c, 3) - (int)(((h1 >> 16) + 8) >> 4));
}

template <int LM, int CM>
__global__ __launch_bounds__(256) void denoise_kernel(dn_args a) {
    constexpr bool MEASURE = LM == 1 || CM == 2;
    __shared__ unsigned tab[MEASURE ? 192 : 1];
    if (MEASURE) {
        if (threadIdx.x < 64) {
#pragma unroll
            for (int k = 0; k < 3; k++) tab[threadIdx.x + 64 * k] = a.tab.w[threadIdx.x + 64 * k];
        }
        __syncthreads();
    }
    const uint8_t *tb = (const uint8_t *)tab, *tl = tb + 256, *tc = tb + 512;
    const int t = blockIdx.x * 256 + threadIdx.x, blk = t >> 2, sub = t & 3, nbx = a.W >> 3, nby = a.H >> 3;
    if (blk >= nbx * nby) return; // (a whole quad: the four lanes of a block stay or leave together)
    const int by = blk / nbx, bx = blk - by * nbx, vbx = (a.vw - 1) >> 3, vby = (a.vh - 1) >> 3;
    if (bx > vbx || by > vby) return; // a block without a visible sample: stored by the owner of its clamped position, below
    const int x0 = 8 * bx, y0 = 8 * by + 2 * sub, W = a.W;
    const size_t at = (size_t)y0 * W + x0, cat = (size_t)(y0 >> 1) * W + x0;
    uint8_t *py = a.y + at, *pc = a.uv + cat;
    uint16_t *ph = a.hy + at, *pch = CM ? a.huv + cat : nullptr;
    // everything the thread owns, before any store
    const uint2 s0 = ldg64(py), s1 = ldg64(py + W);
    uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0, hc = h0;
    uint2 sc = make_uint2(0, 0);
    if (MEASURE) { h0 = ldg128(ph); h1 = ldg128(ph + W); }
    if (CM) sc = ldg64(pc);
    if (CM == 2) hc = ldg128(pch);
    int b = 0;
    if (MEASURE) {
        const int m = dn_quad_sum(dn_measure4(s0.x, h0.x, h0.y) + dn_measure4(s0.y, h0.z, h0.w) + dn_measure4(s1.x, h1.x, h1.y) + dn_measure4(s1.y, h1.z, h1.w));
        b = tb[min(255, m >> 4)];
    }
    uint4 n0, n1, nc;
    uint2 o0, o1, oc;
    o0.x = dn_four<LM == 1>(s0.x, h0.x, h0.y, b, tl, n0.x, n0.y); o0.y = dn_four<LM == 1>(s0.y, h0.z, h0.w, b, tl, n0.z, n0.w);
    o1.x = dn_four<LM == 1>(s1.x, h1.x, h1.y, b, tl, n1.x, n1.y); o1.y = dn_four<LM == 1>(s1.y, h1.z, h1.w, b, tl, n1.z, n1.w);
    if (LM == 1) { stg64(py, o0); stg64(py + W, o1); }
    stg128(ph, n0); stg128(ph + W, n1);
    if (CM) {
        oc.x = dn_four<CM == 2>(sc.x, hc.x, hc.y, b, tc, nc.x, nc.y); oc.y = dn_four<CM == 2>(sc.y, hc.z, hc.w, b, tc, nc.z, nc.w);
        if (CM == 2) stg64(pc, oc);
        stg128(pch, nc);
    }
    // the blocks beside and below without a visible sample: replicas of the last visible column (vw - 1, odd: the high half of its history word, the second byte
    // of its chroma pair's column) and of the last visible row (vh - 1, odd: the thread's second row)
    const bool right = bx == vbx && vbx < nbx - 1, below = by == vby && vby < nby - 1 && sub == (((a.vh - 1) & 7) >> 1);
    if (!right && !below) return;
    const int lx = (a.vw - 1) & 7, pr = lx >> 1;
    const unsigned ry0 = ((dn_pick2(o0, lx >> 2) >> (8 * (lx & 3))) & 255u) * 0x01010101u, ry1 = ((dn_pick2(o1, lx >> 2) >> (8 * (lx & 3))) & 255u) * 0x01010101u;
    const unsigned rh0 = (dn_pick4(n0, pr) >> 16) * 0x00010001u, rh1 = (dn_pick4(n1, pr) >> 16) * 0x00010001u;
    unsigned rc = 0, rhc = 0;
    if (CM) { rc = ((dn_pick2(oc, pr >> 1) >> (16 * (pr & 1))) & 0xffffu) * 0x00010001u; rhc = dn_pick4(nc, pr); }
    if (right) {
        if (LM == 1) { stg64(py + 8, make_uint2(ry0, ry0)); stg64(py + W + 8, make_uint2(ry1, ry1)); }
        stg128(ph + 8, make_uint4(rh0, rh0, rh0, rh0)); stg128(ph + W + 8, make_uint4(rh1, rh1, rh1, rh1));
        if (CM == 2) stg64(pc + 8, make_uint2(rc, rc));
        if (CM) stg128(pch + 8, make_uint4(rhc, rhc, rhc, rhc));
    }
    if (below) {
        const size_t bat = (size_t)(8 * (by + 1)) * W + x0, bcat = (size_t)(4 * (by + 1)) * W + x0;
        for (int j = 0; j < 8; j++) {
            if (LM == 1) stg64(a.y + bat + (size_t)j * W, o1);
            stg128(a.hy + bat + (size_t)j * W, n1);
            if (right) {
                if (LM == 1) stg64(a.y + bat + (size_t)j * W + 8, make_uint2(ry1, ry1));
                stg128(a.hy + bat + (size_t)j * W + 8, make_uint4(rh1, rh1, rh1, rh1));
            }
        }
        for (int j = 0; CM && j < 4; j++) {
            if (CM == 2) stg64(a.uv + bcat + (size_t)j * W, oc);
            stg128(a.huv + bcat + (size_t)j * W, nc);
            if (right) {
                if (CM == 2) stg64(a.uv + bcat + (size_t)j * W + 8, make_uint2(rc, rc));
                stg128(a.huv + bcat + (size_t)j * W + 8, make_uint4(rhc, rhc, rhc, rhc));
            }
        }
    }
}

// y, uv: NV12 surfaces of W x H (multiples of 16) at stride W, 8-byte aligned; hy, huv: their histories, uint16 per sample in the same layout, 16-byte aligned
// (huv: null with cmode 0); vw x vh: the visible size, even, less than 16 short of W x H.  lmode 1: the luma is filtered, 0: it primes / follows; cmode 2: the
// chroma is filtered, 1: it primes, 0: off.  tabs: the 768 bytes of B, the luma's P and the chroma's P (needed when anything is filtered).  -1: arguments outside that.
int k_launch_denoise(uint8_t *y, uint8_t *uv, uint16_t *hy, uint16_t *huv, int W, int H, int vw, int vh, int lmode, int cmode, const uint8_t *tabs, hipStream_t s) {
    if (!y || !uv || !hy || (cmode && !huv) || W <= 0 || H <= 0 || (W & 15) || (H & 15) || ((vw | vh) & 1) || vw > W || vw <= W - 16 || vh > H || vh <= H - 16) return -1;
    if (((((uintptr_t)y) | ((uintptr_t)uv)) & 7) || ((((uintptr_t)hy) | ((uintptr_t)huv)) & 15) || (lmode | 1) != 1 || cmode < 0 || cmode > 2) return -1;
    const bool measure = lmode == 1 || cmode == 2;
    if (measure && !tabs) return -1;
    dn_args a;
    a.y = y; a.uv = uv; a.hy = hy; a.huv = huv; a.W = W; a.H = H; a.vw = vw; a.vh = vh;
    if (measure) memcpy(a.tab.w, tabs, 768); else memset(a.tab.w, 0, 768);
    const dim3 g(((W >> 3) * (H >> 3) * 4 + 255) / 256), b(256);
    switch (3 * lmode + cmode) {
    case 0: hipLaunchKernelGGL((denoise_kernel<0, 0>), g, b, 0, s, a); break;
    case 1: hipLaunchKernelGGL((denoise_kernel<0, 1>), g, b, 0, s, a); break;
    case 2: hipLaunchKernelGGL((denoise_kernel<0, 2>), g, b, 0, s, a); break;
    case 3: hipLaunchKernelGGL((denoise_kernel<1, 0>), g, b, 0, s, a); break;
    case 4: hipLaunchKernelGGL((denoise_kernel<1, 1>), g, b, 0, s, a); break;
    default: hipLaunchKernelGGL((denoise_kernel<1, 2>), g, b, 0, s, a); break;
    }
    return 0;
}
