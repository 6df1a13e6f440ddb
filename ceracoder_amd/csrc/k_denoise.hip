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

// =================================================================== motion compensation
// denoise_search_kernel: per aligned 8 x 8 luma block the whole-sample vector into the history, by full search over the history's codes Q = (H + 8) >> 4.
// A workgroup of four waves covers a tile of 64 x 32 samples (8 x 4 blocks); the window -- the tile with an apron of the range above and below and of the range
// rounded up to a whole word left and right, plus one word, and the rows of the dy that fill the last group -- is converted from the uint16 history to bytes
// while it is staged into LDS (at most 66 rows of 25
// words, 6600 bytes).  A wave takes the tile's blocks one after the other: the block's sixteen source dwords are wave-uniform (lanes 0 .. 7 load a row each, sixteen
// v_readlane bring them to SGPRs), and a lane owns the four adjacent dx of one word column at K consecutive dy -- v_qsad_pk_u16_u8 gives the four SADs of a dy from
// three window words a row, all word-aligned, and a window row read once serves the lane's K dy (K = 5 above range 8: 7 x 9 = 63 tasks at range 16, one pass of the
// wave; K = 2 up to it, K = 1 up to range 4).  The keys of the candidates whose block would leave the surface or the range are all ones; the wave minimum of the key (six v_min_u32 DPP steps)
// is the block's result: keys are unique, so there is no tie logic and the order of evaluation does not matter.  Window words outside the surface are zero and are
// only ever read for candidates that are left out.  No atomics, no waits, no scratch; every loop is bounded by the range.
#define DS_STRIDE 25 // words per window row: (64 + 2 * 16) / 4 + 1; odd: consecutive dy start 25 banks apart
#define DS_LEFT_OUT 0x50000000u
#define DS_ROWS 66   // 31 + 5 * 7: the tile's 32 rows, and 35 dy in seven groups of five at range 16

struct ds_args {
    const uint8_t *y;
    const uint16_t *hy;
    unsigned *vec;
    int W, H, vw, vh, range, lambda;
};

DEV unsigned long long dn_qsad(unsigned lo, unsigned hi, unsigned cur, unsigned long long acc) {
    return __builtin_amdgcn_qsad_pk_u16_u8(((unsigned long long)hi << 32) | lo, cur, acc);
}

template <int K>
__global__ __launch_bounds__(256) void denoise_search_kernel(ds_args a) {
    __shared__ unsigned win[DS_ROWS * DS_STRIDE];
    const int R = a.range, RP = (R + 3) & ~3, W = a.W, H = a.H;
    const int tiles_x = (W + 63) >> 6, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int NG = (2 * R + K) / K; // groups of K dy: the last may reach past the range; those dy are left out, their rows staged like the others
    const int ox = 64 * tx - RP, oy = 32 * ty - R, ww = 17 + (RP >> 1), rows = 31 + K * NG;
    for (int i = threadIdx.x; i < rows * ww; i += 256) {
        const int r = i / ww, q = i - r * ww, gy = oy + r, gx = ox + 4 * q; // (gx is a multiple of 4 and W one of 16: a word lies inside or outside as a whole)
        unsigned v = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const uint2 hw = ldg64(a.hy + (size_t)gy * W + gx);
            const unsigned t0 = hw.x + 0x00080008u, t1 = hw.y + 0x00080008u;
            v = ((t0 >> 4) & 255u) | (((t0 >> 20) & 255u) << 8) | (((t1 >> 4) & 255u) << 16) | (((t1 >> 20) & 255u) << 24);
        }
        win[r * DS_STRIDE + q] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nbx = W >> 3, nby = H >> 3, vbx = (a.vw - 1) >> 3, vby = (a.vh - 1) >> 3;
    const int G = (RP >> 1) + 1, ntask = NG * G; // G word columns of four dx each: dx = -RP + 4 g + o; a lane's task: one column, K dy
    for (int k = 0; k < 8; k++) {
        const int bi = wv + 4 * k, bxi = bi & 7, byi = bi >> 3, bx = 8 * tx + bxi, by = 4 * ty + byi; // (wave-uniform)
        if (bx >= nbx || by >= nby) continue;
        if (bx > vbx || by > vby) { // a block without a visible sample has no vector: the filter replicates into it
            if (lane == 0) stg32(a.vec + (size_t)by * nbx + bx, 0u);
            continue;
        }
        const int X = 8 * bx, Y = 8 * by;
        uint2 cv = make_uint2(0, 0);
        if (lane < 8) cv = ldg64(a.y + (size_t)(Y + lane) * W + X);
        unsigned c[8][2];
#pragma unroll
        for (int r = 0; r < 8; r++) { c[r][0] = (unsigned)__builtin_amdgcn_readlane((int)cv.x, r); c[r][1] = (unsigned)__builtin_amdgcn_readlane((int)cv.y, r); }
        unsigned best = 0xFFFFFFFFu;
        for (int t = lane; t < ntask; t += 64) {
            const int dg = t / G, g = t - dg * G, dyi0 = K * dg, dx0 = 4 * g - RP;
            const unsigned *wp = &win[(8 * byi + dyi0) * DS_STRIDE + 2 * bxi + g];
            unsigned long long acc[K];
#pragma unroll
            for (int d = 0; d < K; d++) acc[d] = 0;
#pragma unroll
            for (int j = 0; j < 8 + K - 1; j++) { // a window row serves the K dy of the lane
                const unsigned w0 = wp[j * DS_STRIDE], w1 = wp[j * DS_STRIDE + 1], w2 = wp[j * DS_STRIDE + 2];
#pragma unroll
                for (int d = 0; d < K; d++) {
                    const int r = j - d;
                    if (r >= 0 && r < 8) { acc[d] = dn_qsad(w0, w1, c[r][0], acc[d]); acc[d] = dn_qsad(w1, w2, c[r][1], acc[d]); }
                }
            }
            // the key is a sum of the cost's, the row's and the column's part: none of its two fields overflows into the other.  A part left out is DS_LEFT_OUT,
            // above every key (at most 20416 << 16 | 65535) and small enough for two of them and a cost to stay below 2^32
            unsigned kx[4];
#pragma unroll
            for (int o = 0; o < 4; o++) {
                const int dx = dx0 + o, ax = dn_abs(dx);
                kx[o] = dx >= -R && dx <= R && X + dx >= 0 && X + dx <= W - 8 ? ((unsigned)(a.lambda * ax) << 16) + (unsigned)(ax * 1089 + dx) : DS_LEFT_OUT;
            }
#pragma unroll
            for (int d = 0; d < K; d++) {
                const int dy = dyi0 + d - R, ay = dn_abs(dy);
                const unsigned ky = dy <= R && Y + dy >= 0 && Y + dy <= H - 8 ? ((unsigned)(a.lambda * ay) << 16) + (unsigned)(ay * 1089 + (dy + 16) * 33 + 16) : DS_LEFT_OUT;
                const unsigned lo = (unsigned)acc[d], hi = (unsigned)(acc[d] >> 32);
                best = min(best, min(min((lo << 16) + ky + kx[0], (lo & 0xFFFF0000u) + ky + kx[1]), min((hi << 16) + ky + kx[2], (hi & 0xFFFF0000u) + ky + kx[3])));
            }
        }
        best = wave64_umin(best); // (0, 0) is always a candidate
        if (lane == 0) {
            const int rem = (int)(best & 0xFFFFu) % 1089, dy = rem / 33 - 16, dx = rem % 33 - 16;
            const unsigned m = (best >> 16) - (unsigned)(a.lambda * (dn_abs(dx) + dn_abs(dy)));
            stg32(a.vec + (size_t)by * nbx + bx, ((unsigned)dx & 255u) | (((unsigned)dy & 255u) << 8) | (m << 16));
        }
    }
}

// denoise_mc_kernel: denoise_kernel's arithmetic and ownership with the history read from one buffer at the block's vector and written to another at the sample's
// own place (displaced reads cross the patches other threads own, so the history cannot be updated in place; the slot's surfaces can: a thread reads only its own
// patch's samples before it writes them).  M and the vector come from the search's entry of the block.  LM, CM as above; launched only when something is filtered.
struct dmc_args {
    uint8_t *y, *uv;
    const uint16_t *hy, *huv;
    uint16_t *ny, *nuv;
    const unsigned *vec;
    int W, H, vw, vh;
    dn_tab tab;
};

// eight history samples from element e of a row as four words: the row is read as aligned words, one more when e is odd (then e + 8 still lies in the row: e + 7 is
// even and at most W - 2)
DEV uint4 dn_hist8(const uint16_t *row, int e) {
    const uint16_t *p = row + (e & ~1);
    const unsigned w0 = ldg32(p), w1 = ldg32(p + 2), w2 = ldg32(p + 4), w3 = ldg32(p + 6);
    if (!(e & 1)) return make_uint4(w0, w1, w2, w3);
    const unsigned w4 = ldg32(p + 8);
    return make_uint4((w0 >> 16) | (w1 << 16), (w1 >> 16) | (w2 << 16), (w2 >> 16) | (w3 << 16), (w3 >> 16) | (w4 << 16));
}
// four chroma pairs (a word each) from pair-aligned element e of a row, and with fx the four one pair further
DEV void dn_pairs(const uint16_t *row, int e, int fx, uint4 &a, uint4 &b) {
    const uint16_t *p = row + e;
    a = make_uint4(ldg32(p), ldg32(p + 2), ldg32(p + 4), ldg32(p + 6));
    b = a;
    if (fx) b = make_uint4(a.y, a.z, a.w, ldg32(p + 8));
}
// per 16-bit half, values up to 4080: the rounded mean of two and of four (the sums stay below 2^16: no carry between the halves)
DEV unsigned dn_avg2(unsigned a, unsigned b) { return ((a + b + 0x00010001u) >> 1) & 0x7FFF7FFFu; }
DEV unsigned dn_avg4(unsigned a, unsigned b, unsigned c, unsigned d) { return ((a + b + c + d + 0x00020002u) >> 2) & 0x3FFF3FFFu; }

template <int LM, int CM>
__global__ __launch_bounds__(256) void denoise_mc_kernel(dmc_args a) {
    static_assert(LM == 1 || CM == 2, "something is filtered");
    __shared__ unsigned tab[192];
    if (threadIdx.x < 64) {
#pragma unroll
        for (int k = 0; k < 3; k++) tab[threadIdx.x + 64 * k] = a.tab.w[threadIdx.x + 64 * k];
    }
    __syncthreads();
    const uint8_t *tb = (const uint8_t *)tab, *tl = tb + 256, *tc = tb + 512;
    const int t = blockIdx.x * 256 + threadIdx.x, blk = t >> 2, sub = t & 3, nbx = a.W >> 3, nby = a.H >> 3;
    if (blk >= nbx * nby) return;
    const int by = blk / nbx, bx = blk - by * nbx, vbx = (a.vw - 1) >> 3, vby = (a.vh - 1) >> 3;
    if (bx > vbx || by > vby) return; // a block without a visible sample: stored by the owner of its clamped position, below
    const int x0 = 8 * bx, y0 = 8 * by + 2 * sub, W = a.W;
    const size_t at = (size_t)y0 * W + x0, cat = (size_t)(y0 >> 1) * W + x0;
    uint8_t *py = a.y + at, *pc = a.uv + cat;
    uint16_t *ph = a.ny + at, *pch = CM ? a.nuv + cat : nullptr;
    const unsigned ve = ldg32(a.vec + blk);
    const int dx = (int)(int8_t)(ve & 255u), dy = (int)(int8_t)((ve >> 8) & 255u);
    const int b = tb[min(255u, ve >> 20)]; // M >> 4
    // everything the thread reads, before any store
    const uint2 s0 = ldg64(py), s1 = ldg64(py + W);
    uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0, hc = h0;
    uint2 sc = make_uint2(0, 0);
    if (LM == 1) { h0 = dn_hist8(a.hy + (size_t)(y0 + dy) * W, x0 + dx); h1 = dn_hist8(a.hy + (size_t)(y0 + 1 + dy) * W, x0 + dx); }
    if (CM) sc = ldg64(pc);
    if (CM == 2) { // H.264's chroma prediction for a whole-sample luma vector, on the history: whole pairs, or the rounded mean of two / four
        const int fx = dx & 1, fy = dy & 1;
        const uint16_t *row = a.huv + (size_t)((y0 >> 1) + (dy >> 1)) * W;
        uint4 p, q;
        dn_pairs(row, x0 + 2 * (dx >> 1), fx, p, q);
        if (fy) {
            uint4 r, s;
            dn_pairs(row + W, x0 + 2 * (dx >> 1), fx, r, s);
            if (fx) hc = make_uint4(dn_avg4(p.x, q.x, r.x, s.x), dn_avg4(p.y, q.y, r.y, s.y), dn_avg4(p.z, q.z, r.z, s.z), dn_avg4(p.w, q.w, r.w, s.w));
            else hc = make_uint4(dn_avg2(p.x, r.x), dn_avg2(p.y, r.y), dn_avg2(p.z, r.z), dn_avg2(p.w, r.w));
        } else if (fx) hc = make_uint4(dn_avg2(p.x, q.x), dn_avg2(p.y, q.y), dn_avg2(p.z, q.z), dn_avg2(p.w, q.w));
        else hc = p;
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
    // the blocks beside and below without a visible sample: replicas, as denoise_kernel stores them
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
            stg128(a.ny + bat + (size_t)j * W, n1);
            if (right) {
                if (LM == 1) stg64(a.y + bat + (size_t)j * W + 8, make_uint2(ry1, ry1));
                stg128(a.ny + bat + (size_t)j * W + 8, make_uint4(rh1, rh1, rh1, rh1));
            }
        }
        for (int j = 0; CM && j < 4; j++) {
            if (CM == 2) stg64(a.uv + bcat + (size_t)j * W, oc);
            stg128(a.nuv + bcat + (size_t)j * W, nc);
            if (right) {
                if (CM == 2) stg64(a.uv + bcat + (size_t)j * W + 8, make_uint2(rc, rc));
                stg128(a.nuv + bcat + (size_t)j * W + 8, make_uint4(rhc, rhc, rhc, rhc));
            }
        }
    }
}

// The search alone: y the luma surface, hy its history (both as in k_launch_denoise), vec: (W / 8) (H / 8) words, one per block in raster order -- dx in byte 0, dy
// in byte 1 (int8), the vector's cost M in the high half; zero for a block without a visible sample.  range 1 .. 16; lambda: the penalty per sample of vector
// length, at most 128.  -1: arguments outside that.
int k_launch_denoise_search(const uint8_t *y, const uint16_t *hy, unsigned *vec, int W, int H, int vw, int vh, int range, int lambda, hipStream_t s) {
    if (!y || !hy || !vec || W <= 0 || H <= 0 || (W & 15) || (H & 15) || ((vw | vh) & 1) || vw > W || vw <= W - 16 || vh > H || vh <= H - 16) return -1;
    if ((((uintptr_t)y) & 7) || (((uintptr_t)hy) & 15) || (((uintptr_t)vec) & 3) || range < 1 || range > 16 || lambda < 0 || lambda > 128) return -1;
    ds_args a;
    a.y = y; a.hy = hy; a.vec = vec; a.W = W; a.H = H; a.vw = vw; a.vh = vh; a.range = range; a.lambda = lambda;
    // K dy a lane: 5 above range 8 (at 16: 7 x 9 = 63 tasks, one pass of the wave), 2 up to it (at 8: 9 x 5 = 45), 1 up to 4 (at 4: 9 x 3 = 27)
    const dim3 g(((W + 63) >> 6) * ((H + 31) >> 5));
    if (range > 8) hipLaunchKernelGGL(denoise_search_kernel<5>, g, dim3(256), 0, s, a);
    else if (range > 4) hipLaunchKernelGGL(denoise_search_kernel<2>, g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(denoise_search_kernel<1>, g, dim3(256), 0, s, a);
    return 0;
}

// The compensated filter: k_launch_denoise's arguments with the histories read (hy, huv) and written (ny, nuv: other buffers of the same layout) apart and the
// search's vec.  lmode, cmode as there, with something filtered (lmode 1 or cmode 2); huv is needed with cmode 2, nuv with cmode 1 or 2.  -1: arguments outside that.
int k_launch_denoise_mc(uint8_t *y, uint8_t *uv, const uint16_t *hy, const uint16_t *huv, uint16_t *ny, uint16_t *nuv, const unsigned *vec, int W, int H, int vw, int vh,
                        int lmode, int cmode, const uint8_t *tabs, hipStream_t s) {
    if (!y || !uv || !hy || !ny || !vec || !tabs || (cmode == 2 && !huv) || (cmode && !nuv) || W <= 0 || H <= 0 || (W & 15) || (H & 15)) return -1;
    if (((vw | vh) & 1) || vw > W || vw <= W - 16 || vh > H || vh <= H - 16 || (lmode | 1) != 1 || cmode < 0 || cmode > 2 || (lmode != 1 && cmode != 2)) return -1;
    if (((((uintptr_t)y) | ((uintptr_t)uv)) & 7) || ((((uintptr_t)hy) | ((uintptr_t)huv) | ((uintptr_t)ny) | ((uintptr_t)nuv)) & 15) || (((uintptr_t)vec) & 3)) return -1;
    if (hy == ny || (cmode == 2 && huv == nuv)) return -1;
    dmc_args a;
    a.y = y; a.uv = uv; a.hy = hy; a.huv = huv; a.ny = ny; a.nuv = nuv; a.vec = vec; a.W = W; a.H = H; a.vw = vw; a.vh = vh;
    memcpy(a.tab.w, tabs, 768);
    const dim3 g(((W >> 3) * (H >> 3) * 4 + 255) / 256), b(256);
    switch (3 * lmode + cmode) {
    case 2: hipLaunchKernelGGL((denoise_mc_kernel<0, 2>), g, b, 0, s, a); break;
    case 3: hipLaunchKernelGGL((denoise_mc_kernel<1, 0>), g, b, 0, s, a); break;
    case 4: hipLaunchKernelGGL((denoise_mc_kernel<1, 1>), g, b, 0, s, a); break;
    default: hipLaunchKernelGGL((denoise_mc_kernel<1, 2>), g, b, 0, s, a); break;
    }
    return 0;
}
