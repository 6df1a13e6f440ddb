// k_csc.hip -- input conversion to NV12 for the formats csc_kernel (k_handover.hip) does not take: planar 4:2:2 / 4:4:4 (Y42B, Y444), NV21, and
// RGB in six byte orders (DESIGN.md section 11 states the rule).  Hand-written HIP for gfx950 (CDNA4, wave64); part of libmi355enc.
// Shape of csc_kernel: one thread converts an 8 x 2 luma patch and its 4 chroma pairs; on the fast path every global access is an aligned
// 4-, 8- or 16-byte word and a patch row is contiguous; the picture's edge, and planes whose address or stride is not suitably aligned,
// go byte by byte with clamped source coordinates (which also fills the coded-size margin).  Copy-shaped: 4 P or 3 P in, 1.5 P out.
#include "kernels_common.hpp"

struct csc2_args {
    const uint8_t *p0, *p1, *p2; // planar: Y, U, V (NV21: Y, VU); RGB: p0 only
    int s0, s1, s2;              // their strides in bytes
    uint8_t *dy, *duv;           // NV12 destination, coded size W x H, stride W
    int vw, vh, W, H;            // visible and coded size
    int yr, yg, yb, br, bg, bb, rr, rg, rb, off; // RGB: the matrix in 2^-16 units and the luma offset (mi355enc_csc_coefficients)
};

// Four values (each fits 16 bits) -> clipped bytes of one word through the packed 16-bit forms and v_perm, not `clip255(a) | clip255(b) << 8 | ...`:
// for that hipcc selects gfx950's v_ashr_pk_u8_i32, whose upper half is not cleared on this hardware (tests/test_abi_cpu.py).
typedef short csc_s2 __attribute__((ext_vector_type(2)));
DEV unsigned csc_pack4(int a, int b, int c, int d) {
    const csc_s2 lo = __builtin_bit_cast(csc_s2, __builtin_amdgcn_perm((unsigned)b, (unsigned)a, 0x05040100u));
    const csc_s2 hi = __builtin_bit_cast(csc_s2, __builtin_amdgcn_perm((unsigned)d, (unsigned)c, 0x05040100u));
    const csc_s2 l = __builtin_elementwise_min(__builtin_elementwise_max(lo, (csc_s2)(0)), (csc_s2)(255));
    const csc_s2 h = __builtin_elementwise_min(__builtin_elementwise_max(hi, (csc_s2)(0)), (csc_s2)(255));
    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, h), __builtin_bit_cast(unsigned, l), 0x06040200u);
}
DEV void csc_store(const csc2_args &a, int ry, int x0, const uint2 *yrow, const unsigned *uvw) {
    stg64(a.dy + (size_t)(2 * ry) * a.W + x0, yrow[0]);
    stg64(a.dy + (size_t)(2 * ry + 1) * a.W + x0, yrow[1]);
    stg64(a.duv + (size_t)ry * a.W + x0, make_uint2(uvw[0], uvw[1]));
}
// 8 luma samples of a row, the source column clamped to the visible width
DEV uint2 csc_luma_row(const uint8_t *sp, int x0, int vw, bool fast) {
    if (fast) return ldg64(sp + x0);
    unsigned w[2] = {0, 0};
    for (int i = 0; i < 8; i++) { const int sx = x0 + i < vw ? x0 + i : vw - 1; w[i >> 2] |= ldg8(sp + sx) << (8 * (i & 3)); }
    return make_uint2(w[0], w[1]);
}

// =================================================================== planar formats
// 4 Y42B: chroma half width, full height -> the rounded mean of the two rows (csc_kernel's 4:2:2 rule).  5 Y444: chroma by the [1 2 1] x [1 1]
// tap cosited with the even luma column, (sum + 4) >> 3.  7 NV21: NV12 with V before U.
template <int FMT>
__global__ __launch_bounds__(256) void csc_planar_kernel(csc2_args a) {
    const int tx = blockIdx.x * 256 + threadIdx.x, per_row = a.W >> 3, rows2 = a.H >> 1;
    if (tx >= per_row * rows2) return;
    const int ry = tx / per_row, cx = tx - ry * per_row, x0 = cx * 8;
    const bool vis = x0 + 8 <= a.vw; // visible width is even: a patch is fully visible, or clamped per byte
    const bool fast = vis && (a.s0 & 7) == 0 && (((uintptr_t)a.p0) & 7) == 0;
    const int base = 2 * ry < a.vh ? 2 * ry : a.vh - 2; // margin rows: the last chroma row (of the last two source rows), the last luma row
    uint2 yrow[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int sy = 2 * ry + r < a.vh ? 2 * ry + r : a.vh - 1;
        yrow[r] = csc_luma_row(a.p0 + (size_t)sy * a.s0, x0, a.vw, fast);
    }
    unsigned uvw[2];
    const int cw = a.vw >> 1;
    if (FMT == 7) {
        const uint8_t *sp = a.p1 + (size_t)(base >> 1) * a.s1;
        unsigned w[2];
        if (vis && (a.s1 & 7) == 0 && (((uintptr_t)a.p1) & 7) == 0) { const uint2 q = ldg64(sp + x0); w[0] = q.x; w[1] = q.y; }
        else
            for (int i = 0; i < 2; i++) {
                w[i] = 0;
                for (int k = 0; k < 2; k++) { const int c = cx * 4 + 2 * i + k < cw ? cx * 4 + 2 * i + k : cw - 1; w[i] |= (ldg8(sp + 2 * c) | (ldg8(sp + 2 * c + 1) << 8)) << (16 * k); }
            }
        uvw[0] = __builtin_amdgcn_perm(0u, w[0], 0x02030001u); // V U V U -> U V U V
        uvw[1] = __builtin_amdgcn_perm(0u, w[1], 0x02030001u);
    } else if (FMT == 4) {
        unsigned c[2][2]; // [plane][row]: 4 samples
        const bool cfast = vis && ((a.s1 | a.s2) & 3) == 0 && ((((uintptr_t)a.p1) | ((uintptr_t)a.p2)) & 3) == 0;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint8_t *up = a.p1 + (size_t)(base + r) * a.s1, *vp = a.p2 + (size_t)(base + r) * a.s2;
            if (cfast) { c[0][r] = ldg32(up + cx * 4); c[1][r] = ldg32(vp + cx * 4); }
            else {
                c[0][r] = c[1][r] = 0;
                for (int i = 0; i < 4; i++) { const int sx = cx * 4 + i < cw ? cx * 4 + i : cw - 1; c[0][r] |= ldg8(up + sx) << (8 * i); c[1][r] |= ldg8(vp + sx) << (8 * i); }
            }
        }
        const unsigned u = avg4(c[0][0], c[0][1]), v = avg4(c[1][0], c[1][1]);
        uvw[0] = __builtin_amdgcn_perm(v, u, 0x05010400u); // U0 V0 U1 V1
        uvw[1] = __builtin_amdgcn_perm(v, u, 0x07030602u); // U2 V2 U3 V3
    } else {
        int s[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}; // [plane][site]: the eight-weight sums
        const bool cfast = vis && ((a.s1 | a.s2) & 7) == 0 && ((((uintptr_t)a.p1) | ((uintptr_t)a.p2)) & 7) == 0;
#pragma unroll
        for (int pl = 0; pl < 2; pl++)
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const uint8_t *sp = (pl ? a.p2 : a.p1) + (size_t)(base + r) * (pl ? a.s2 : a.s1);
                if (cfast) {
                    const uint2 q = ldg64(sp + x0);
                    const int left = (int)ldg8(sp + (x0 ? x0 - 1 : 0)); // the column left of the patch: read here, not taken from a neighbouring lane
                    const unsigned w[2] = {q.x, q.y};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int m = 2 * i, l = i ? byte_of(w[(m - 1) >> 2], (m - 1) & 3) : left;
                        s[pl][i] += l + 2 * byte_of(w[m >> 2], m & 3) + byte_of(w[(m + 1) >> 2], (m + 1) & 3);
                    }
                } else
                    for (int i = 0; i < 4; i++) {
                        const int c2 = 2 * (cx * 4 + i < cw ? cx * 4 + i : cw - 1); // <= vw - 2: only the left tap can leave the picture
                        s[pl][i] += (int)ldg8(sp + (c2 ? c2 - 1 : 0)) + 2 * (int)ldg8(sp + c2) + (int)ldg8(sp + c2 + 1);
                    }
            }
        uvw[0] = pack4((s[0][0] + 4) >> 3, (s[1][0] + 4) >> 3, (s[0][1] + 4) >> 3, (s[1][1] + 4) >> 3); // sums <= 2040: no clip, every byte in range
        uvw[1] = pack4((s[0][2] + 4) >> 3, (s[1][2] + 4) >> 3, (s[0][3] + 4) >> 3, (s[1][3] + 4) >> 3);
    }
    csc_store(a, ry, x0, yrow, uvw);
}

// =================================================================== RGB
// BPP 4 or 3 bytes per pixel; RO, GO, BO: the byte of each component inside a pixel.  Luma per pixel, chroma per 2 x 2 site from the
// [1 2 1] x [1 1] sums of R, G and B (the sum is taken before the matrix: one matrix product per site).
template <int BPP> DEV unsigned rgb_px(const uint8_t *sp, int x) { // the pixel's bytes in the low 24 / 32 bits, byte by byte
    unsigned v = ldg8(sp + BPP * x) | (ldg8(sp + BPP * x + 1) << 8) | (ldg8(sp + BPP * x + 2) << 16);
    if (BPP == 4) v |= ldg8(sp + 4 * x + 3) << 24;
    return v;
}
template <int BPP, int RO, int GO, int BO>
__global__ __launch_bounds__(256) void csc_rgb_kernel(csc2_args a) {
    const int tx = blockIdx.x * 256 + threadIdx.x, per_row = a.W >> 3, rows2 = a.H >> 1;
    if (tx >= per_row * rows2) return;
    const int ry = tx / per_row, cx = tx - ry * per_row, x0 = cx * 8;
    constexpr int AL = BPP == 4 ? 15 : 7; // a patch row is 32 bytes at 32 cx, or 24 bytes at 24 cx
    // fast: the patch lies inside the visible picture (its rows are then the chroma rows as well) and its rows can be read as aligned words
    const bool fast = x0 + 8 <= a.vw && 2 * ry < a.vh && (a.s0 & AL) == 0 && (((uintptr_t)a.p0) & AL) == 0;
    const int cw = a.vw >> 1, base = 2 * ry < a.vh ? 2 * ry : a.vh - 2;
    uint2 yrow[2];
    int sr[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
    const int yoff = (a.off << 16) + (1 << 15);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        unsigned px[9]; // [0]: the pixel left of the patch (the picture's first column repeats itself), [1 + i]: pixel i
        if (fast) {
            const uint8_t *sp = a.p0 + (size_t)(2 * ry + r) * a.s0 + BPP * x0;
            if (BPP == 4) {
                const uint4 q0 = ldg128(sp), q1 = ldg128(sp + 16);
                px[1] = q0.x; px[2] = q0.y; px[3] = q0.z; px[4] = q0.w; px[5] = q1.x; px[6] = q1.y; px[7] = q1.z; px[8] = q1.w;
                px[0] = cx ? ldg32(sp - 4) : px[1];
            } else {
                const uint2 q0 = ldg64(sp), q1 = ldg64(sp + 8), q2 = ldg64(sp + 16);
                const unsigned w[6] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y};
#pragma unroll
                for (int i = 0; i < 8; i++) { // byte 3 i of the row: inside one word, or across two (v_alignbyte)
                    const int o = 3 * i;
                    px[1 + i] = (o & 3) <= 1 ? w[o >> 2] >> (8 * (o & 3)) : __builtin_amdgcn_alignbyte(w[(o >> 2) + 1], w[o >> 2], (unsigned)(o & 3));
                }
                px[0] = cx ? ldg32(sp - 4) >> 8 : px[1]; // the aligned word in front of the patch ends with the pixel
            }
        }
        if (2 * ry < a.vh) { // luma of this row (the margin rows below the picture repeat its last row: after the loop)
            const uint8_t *sp = a.p0 + (size_t)(2 * ry + r) * a.s0;
            int yv[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const unsigned p = fast ? px[1 + i] : rgb_px<BPP>(sp, x0 + i < a.vw ? x0 + i : a.vw - 1);
                yv[i] = (a.yr * byte_of(p, RO) + a.yg * byte_of(p, GO) + a.yb * byte_of(p, BO) + yoff) >> 16;
            }
            yrow[r] = make_uint2(csc_pack4(yv[0], yv[1], yv[2], yv[3]), csc_pack4(yv[4], yv[5], yv[6], yv[7]));
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            unsigned l, m, n;
            if (fast) { l = px[2 * i]; m = px[2 * i + 1]; n = px[2 * i + 2]; }
            else {
                const uint8_t *sp = a.p0 + (size_t)(base + r) * a.s0;
                const int c2 = 2 * (cx * 4 + i < cw ? cx * 4 + i : cw - 1); // <= vw - 2: only the left tap can leave the picture
                l = rgb_px<BPP>(sp, c2 ? c2 - 1 : 0); m = rgb_px<BPP>(sp, c2); n = rgb_px<BPP>(sp, c2 + 1);
            }
            sr[i] += byte_of(l, RO) + 2 * byte_of(m, RO) + byte_of(n, RO);
            sg[i] += byte_of(l, GO) + 2 * byte_of(m, GO) + byte_of(n, GO);
            sb[i] += byte_of(l, BO) + 2 * byte_of(m, BO) + byte_of(n, BO);
        }
    }
    if (2 * ry >= a.vh) { // margin rows: the luma of the last visible row
        const uint8_t *sp = a.p0 + (size_t)(a.vh - 1) * a.s0;
        int yv[8];
        for (int i = 0; i < 8; i++) {
            const unsigned p = rgb_px<BPP>(sp, x0 + i < a.vw ? x0 + i : a.vw - 1);
            yv[i] = (a.yr * byte_of(p, RO) + a.yg * byte_of(p, GO) + a.yb * byte_of(p, BO) + yoff) >> 16;
        }
        yrow[0] = yrow[1] = make_uint2(csc_pack4(yv[0], yv[1], yv[2], yv[3]), csc_pack4(yv[4], yv[5], yv[6], yv[7]));
    }
    int cb[4], cr[4];
    const int coff = (128 << 19) + (1 << 18);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        cb[i] = (a.br * sr[i] + a.bg * sg[i] + a.bb * sb[i] + coff) >> 19;
        cr[i] = (a.rr * sr[i] + a.rg * sg[i] + a.rb * sb[i] + coff) >> 19;
    }
    const unsigned uvw[2] = {csc_pack4(cb[0], cr[0], cb[1], cr[1]), csc_pack4(cb[2], cr[2], cb[3], cr[3])};
    csc_store(a, ry, x0, yrow, uvw);
}

// fmt: MI355ENC_FMT_* of include/mi355enc.h (4 Y42B, 5 Y444, 7 NV21, 8 BGRX, 9 RGBX, 10 XRGB, 11 XBGR, 12 BGR, 13 RGB); coef: the ten words of
// mi355enc_csc_coefficients (RGB formats only).  -1: not a format of this file.
int k_launch_csc2(int fmt, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2, int s0, int s1, int s2, uint8_t *dy, uint8_t *duv,
                  int vw, int vh, int W, int H, const int *coef, hipStream_t s) {
    csc2_args a = {};
    a.p0 = p0; a.p1 = p1; a.p2 = p2; a.s0 = s0; a.s1 = s1; a.s2 = s2; a.dy = dy; a.duv = duv; a.vw = vw; a.vh = vh; a.W = W; a.H = H;
    if (fmt >= 8) {
        if (!coef) return -1;
        a.yr = coef[0]; a.yg = coef[1]; a.yb = coef[2]; a.br = coef[3]; a.bg = coef[4]; a.bb = coef[5]; a.rr = coef[6]; a.rg = coef[7]; a.rb = coef[8]; a.off = coef[9];
    }
    const dim3 g(((W >> 3) * (H >> 1) + 255) / 256), b(256);
    switch (fmt) {
    case 4: hipLaunchKernelGGL(csc_planar_kernel<4>, g, b, 0, s, a); break;
    case 5: hipLaunchKernelGGL(csc_planar_kernel<5>, g, b, 0, s, a); break;
    case 7: hipLaunchKernelGGL(csc_planar_kernel<7>, g, b, 0, s, a); break;
    case 8: hipLaunchKernelGGL((csc_rgb_kernel<4, 2, 1, 0>), g, b, 0, s, a); break;  // B G R x
    case 9: hipLaunchKernelGGL((csc_rgb_kernel<4, 0, 1, 2>), g, b, 0, s, a); break;  // R G B x
    case 10: hipLaunchKernelGGL((csc_rgb_kernel<4, 1, 2, 3>), g, b, 0, s, a); break; // x R G B
    case 11: hipLaunchKernelGGL((csc_rgb_kernel<4, 3, 2, 1>), g, b, 0, s, a); break; // x B G R
    case 12: hipLaunchKernelGGL((csc_rgb_kernel<3, 2, 1, 0>), g, b, 0, s, a); break; // B G R
    case 13: hipLaunchKernelGGL((csc_rgb_kernel<3, 0, 1, 2>), g, b, 0, s, a); break; // R G B
    default: return -1;
    }
    return 0;
}
