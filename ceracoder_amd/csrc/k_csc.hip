// k_csc.hip -- input conversion to NV12 for the formats csc_kernel (k_handover.hip) does not take: planar 4:2:2 / 4:4:4 (Y42B, Y444), NV21, and
// RGB in six byte orders (DESIGN.md section 11 states the rule).  Hand-written HIP for gfx950 (CDNA4, wave64); part of libmi355enc.
// Shape of csc_kernel: one thread converts an 8 x 2 luma patch and its 4 chroma pairs; on the fast path every global access is an aligned
// 4-, 8- or 16-byte word and a patch row is contiguous; the picture's edge, and planes whose address or stride is not suitably aligned,
// go byte by byte with clamped source coordinates (which also fills the coded-size margin).  Copy-shaped: 4 P or 3 P in, 1.5 P out.
// Also here: the 10-bit formats and GRAY8 (csc_deep_kernel), and the colour step on the coded NV12 surfaces (yuv_convert_kernel).
#include "kernels_common.hpp"

struct csc2_args {
    const uint8_t *p0, *p1, *p2; // planar: Y, U, V (NV21: Y, VU); RGB: p0 only
    int s0, s1, s2;              // their strides in bytes
    uint8_t *dy, *duv;           // NV12 destination, coded size W x H, stride W
    int vw, vh, W, H;            // visible and coded size
    int yr, yg, yb, br, bg, bb, rr, rg, rb, off; // RGB: the matrix in 2^-16 units and the luma offset (mi355enc_csc_coefficients)
};

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

// =================================================================== 10-bit formats and GRAY8
// 14 P010: 16-bit words, the sample in the upper ten bits; planes Y and (Cb, Cr) pairs.  15 I420_10: 16-bit words, the sample in the lower ten bits; planes Y, U, V.
// 16 v210: groups of six pixels in four 32-bit words of three 10-bit fields, 4:2:2.  17 GRAY8: luma bytes, every chroma byte 128.
// 10 -> 8 bits: min(255, (v + 2) >> 2); 4:2:2 chroma from the sum S of its two rows: min(255, (S + 4) >> 3).
// One thread makes a PW x 2 luma patch and its PW / 2 chroma pairs.  PW is 8, v210's is 24: four groups (64 bytes, four 16-byte loads) are the fewest whose luma
// fills whole 8-byte words, so every store of the fast path stays an aligned 8-byte one; the coded width is a multiple of 16, not of 24, so the last patch of a
// row may keep only its first one or two 8-sample pieces.  Margin rows read the picture's last rows on the same path.  A patch that reaches past the visible
// width, and planes that are not 16-byte (I420_10's chroma: 8-byte) aligned, go sample by sample with clamped source coordinates and byte loads.
DEV int deep8(int v10) { const int v = (v10 + 2) >> 2; return v > 255 ? 255 : v; }
// luma sample (sx, sy) as the byte it becomes
template <int FMT> DEV int deep_luma(const csc2_args &a, int sx, int sy) {
    const uint8_t *row = a.p0 + (size_t)sy * a.s0;
    if (FMT == 14) return deep8(deep_word(row + 2 * sx) >> 6);
    if (FMT == 15) return deep8(deep_word(row + 2 * sx) & 1023);
    if (FMT == 16) { const int g = sx / 6, k = sx - 6 * g; return deep8((int)v210_field(row, 4 * g + v210_yw(k), v210_ys(k))); }
    return (int)ldg8(row + sx);
}
// chroma sample c (comp 0 Cb, 1 Cr) of the chroma row made from luma rows base, base + 1
template <int FMT> DEV int deep_chroma(const csc2_args &a, int c, int base, int comp) {
    if (FMT == 14) return deep8(deep_word(a.p1 + (size_t)(base >> 1) * a.s1 + 4 * c + 2 * comp) >> 6);
    if (FMT == 15) return deep8(deep_word((comp ? a.p2 + (size_t)(base >> 1) * a.s2 : a.p1 + (size_t)(base >> 1) * a.s1) + 2 * c) & 1023);
    if (FMT == 16) {
        const int g = c / 3, k = 2 * (c - 3 * g) + comp;
        const int s = (int)v210_field(a.p0 + (size_t)base * a.s0, 4 * g + v210_cw(k), v210_cs(k)) + (int)v210_field(a.p0 + (size_t)(base + 1) * a.s0, 4 * g + v210_cw(k), v210_cs(k));
        const int v = (s + 4) >> 3;
        return v > 255 ? 255 : v;
    }
    return 128;
}
template <int FMT>
__global__ __launch_bounds__(256) void csc_deep_kernel(csc2_args a) {
    constexpr int PW = FMT == 16 ? 24 : 8;
    const int tx = blockIdx.x * 256 + threadIdx.x, per_row = (a.W + PW - 1) / PW, rows2 = a.H >> 1;
    if (tx >= per_row * rows2) return;
    const int ry = tx / per_row, cx = tx - ry * per_row, x0 = cx * PW;
    // margin rows below the picture: the last luma row, the last chroma row (of the last two source rows)
    const bool margin = 2 * ry >= a.vh;
    const int base = margin ? a.vh - 2 : 2 * ry, sy[2] = {margin ? a.vh - 1 : 2 * ry, margin ? a.vh - 1 : 2 * ry + 1};
    const bool vis = x0 + PW <= a.vw; // visible width is even: a patch is fully visible, or clamped per sample
    bool fast = vis && (a.s0 & 15) == 0 && (((uintptr_t)a.p0) & 15) == 0;
    if (FMT == 14) fast = fast && (a.s1 & 15) == 0 && (((uintptr_t)a.p1) & 15) == 0;
    if (FMT == 15) fast = fast && ((a.s1 | a.s2) & 7) == 0 && ((((uintptr_t)a.p1) | ((uintptr_t)a.p2)) & 7) == 0;
    if (FMT == 17) fast = vis && (a.s0 & 7) == 0 && (((uintptr_t)a.p0) & 7) == 0;
    if (!fast) { // sample by sample, in pieces of 8 luma columns: the loads of a piece do not wait for each other, and the stores stay the 8-byte ones
        const int cw = a.vw >> 1;
        for (int j = 0; j < PW / 8 && x0 + 8 * j < a.W; j++) {
            const int xp = x0 + 8 * j;
            uint2 yrow[2];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                int v[8];
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = deep_luma<FMT>(a, xp + i < a.vw ? xp + i : a.vw - 1, sy[r]);
                yrow[r] = make_uint2(pack4(v[0], v[1], v[2], v[3]), pack4(v[4], v[5], v[6], v[7])); // (every value is a byte already)
            }
            int c[8];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int cc = (xp >> 1) + i < cw ? (xp >> 1) + i : cw - 1;
                c[2 * i] = deep_chroma<FMT>(a, cc, base, 0);
                c[2 * i + 1] = deep_chroma<FMT>(a, cc, base, 1);
            }
            const unsigned uvw[2] = {pack4(c[0], c[1], c[2], c[3]), pack4(c[4], c[5], c[6], c[7])};
            csc_store(a, ry, xp, yrow, uvw);
        }
        return;
    }
    if (FMT == 16) {
        int cs[24]; // the row-pair sums: Cb, Cr of pair i at [2 i], [2 i + 1]
        uint2 yw[2][3]; // luma of source rows base, base + 1
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint8_t *sp = a.p0 + (size_t)(base + r) * a.s0 + (size_t)cx * 64;
            int yv[24];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const uint4 q = ldg128(sp + 16 * g);
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    yv[6 * g + k] = (v210_get(q, v210_yw(k), v210_ys(k)) + 2) >> 2;
                    const int c = v210_get(q, v210_cw(k), v210_cs(k));
                    cs[6 * g + k] = r ? cs[6 * g + k] + c : c;
                }
            }
#pragma unroll
            for (int j = 0; j < 3; j++) yw[r][j] = make_uint2(csc_pack4(yv[8 * j], yv[8 * j + 1], yv[8 * j + 2], yv[8 * j + 3]), csc_pack4(yv[8 * j + 4], yv[8 * j + 5], yv[8 * j + 6], yv[8 * j + 7]));
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            stg64(a.dy + (size_t)(2 * ry) * a.W + x0 + 8 * j, margin ? yw[1][j] : yw[0][j]); // (margin rows: both are the picture's last row)
            stg64(a.dy + (size_t)(2 * ry + 1) * a.W + x0 + 8 * j, yw[1][j]);
            stg64(a.duv + (size_t)ry * a.W + x0 + 8 * j, make_uint2(csc_pack4((cs[8 * j] + 4) >> 3, (cs[8 * j + 1] + 4) >> 3, (cs[8 * j + 2] + 4) >> 3, (cs[8 * j + 3] + 4) >> 3),
                                                                   csc_pack4((cs[8 * j + 4] + 4) >> 3, (cs[8 * j + 5] + 4) >> 3, (cs[8 * j + 6] + 4) >> 3, (cs[8 * j + 7] + 4) >> 3)));
        }
        return;
    }
    uint2 yrow[2];
    unsigned uvw[2];
    if (FMT == 17) {
        yrow[0] = ldg64(a.p0 + (size_t)sy[0] * a.s0 + x0);
        yrow[1] = ldg64(a.p0 + (size_t)sy[1] * a.s0 + x0);
        uvw[0] = uvw[1] = 0x80808080u;
    } else {
        constexpr int SH = FMT == 14 ? 6 : 0; // (v >> 6, or v & 1023: one shift and one mask serve both)
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint4 q = ldg128(a.p0 + (size_t)sy[r] * a.s0 + 2 * x0);
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
            int v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = (int)((((w[i >> 1] >> (16 * (i & 1))) & 0xffffu) >> SH & 1023u) + 2) >> 2;
            yrow[r] = make_uint2(csc_pack4(v[0], v[1], v[2], v[3]), csc_pack4(v[4], v[5], v[6], v[7]));
        }
        int c[8]; // Cb0 Cr0 Cb1 Cr1 ...
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
        uvw[0] = csc_pack4((c[0] + 2) >> 2, (c[1] + 2) >> 2, (c[2] + 2) >> 2, (c[3] + 2) >> 2);
        uvw[1] = csc_pack4((c[4] + 2) >> 2, (c[5] + 2) >> 2, (c[6] + 2) >> 2, (c[7] + 2) >> 2);
    }
    csc_store(a, ry, x0, yrow, uvw);
}

// =================================================================== the colour step
// YUV of one (range, matrix) -> YUV of another, in place on NV12 surfaces of the coded size.  Pointwise: a luma sample uses the chroma pair of its own 2 x 2 block.
// One thread owns an 8 x 2 luma patch and its four chroma pairs: all three words are read before the first is written, and no other thread touches them, which
// is what makes in place safe.  [x0, x1) x [y0, y1) (even) is the part of the surfaces that is picture; everything else is border and keeps its bytes: a patch
// outside it is left alone, one that straddles its left or right edge merges converted and original bytes per column pair.
struct yuv_args {
    uint8_t *y, *uv;
    int W, H, x0, x1, y0, y1;
    int cyy, cyb, cyr, cbb, cbr, crb, crr, oy, oy2;
};
__global__ __launch_bounds__(256) void yuv_convert_kernel(yuv_args a) {
    const int tx = blockIdx.x * 256 + threadIdx.x, per_row = a.W >> 3, rows2 = a.H >> 1;
    if (tx >= per_row * rows2) return;
    const int ry = tx / per_row, cx = tx - ry * per_row, x0 = cx * 8;
    if (2 * ry < a.y0 || 2 * ry >= a.y1 || x0 + 8 <= a.x0 || x0 >= a.x1) return;
    uint8_t *py = a.y + (size_t)(2 * ry) * a.W + x0, *puv = a.uv + (size_t)ry * a.W + x0;
    const uint2 s0 = ldg64(py), s1 = ldg64(py + a.W), sc = ldg64(puv);
    const unsigned yw[2][2] = {{s0.x, s0.y}, {s1.x, s1.y}}, cw[2] = {sc.x, sc.y};
    int t[4], nb[4], nr[4];
    const int yoff = (a.oy2 << 16) + (1 << 15), coff = (128 << 16) + (1 << 15);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int cb = byte_of(cw[i >> 1], 2 * (i & 1)) - 128, cr = byte_of(cw[i >> 1], 2 * (i & 1) + 1) - 128;
        t[i] = a.cyb * cb + a.cyr * cr + yoff;
        nb[i] = (a.cbb * cb + a.cbr * cr + coff) >> 16;
        nr[i] = (a.crb * cb + a.crr * cr + coff) >> 16;
    }
    uint2 oy[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        int v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = (a.cyy * (byte_of(yw[r][i >> 2], i & 3) - a.oy) + t[i >> 1]) >> 16;
        oy[r] = make_uint2(csc_pack4(v[0], v[1], v[2], v[3]), csc_pack4(v[4], v[5], v[6], v[7]));
    }
    uint2 ouv = make_uint2(csc_pack4(nb[0], nr[0], nb[1], nr[1]), csc_pack4(nb[2], nr[2], nb[3], nr[3]));
    if (x0 < a.x0 || x0 + 8 > a.x1) { // straddles an edge of the picture rectangle: per column pair, converted inside, the original bytes outside
        unsigned m[2];
#pragma unroll
        for (int k = 0; k < 2; k++) m[k] = (x0 + 4 * k >= a.x0 && x0 + 4 * k < a.x1 ? 0x0000ffffu : 0u) | (x0 + 4 * k + 2 >= a.x0 && x0 + 4 * k + 2 < a.x1 ? 0xffff0000u : 0u);
        oy[0] = make_uint2((oy[0].x & m[0]) | (s0.x & ~m[0]), (oy[0].y & m[1]) | (s0.y & ~m[1]));
        oy[1] = make_uint2((oy[1].x & m[0]) | (s1.x & ~m[0]), (oy[1].y & m[1]) | (s1.y & ~m[1]));
        ouv = make_uint2((ouv.x & m[0]) | (sc.x & ~m[0]), (ouv.y & m[1]) | (sc.y & ~m[1]));
    }
    stg64(py, oy[0]);
    stg64(py + a.W, oy[1]);
    stg64(puv, ouv);
}
// y, uv: NV12 surfaces of W x H (multiples of 16 / 2) at stride W, 8-byte aligned; rect: x0, x1, y0, y1 (even, inside the surfaces); coef: the nine words of
// mi355enc_yuv_coefficients.  -1: arguments outside that.
int k_launch_yuv_convert(uint8_t *y, uint8_t *uv, int W, int H, const int rect[4], const int *coef, hipStream_t s) {
    if (!y || !uv || !rect || !coef || W <= 0 || H <= 0 || (W & 7) || (H & 1) || ((((uintptr_t)y) | ((uintptr_t)uv)) & 7)) return -1;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return -1;
    yuv_args a;
    a.y = y; a.uv = uv; a.W = W; a.H = H; a.x0 = rect[0]; a.x1 = rect[1]; a.y0 = rect[2]; a.y1 = rect[3];
    a.cyy = coef[0]; a.cyb = coef[1]; a.cyr = coef[2]; a.cbb = coef[3]; a.cbr = coef[4]; a.crb = coef[5]; a.crr = coef[6]; a.oy = coef[7]; a.oy2 = coef[8];
    hipLaunchKernelGGL(yuv_convert_kernel, dim3(((W >> 3) * (H >> 1) + 255) / 256), dim3(256), 0, s, a);
    return 0;
}

// fmt: MI355ENC_FMT_* of include/mi355enc.h (4 Y42B, 5 Y444, 7 NV21, 8 BGRX, 9 RGBX, 10 XRGB, 11 XBGR, 12 BGR, 13 RGB, 14 P010, 15 I420_10, 16 V210, 17 GRAY8); coef: the ten words of
// mi355enc_csc_coefficients (RGB formats only).  -1: not a format of this file.
int k_launch_csc2(int fmt, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2, int s0, int s1, int s2, uint8_t *dy, uint8_t *duv,
                  int vw, int vh, int W, int H, const int *coef, hipStream_t s) {
    csc2_args a = {};
    a.p0 = p0; a.p1 = p1; a.p2 = p2; a.s0 = s0; a.s1 = s1; a.s2 = s2; a.dy = dy; a.duv = duv; a.vw = vw; a.vh = vh; a.W = W; a.H = H;
    if (fmt >= 8 && fmt <= 13) {
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
    case 14: hipLaunchKernelGGL(csc_deep_kernel<14>, g, b, 0, s, a); break;
    case 15: hipLaunchKernelGGL(csc_deep_kernel<15>, g, b, 0, s, a); break;
    case 16: hipLaunchKernelGGL(csc_deep_kernel<16>, dim3((((W + 23) / 24) * (H >> 1) + 255) / 256), b, 0, s, a); break; // 24 x 2 patches
    case 17: hipLaunchKernelGGL(csc_deep_kernel<17>, g, b, 0, s, a); break;
    default: return -1;
    }
    return 0;
}
