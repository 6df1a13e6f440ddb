// k_orient.hip -- orientation of the input picture: the eight methods of GstVideoOrientationMethod as a pure permutation of
// samples, NV12 of the pre-orientation visible size -> the coded NV12 surfaces of stride W, margin included.  One launch per picture, both planes.
//
// A method is a transpose (or none) followed by mirrors.  With (x, y) the output sample, (u, v) = transposing ? (y, x) : (x, y),
//   sx = mirror_x ? in_w - 1 - u : u,   sy = mirror_y ? in_h - 1 - v : v        (mi355enc_orient_source states the same rule on the host)
//   method    1 90r   2 180   3 90l   4 horiz   5 vert   6 ul-lr   7 ur-ll
//   transpose   x               x                          x         x
//   mirror_x            x       x       x                            x
//   mirror_y    x       x                        x                   x
// Luma moves as bytes, chroma as 16-bit (Cb, Cr) units through the same code (ES = 1 / 2): a pair is never split.
//
// Transposing methods (orient_t_kernel): a workgroup takes 128 source bytes (128 luma samples / 64 pairs: output ROWS) x 128 output elements along x
// (source ROWS) through a 16 KB LDS tile.  Rows and mirrors cost nothing: the tile's LDS row r holds the source row of output column ox0 + r, whichever
// way the method runs through the source rows, and a mirrored source column only changes the output ROW a word is stored to -- so both global sides are
// row-contiguous, aligned and in memory order: 16-byte loads (a source row's 128 bytes by eight lanes), 8-byte (luma) / 16-byte (chroma) stores, a full
// 128 / 256 bytes of an output row per store instruction and row.
// LDS layout: row r = 32 dwords at r * 32, dword c of it at c ^ (((r >> 3) & 7) << 2).  The swizzle moves whole 16-byte slots, so the row-wise
// ds_write_b128 stay aligned: eight lanes write the eight slots of one row, 32 distinct banks, no conflict.  A lane of the column-wise pass reads dword c
// of the eight rows 8 g .. 8 g + 7 (eight ds_read_b32; banks are (a / 4) mod 32, conflicts counted per 32-lane half).  A half holds g = 0 .. 7 (or 8 .. 15)
// x c = c0 .. c0 + 3, c0 a multiple of 4: bank = (c0 ^ 4 (g & 7)) + (c & 3) -- eight distinct multiples of four plus 0 .. 3: 32 distinct banks, 0 conflicts
// (unswizzled: every g on the same four banks, 8-way).  The 8 x 4 bytes (4 x 2 pairs) a lane holds are transposed in registers by v_perm_b32.
//
// Non-transposing methods (orient_f_kernel): no LDS.  A lane takes 16 output bytes of one row: with mirror_x the source word at the mirrored
// position, its dwords in reverse order and each dword's bytes (chroma: 16-bit halves) reversed by one v_perm_b32.
//
// Guarded byte path, both kernels: a source word is loaded whole only where the plane's address and stride allow it and all of it is visible (the
// caller's planes of mi355enc_submit_device lie at any address and stride, and nothing behind a row's visible width is ever read); everything else is
// assembled byte by byte.  A destination that is not 16-byte aligned is stored byte by byte.
// Margin up to W x H (pad_kernel's rule: the last visible column / row, chroma the last pair): the columns from the clamped LDS row / the clamped source
// element of the words that reach behind the visible width, the rows by the owners of the last visible row, who store their words again -- filled
// from registers, never read back.  No wait, no atomic.
#include "kernels_common.hpp"

#define OT_ROWS 128                  /* LDS rows of a tile: output elements along x */
#define OT_DW 32                     /* dwords per LDS row: 128 source bytes */
#define SEL_REV8 0x00010203u         /* v_perm_b32: the four bytes of the low operand reversed */
#define SEL_REV16 0x01000302u        /* ... its two 16-bit halves exchanged (pair-preserving) */
#define SEL_ZIP_LO 0x05010400u       /* {lo.0, hi.0, lo.1, hi.1} */
#define SEL_ZIP_HI 0x07030602u       /* {lo.2, hi.2, lo.3, hi.3} */
#define SEL_H_LO 0x05040100u         /* {lo.0, lo.1, hi.0, hi.1} */
#define SEL_H_HI 0x07060302u         /* {lo.2, lo.3, hi.2, hi.3} */

struct orient_args {
    const uint8_t *sy, *suv; // source NV12 of the pre-orientation visible size in_w x in_h
    int ssy, ssuv;           // ... and its strides
    uint8_t *dy, *duv;       // destination surfaces: coded size W x H, stride W
    int in_w, in_h, W, H;
    int fx, fy;              // mirror_x, mirror_y
    int ntx_l, tiles_l;      // transposing: source-x tiles of the luma plane, all luma tiles; non-transposing: luma lanes in tiles_l
    int ntx_c;
};

// one plane as the element-size template sees it (sizes in elements)
struct orient_plane {
    const uint8_t *src; uint8_t *dst;
    int ss, iw, ih, Wd, Hd;
    bool sal, dal; // source address and stride / destination address are multiples of 16
};
template <int ES> DEV orient_plane plane_of(const orient_args &a) {
    orient_plane p;
    p.src = ES == 1 ? a.sy : a.suv; p.dst = ES == 1 ? a.dy : a.duv; p.ss = ES == 1 ? a.ssy : a.ssuv;
    p.iw = a.in_w / ES; p.ih = a.in_h / ES; p.Wd = a.W / ES; p.Hd = a.H / ES;
    p.sal = ((((uintptr_t)p.src) | (uintptr_t)(unsigned)p.ss) & 15) == 0;
    p.dal = (((uintptr_t)p.dst) & 15) == 0; // (the stride W is a multiple of 16)
    return p;
}
// N dwords (2 or 4) to dst: one aligned word, or byte by byte
template <int N> DEV void st_words(uint8_t *dst, const unsigned *w, bool al) {
    if (al) {
        if (N == 2) stg64(dst, make_uint2(w[0], w[1])); else stg128(dst, make_uint4(w[0], w[1], w[2], w[3]));
    } else
#pragma unroll
        for (int i = 0; i < 4 * N; i++) stg8(dst + i, (w[i >> 2] >> (8 * (i & 3))) & 255u);
}

// ------------------------------------------------------------------ transposing methods
DEV int ot_pos(int r, int c) { return r * OT_DW + (c ^ (((r >> 3) & 7) << 2)); }

template <int ES> DEV void orient_t_tile(const orient_args &a, unsigned *lds, int tile, int ntx) {
    const orient_plane p = plane_of<ES>(a);
    const int TW = 128 / ES;
    const int t = threadIdx.x, bx = tile % ntx, by = tile / ntx;
    const int sx0 = bx * TW, ox0 = by * OT_ROWS;
    const int vw = p.ih, vh = p.iw; // the oriented visible size
    // row-wise: LDS row r <- the source row of output column ox0 + r
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int idx = t + 256 * i, r = idx >> 3, ch = idx & 7, ox = ox0 + r;
        if (ox >= vw) continue; // (margin columns read the clamped row)
        const int sy = a.fy ? p.ih - 1 - ox : ox, e0 = sx0 + ch * (16 / ES);
        const uint8_t *row = p.src + (size_t)sy * p.ss;
        uint4 v;
        if (p.sal && e0 + 16 / ES <= p.iw) v = ldg128(row + (size_t)e0 * ES);
        else {
            unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int b = 0; b < 16; b++)
                if (e0 + b / ES < p.iw) w[b >> 2] |= ldg8(row + (size_t)e0 * ES + b) << (8 * (b & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *(uint4 *)&lds[ot_pos(r, 4 * ch)] = v;
    }
    __syncthreads();
    // column-wise: dword c of rows 8 g .. 8 g + 7 -> 4 output rows of 8 bytes (luma) / 2 output rows of 8 pairs (chroma)
    const int rmax = vw - 1 - ox0; // the tile's last visible row, >= 0: W - vw <= 15 and ox0 is a multiple of 128 below W, so no tile lies wholly in the margin
    const int sxe = a.fx ? 0 : p.iw - 1; // the source column of the last visible output row
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int T = t + 256 * i, g = (T & 7) | ((T >> 2) & 8), c = ((T >> 3) & 3) | ((T >> 6) << 2);
        const int oxw = ox0 + 8 * g;
        if (oxw >= p.Wd) continue; // (Wd is a multiple of 8: a word is all inside or all outside)
        unsigned d[8];
#pragma unroll
        for (int k = 0; k < 8; k++) { const int r = 8 * g + k < rmax ? 8 * g + k : rmax; d[k] = lds[ot_pos(r, c)]; }
#pragma unroll
        for (int b = 0; b < 4 / ES; b++) {
            const int sx = sx0 + (4 / ES) * c + b;
            if (sx >= p.iw) continue;
            unsigned o[4];
            if (ES == 1) {
                const unsigned z0 = __builtin_amdgcn_perm(d[1], d[0], b < 2 ? SEL_ZIP_LO : SEL_ZIP_HI), z1 = __builtin_amdgcn_perm(d[3], d[2], b < 2 ? SEL_ZIP_LO : SEL_ZIP_HI);
                const unsigned z2 = __builtin_amdgcn_perm(d[5], d[4], b < 2 ? SEL_ZIP_LO : SEL_ZIP_HI), z3 = __builtin_amdgcn_perm(d[7], d[6], b < 2 ? SEL_ZIP_LO : SEL_ZIP_HI);
                o[0] = __builtin_amdgcn_perm(z1, z0, (b & 1) ? SEL_H_HI : SEL_H_LO);
                o[1] = __builtin_amdgcn_perm(z3, z2, (b & 1) ? SEL_H_HI : SEL_H_LO);
            } else {
#pragma unroll
                for (int m = 0; m < 4; m++) o[m] = __builtin_amdgcn_perm(d[2 * m + 1], d[2 * m], b ? SEL_H_HI : SEL_H_LO);
            }
            const int oy = a.fx ? p.iw - 1 - sx : sx;
            uint8_t *dst = p.dst + (size_t)oy * a.W + (size_t)oxw * ES;
            st_words<2 * ES>(dst, o, p.dal);
            if (sx == sxe)
                for (int m = vh; m < p.Hd; m++) st_words<2 * ES>(p.dst + (size_t)m * a.W + (size_t)oxw * ES, o, p.dal);
        }
    }
}
__global__ __launch_bounds__(256) void orient_t_kernel(const orient_args a) {
    __shared__ __attribute__((aligned(16))) unsigned lds[OT_ROWS * OT_DW];
    const int tile = blockIdx.x; // (uniform: a workgroup belongs to one plane)
    if (tile < a.tiles_l) orient_t_tile<1>(a, lds, tile, a.ntx_l);
    else orient_t_tile<2>(a, lds, tile - a.tiles_l, a.ntx_c);
}

// ------------------------------------------------------------------ non-transposing methods
template <int ES> DEV void orient_f_word(const orient_args &a, int i) {
    const orient_plane p = plane_of<ES>(a);
    const int per_row = a.W >> 4, oy = i / per_row, xb = (i - oy * per_row) * 16; // output row (visible), first output byte
    const int sy = a.fy ? p.ih - 1 - oy : oy, rowbytes = p.iw * ES;
    const uint8_t *row = p.src + (size_t)sy * p.ss;
    unsigned w[4] = {0, 0, 0, 0};
    if (xb + 16 <= rowbytes) { // all visible: the word at the (mirrored) position
        const uint8_t *sp = row + (a.fx ? rowbytes - 16 - xb : xb);
        if ((((uintptr_t)sp) & 15) == 0) { const uint4 v = ldg128(sp); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
        else if ((((uintptr_t)sp) & 7) == 0) { const uint2 v0 = ldg64(sp), v1 = ldg64(sp + 8); w[0] = v0.x; w[1] = v0.y; w[2] = v1.x; w[3] = v1.y; }
        else
#pragma unroll
            for (int b = 0; b < 16; b++) w[b >> 2] |= ldg8(sp + b) << (8 * (b & 3));
        if (a.fx) { // reversed word order, and the bytes (pairs) inside each dword
            const unsigned sel = ES == 1 ? SEL_REV8 : SEL_REV16;
            const unsigned r0 = __builtin_amdgcn_perm(0u, w[3], sel), r1 = __builtin_amdgcn_perm(0u, w[2], sel);
            const unsigned r2 = __builtin_amdgcn_perm(0u, w[1], sel), r3 = __builtin_amdgcn_perm(0u, w[0], sel);
            w[0] = r0; w[1] = r1; w[2] = r2; w[3] = r3;
        }
    } else // the word reaches behind the visible width: element by element, the margin repeats the last visible one
#pragma unroll
        for (int b = 0; b < 16; b++) {
            const int e = (xb + b) / ES, ec = e < p.iw ? e : p.iw - 1, sx = a.fx ? p.iw - 1 - ec : ec;
            w[b >> 2] |= ldg8(row + (size_t)sx * ES + (b & (ES - 1))) << (8 * (b & 3));
        }
    st_words<4>(p.dst + (size_t)oy * a.W + xb, w, p.dal);
    if (oy == p.ih - 1)
        for (int m = p.ih; m < p.Hd; m++) st_words<4>(p.dst + (size_t)m * a.W + xb, w, p.dal);
}
__global__ __launch_bounds__(256) void orient_f_kernel(const orient_args a) {
    const int i = blockIdx.x * 256 + threadIdx.x, nc = (a.W >> 4) * (a.in_h >> 1);
    if (i < a.tiles_l) orient_f_word<1>(a, i);
    else if (i < a.tiles_l + nc) orient_f_word<2>(a, i - a.tiles_l);
}

// in_w x in_h (even): the pre-orientation visible size; W x H: the coded size of the oriented picture.  -1: not a method / the sizes do not fit
int k_launch_orient(int method, const uint8_t *sy, int ssy, const uint8_t *suv, int ssuv, int in_w, int in_h, uint8_t *dy, uint8_t *duv, int W, int H, hipStream_t s) {
    if (method < 1 || method > 7 || in_w < 2 || in_h < 2 || ((in_w | in_h) & 1) || ((W | H) & 15) || ssy < in_w || ssuv < in_w) return -1;
    const bool tr = method == 1 || method == 3 || method == 6 || method == 7;
    const int ow = tr ? in_h : in_w, oh = tr ? in_w : in_h;
    if (ow > W || oh > H || W - ow > 15 || H - oh > 15) return -1;
    orient_args a;
    a.sy = sy; a.suv = suv; a.ssy = ssy; a.ssuv = ssuv; a.dy = dy; a.duv = duv; a.in_w = in_w; a.in_h = in_h; a.W = W; a.H = H;
    a.fx = method == 2 || method == 3 || method == 4 || method == 7;
    a.fy = method == 1 || method == 2 || method == 5 || method == 7;
    if (tr) {
        a.ntx_l = (in_w + 127) / 128; a.ntx_c = (in_w / 2 + 63) / 64;
        a.tiles_l = a.ntx_l * ((W + OT_ROWS - 1) / OT_ROWS);
        const int tiles_c = a.ntx_c * ((W / 2 + OT_ROWS - 1) / OT_ROWS);
        hipLaunchKernelGGL(orient_t_kernel, dim3((unsigned)(a.tiles_l + tiles_c)), dim3(256), 0, s, a);
    } else {
        a.ntx_l = a.ntx_c = 0;
        a.tiles_l = (W >> 4) * in_h;
        const int n = a.tiles_l + (W >> 4) * (in_h >> 1);
        hipLaunchKernelGGL(orient_f_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    }
    return 0;
}
