// k_snapshot.hip -- the device half of the JPEG stills (DESIGN.md section 18 states the rule): box reduction by 1, 2, 4 or 8, level shift, the 8x8 forward
// DCT (IJG's accurate integer one, jfdctint: CONST_BITS 13 / PASS1_BITS 2, rows first) and libjpeg's quantiser, from NV12 planes at any address and stride
// to dense int16 levels in the layout mi355enc_jpeg_entropy_decode returns -- what the host's Huffman writer (snapshot_host.c) codes.  The mirror image of
// k_jpeg.hip, with its shape.  Hand-written HIP for gfx950 (CDNA4, wave64); part of libmi355enc.
//
// One launch per still, one wave64 per task, eight lanes per block.  A luma task is eight horizontally adjacent blocks of one block row: lane 8 b + k loads
// (and reduces) row k of block b -- at reduction 1 the eight lanes of a row read one contiguous 64-byte line -- and runs the row pass in registers; LDS turns
// rows into columns (int16, the block stride of k_jpeg.hip: the column reads of eight blocks fall into different banks), lane 8 b + c runs the column pass of
// column c, quantises its eight coefficients and writes the levels back to LDS, from where lane 8 b + r takes row r: the wave's store is 1 KB in one piece.
// A chroma task is four Cb blocks (lanes 0 .. 31) and the Cr blocks of the same places (lanes 32 .. 63), each lane taking its component out of the NV12 pairs.
// The reduction runs on the way in, four samples an instruction (v_sad_u8 against zero).  A lane whose eight samples are not all inside the picture, and every
// lane of a plane whose address or stride is no multiple of four, goes byte by byte with clamped coordinates: no byte outside the visible picture is read.
// The division of the quantiser is a multiplication with ceil(2^32 / (8 q)) (the host's table: mi355enc_snapshot_reciprocal; exact for every numerator below 2^21).
// Ordinary vector stores only; the levels and the per-block hints may lie in pinned host memory.
#include "kernels_common.hpp"

struct snap_args {
    const uint8_t *sy, *suv; // NV12 source
    int ys, uvs;             // strides
    int w, h;                // visible size (even)
    int ow, oh, cow, coh;    // reduced luma / chroma size
    int al_y, al_uv;         // address and stride are multiples of four: dword loads
    const uint2 *tab;        // [2][64] {m, 4 q}, natural order (snapshot_tab_t)
    int16_t *levels;         // the blocks, 64 int16 each, natural order
    uint8_t *hint;           // per block: zigzag index of its last non-zero level
    unsigned first1, first2; // first block of Cb, Cr (luma: 0)
    int bw0, bwc;            // blocks per row of the MCU-padded luma / chroma plane
    int lgroups, ntask_l;    // luma tasks: groups of eight blocks per block row, and their number
    int cgroups, ntask;      // chroma tasks: groups of four blocks per block row; all tasks
};

#define SNAP_STRIDE 72 // int16 per block in LDS (144 bytes: rows stay 16-byte aligned, the column reads of eight blocks fall into different banks)

// k_zz_t[c * 8 + v]: the zigzag index of natural position v * 8 + c
static __device__ const uint8_t k_zz_t[64] = {0,  2,  3,  9,  10, 20, 21, 35, 1,  4,  8,  11, 19, 22, 34, 36, 5,  7,  12, 18, 23, 33, 37, 48, 6,  13, 17, 24, 32, 38, 47, 49,
                                              14, 16, 25, 31, 39, 46, 50, 57, 15, 26, 30, 40, 45, 51, 56, 58, 27, 29, 41, 44, 52, 55, 59, 62, 28, 42, 43, 53, 54, 60, 61, 63};

// Eight reduced samples: row Y, columns X0 .. X0 + 7 of the reduction (rw x rh) of a plane of pw x ph units.  UNIT 1: a unit is a byte; 2: a (Cb, Cr) pair, of
// which `half` says the byte.  Output coordinates are clamped to the reduced plane (the MCU padding repeats its last column and row), source coordinates to the plane.
template <int L, int UNIT> DEV void snap_load(const uint8_t *p, int stride, bool al, int pw, int ph, int rw, int rh, int X0, int Y, int half, int *v) {
    constexpr int S = 1 << L;
    const int y = Y < rh ? Y : rh - 1;
    unsigned acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = 0u;
    if (al && S * (X0 + 8) <= pw) { // all 8 S units of every row lie inside the plane: dwords
        constexpr int ND = UNIT * S * 2; // dwords per row
        constexpr int UJ = L >= 2 ? 1 : S;
#pragma unroll UJ
        for (int j = 0; j < S; j++) {
            const int row = S * y + j < ph ? S * y + j : ph - 1;
            const uint8_t *r = p + (size_t)row * stride + UNIT * S * X0;
#pragma unroll
            for (int d = 0; d < ND; d++) {
                unsigned wv = ldg32(r + 4 * d);
                if (UNIT == 2) wv = half ? (wv >> 8) & 0x00FF00FFu : wv & 0x00FF00FFu; // this lane's component of two pairs, in bytes 0 and 2
                if (UNIT == 1 && L == 0) {
                    acc[4 * d] = wv & 255u; acc[4 * d + 1] = (wv >> 8) & 255u; acc[4 * d + 2] = (wv >> 16) & 255u; acc[4 * d + 3] = wv >> 24;
                } else if ((UNIT == 1 && L == 1) || (UNIT == 2 && L == 0)) {
                    acc[2 * d] = __builtin_amdgcn_sad_u8(wv & 0xFFFFu, 0u, acc[2 * d]);
                    acc[2 * d + 1] = __builtin_amdgcn_sad_u8(wv >> 16, 0u, acc[2 * d + 1]);
                } else {
                    constexpr int PER = UNIT == 1 ? S / 4 : S / 2; // dwords per output sample
                    acc[d / PER] = __builtin_amdgcn_sad_u8(wv, 0u, acc[d / PER]);
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int x = X0 + i < rw ? X0 + i : rw - 1;
#pragma unroll 1
            for (int j = 0; j < S; j++) {
                const int row = S * y + j < ph ? S * y + j : ph - 1;
                const uint8_t *r = p + (size_t)row * stride + (UNIT == 2 ? half : 0);
#pragma unroll 1
                for (int ii = 0; ii < S; ii++) {
                    const int col = S * x + ii < pw ? S * x + ii : pw - 1;
                    acc[i] += ldg8(r + UNIT * col);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = (int)((acc[i] + (unsigned)((S * S) >> 1)) >> (2 * L));
}

// one 8-point pass of jfdctint: d in, o out; COL 0: the row pass (results scaled up by 2^PASS1_BITS), 1: the column pass (scaled down again; the result is 8 x the DCT)
DEV int snap_r(int x, int n) { return (x + (1 << (n - 1))) >> n; }
template <int COL> DEV void jfdct_1d(const int *d, int *o) {
    constexpr int N = COL ? 15 : 11;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    o[0] = COL ? snap_r(t10 + t11, 2) : (t10 + t11) * 4;
    o[4] = COL ? snap_r(t10 - t11, 2) : (t10 - t11) * 4;
    const int z = (t12 + t13) * 4433;
    o[2] = snap_r(z + t13 * 6270, N);
    o[6] = snap_r(z - t12 * 15137, N);
    const int z1 = t4 + t7, z2 = t5 + t6;
    int z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    z3 = z5 - z3 * 16069; z4 = z5 - z4 * 3196;
    o[7] = snap_r(t4 * 2446 - z1 * 7373 + z3, N);
    o[5] = snap_r(t5 * 16819 - z2 * 20995 + z4, N);
    o[3] = snap_r(t6 * 25172 - z2 * 20995 + z3, N);
    o[1] = snap_r(t7 * 12299 - z1 * 7373 + z4, N);
}
DEV unsigned snap_pack2(int a, int b) { return ((unsigned)a & 0xFFFFu) | ((unsigned)b << 16); }

// L: log2 of the reduction.  What a wave does depends on its task alone, so every branch on it is uniform.
template <int L>
__global__ __launch_bounds__(256) void snapshot_kernel(snap_args a) {
    __shared__ __attribute__((aligned(16))) int16_t s_rows[4][8 * SNAP_STRIDE];
    __shared__ __attribute__((aligned(16))) int16_t s_lev[4][8 * SNAP_STRIDE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, k = lane & 7, bsel = lane >> 3;
    int task = blockIdx.x * 4 + wave;
    const bool live = task < a.ntask; // (every wave reaches the barriers; one past the end works on task 0 and stores nothing)
    if (!live) task = 0;
    const bool chroma = task >= a.ntask_l;
    int brow, bx, bwp, v[8];
    unsigned first = 0;
    if (!chroma) {
        brow = task / a.lgroups;
        bx = (task - brow * a.lgroups) * 8 + bsel;
        bwp = a.bw0;
        snap_load<L, 1>(a.sy, a.ys, a.al_y != 0, a.w, a.h, a.ow, a.oh, bx * 8, brow * 8 + k, 0, v);
    } else {
        const int t = task - a.ntask_l, half = lane >> 5;
        brow = t / a.cgroups;
        bx = (t - brow * a.cgroups) * 4 + (bsel & 3);
        bwp = a.bwc;
        first = half ? a.first2 : a.first1;
        snap_load<L, 2>(a.suv, a.uvs, a.al_uv != 0, a.w >> 1, a.h >> 1, a.cow, a.coh, bx * 8, brow * 8 + k, half, v);
    }
    int d[8], o[8];
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = v[i] - 128;
    jfdct_1d<0>(d, o); // |o| <= 5683: fits 16 bits
    *(uint4 *)&s_rows[wave][bsel * SNAP_STRIDE + k * 8] = make_uint4(snap_pack2(o[0], o[1]), snap_pack2(o[2], o[3]), snap_pack2(o[4], o[5]), snap_pack2(o[6], o[7]));
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = s_rows[wave][bsel * SNAP_STRIDE + i * 8 + k];
    jfdct_1d<1>(d, o); // o[i]: the coefficient at natural position 8 i + k
    const uint2 *tab = a.tab + (chroma ? 64 : 0);
    unsigned last = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint2 e = ldg64(tab + i * 8 + k);
        const unsigned n = (unsigned)(o[i] < 0 ? -o[i] : o[i]) + e.y; // |c| + 4 q
        const int l = (int)__umulhi(n, e.x);                          // / (8 q)
        const unsigned zz = k_zz_t[k * 8 + i];
        if (l && zz > last) last = zz;
        s_lev[wave][bsel * SNAP_STRIDE + i * 8 + k] = (int16_t)(o[i] < 0 ? -l : l);
    }
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) { const unsigned t = (unsigned)__shfl_xor((int)last, m, 64); last = t > last ? t : last; } // over the block's eight lanes
    __syncthreads();
    const uint4 r = *(const uint4 *)&s_lev[wave][bsel * SNAP_STRIDE + k * 8];
    if (live && bx < bwp) {
        const size_t blk = (size_t)first + (size_t)brow * bwp + bx;
        stg128(a.levels + blk * 64 + k * 8, r);
        if (k == 0) stg8(a.hint + blk, last);
    }
}

// NV12 planes of w x h (even, at least 2) at any address and stride, reduced by 2^log2s, as the levels of a 4:2:0 still of ceil(w / s) x ceil(h / s): levels
// (64 int16 per block) and hint (one byte per block) for the blocks of jpeg_host_layout's layout, device or pinned host memory, levels 16-byte aligned; d_tab: the
// snapshot_tab_t of the quality, on the device.  -1: sizes or a reduction it does not take.
int k_launch_snapshot(const uint8_t *sy, int ys, const uint8_t *suv, int uvs, int w, int h, int log2s, const void *d_tab, int16_t *levels, uint8_t *hint, hipStream_t s) {
    if (w < 2 || h < 2 || ((w | h) & 1) || w > 16384 || h > 16384 || log2s < 0 || log2s > 3 || ys < w || uvs < w) return -1;
    const int S = 1 << log2s;
    snap_args a = {};
    a.sy = sy; a.suv = suv; a.ys = ys; a.uvs = uvs; a.w = w; a.h = h;
    a.ow = (w + S - 1) / S; a.oh = (h + S - 1) / S; a.cow = (a.ow + 1) / 2; a.coh = (a.oh + 1) / 2;
    a.al_y = (((uintptr_t)sy | (uintptr_t)ys) & 3) == 0;
    a.al_uv = (((uintptr_t)suv | (uintptr_t)uvs) & 3) == 0;
    a.tab = (const uint2 *)d_tab; a.levels = levels; a.hint = hint;
    const int mcux = (a.ow + 15) / 16, mcuy = (a.oh + 15) / 16;
    a.bw0 = 2 * mcux; a.bwc = mcux;
    a.first1 = (unsigned)(2 * mcux) * (unsigned)(2 * mcuy); a.first2 = a.first1 + (unsigned)mcux * (unsigned)mcuy;
    a.lgroups = (a.bw0 + 7) / 8; a.ntask_l = 2 * mcuy * a.lgroups;
    a.cgroups = (mcux + 3) / 4; a.ntask = a.ntask_l + mcuy * a.cgroups;
    const dim3 grid((unsigned)((a.ntask + 3) / 4));
    if (log2s == 0) hipLaunchKernelGGL(snapshot_kernel<0>, grid, dim3(256), 0, s, a);
    else if (log2s == 1) hipLaunchKernelGGL(snapshot_kernel<1>, grid, dim3(256), 0, s, a);
    else if (log2s == 2) hipLaunchKernelGGL(snapshot_kernel<2>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(snapshot_kernel<3>, grid, dim3(256), 0, s, a);
    return 0;
}
