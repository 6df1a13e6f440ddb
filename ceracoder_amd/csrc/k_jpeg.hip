// k_jpeg.hip -- the device half of MJPEG input (DESIGN.md section 14 states the rule): dequantisation, the 8x8 inverse DCT (IJG's accurate
// integer one, CONST_BITS 13 / PASS1_BITS 2), level shift, clamp and the step to NV12, from the dense int16 coefficient blocks the host's
// entropy decode leaves (jpeg_host.c).  Hand-written HIP for gfx950 (CDNA4, wave64); part of libmi355enc.
//
// One wave64 per task, eight lanes per block.  A luma task is eight horizontally adjacent blocks of one block row: lane 8 b + k loads row k of
// block b (16 bytes; the wave reads 1 KB in one piece), LDS turns rows into columns, lane 8 b + c runs the column pass of column c in
// registers, LDS turns columns into rows, lane 8 b + r runs the row pass of row r and holds eight samples: an output row of the wave is one
// contiguous 64-byte store.  A chroma task of a 4:2:0 / 4:2:2 picture is four U blocks (lanes 0 .. 31) and the four V blocks beside them
// (lanes 32 .. 63): the halves exchange their rows, interleave them and store NV12 directly, 4:2:2 after the rounded mean of each row pair
// inside the block.  Only visible samples are stored; the lanes that own the last visible column, row or chroma pair repeat it up to the
// coded size.  4:4:4 goes through planar scratch and csc_planar_kernel<Y444> (k_csc.hip); grey is luma plus a 128 fill.
// All arithmetic is 32-bit two's complement with wrap-around (unsigned here), the right shifts are arithmetic, the clip is a plain clip.
#include "kernels_common.hpp"

struct jpeg_args {
    const int16_t *coef;  // the blocks, 64 int16 each, natural order
    const uint16_t *qt;   // [3][64], natural order
    unsigned first[3];    // first block of each component
    int bw[3];            // blocks per row of its MCU-padded plane
    int vw, vh;           // visible luma size (even)
    uint8_t *dst[3];      // NV12: luma, interleaved chroma, -; planar (4:4:4): Y, U, V
    int stride, W, H;     // of the destination: row stride, and the size rows / columns are repeated up to (luma samples)
    int lgroups, ntask_l; // luma tasks: groups of eight blocks per block row, and their number
    int cgroups, ntask;   // chroma tasks: groups per block row; all tasks
};

#define JPEG_IN_STRIDE 72 // int16 per block in LDS (144 bytes: the column reads of eight blocks fall into different banks)
#define JPEG_WS_STRIDE 68 // int32 per block in LDS (272 bytes: rows stay 16-byte aligned)

// one 8-point pass of jidctint: d in, o out; SHIFT 11 (columns) or 18 (rows)
template <int SHIFT> DEV void jidct_1d(const unsigned *d, int *o) {
    unsigned z1 = (d[2] + d[6]) * 4433u;
    const unsigned t2 = z1 - d[6] * 15137u, t3 = z1 + d[2] * 6270u;
    const unsigned t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
    const unsigned t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    unsigned o0 = d[7], o1 = d[5], o2 = d[3], o3 = d[1];
    z1 = o0 + o3;
    unsigned z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const unsigned z5 = (z3 + z4) * 9633u;
    o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
    z1 *= 0u - 7373u; z2 *= 0u - 20995u; z3 *= 0u - 16069u; z4 *= 0u - 3196u;
    z3 += z5; z4 += z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    const unsigned rnd = 1u << (SHIFT - 1);
    o[0] = (int)(t10 + o3 + rnd) >> SHIFT; o[7] = (int)(t10 - o3 + rnd) >> SHIFT;
    o[1] = (int)(t11 + o2 + rnd) >> SHIFT; o[6] = (int)(t11 - o2 + rnd) >> SHIFT;
    o[2] = (int)(t12 + o1 + rnd) >> SHIFT; o[5] = (int)(t12 - o1 + rnd) >> SHIFT;
    o[3] = (int)(t13 + o0 + rnd) >> SHIFT; o[4] = (int)(t13 - o0 + rnd) >> SHIFT;
}

// four values that fit 16 bits -> clipped bytes of one word, through the packed 16-bit forms and v_perm (k_csc.hip: csc_pack4)
typedef short jpeg_s2 __attribute__((ext_vector_type(2)));
DEV unsigned ldg16u(const void *p) { return *(const GAS uint16_t *)p; }
DEV unsigned jpeg_pack4(int a, int b, int c, int d) {
    const jpeg_s2 lo = __builtin_bit_cast(jpeg_s2, __builtin_amdgcn_perm((unsigned)b, (unsigned)a, 0x05040100u));
    const jpeg_s2 hi = __builtin_bit_cast(jpeg_s2, __builtin_amdgcn_perm((unsigned)d, (unsigned)c, 0x05040100u));
    const jpeg_s2 l = __builtin_elementwise_min(__builtin_elementwise_max(lo, (jpeg_s2)(0)), (jpeg_s2)(255));
    const jpeg_s2 h = __builtin_elementwise_min(__builtin_elementwise_max(hi, (jpeg_s2)(0)), (jpeg_s2)(255));
    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, h), __builtin_bit_cast(unsigned, l), 0x06040200u);
}

// Eight units (UNIT 1: samples of a plane; 2: chroma pairs) at unit column x0 of row y into a plane whose visible size is vw x vh units: nothing outside
// it; the owner of the last visible unit repeats it up to column Wd, the owners of the last visible row repeat it up to row Hd.  n: units in v (8 or 4).
template <int UNIT, int N> DEV void jpeg_store(uint8_t *dst, int stride, int vw, int vh, int Wd, int Hd, int x0, int y, uint2 v) {
    if (y >= vh || x0 >= vw) return;
    const int nrows = y == vh - 1 ? Hd - y : 1;
    const bool last = x0 + N >= vw, fast = !last || (x0 + N == vw && Wd == vw);
    const unsigned long long val = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
    for (int r = 0; r < nrows; r++) {
        uint8_t *p = dst + (size_t)(y + r) * stride;
        if (fast) stg64(p + UNIT * x0, v);
        else
            for (int x = x0; x < Wd; x++) {
                const int i = (x < vw ? x : vw - 1) - x0;
                if (UNIT == 1) stg8(p + x, (unsigned)(val >> (8 * i)) & 255u);
                else stg16(p + 2 * x, (int)((val >> (16 * i)) & 0xFFFFu));
            }
    }
}

// One launch per picture.  CMODE 0: plane tasks only (luma of a grey picture; Y, U and V of a 4:4:4 picture: plane = task / ntask_l); 1 / 2: the luma tasks, then
// the chroma tasks of a 4:2:0 / 4:2:2 picture.  What a wave does depends on its task alone, so every branch on it is uniform.
template <int CMODE>
__global__ __launch_bounds__(256) void jpeg_idct_kernel(jpeg_args a) {
    __shared__ __attribute__((aligned(16))) int16_t s_in[4][8 * JPEG_IN_STRIDE];
    __shared__ __attribute__((aligned(16))) int s_ws[4][8 * JPEG_WS_STRIDE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, k = lane & 7, bsel = lane >> 3;
    int task = blockIdx.x * 4 + wave;
    const bool live = task < a.ntask; // (every wave reaches the barriers; one past the end works on task 0 and stores nothing)
    if (!live) task = 0;
    const bool chroma = CMODE != 0 && task >= a.ntask_l;
    int comp, brow, bx;
    if (!chroma) {
        comp = task / a.ntask_l;
        const int t = task - comp * a.ntask_l;
        brow = t / a.lgroups;
        bx = (t - brow * a.lgroups) * 8 + bsel;
    } else {
        const int t = task - a.ntask_l;
        comp = 1 + (lane >> 5);
        brow = t / a.cgroups;
        bx = (t - brow * a.cgroups) * 4 + (bsel & 3);
    }
    // (selects, not indexed kernel arguments: an index the compiler cannot resolve would put the arrays into scratch memory)
    const int bwc = comp == 0 ? a.bw[0] : a.bw[1];
    const unsigned first = comp == 0 ? a.first[0] : comp == 1 ? a.first[1] : a.first[2];
    const int bxc = bx < bwc ? bx : bwc - 1; // blocks past the padded plane: read a block that is there, store nothing (their columns are not visible)
    const int16_t *blk = a.coef + ((size_t)first + (size_t)brow * bwc + bxc) * 64;
    *(uint4 *)&s_in[wave][bsel * JPEG_IN_STRIDE + k * 8] = ldg128(blk + k * 8);
    __syncthreads();
    unsigned d[8];
    int o[8];
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = (unsigned)(int)s_in[wave][bsel * JPEG_IN_STRIDE + i * 8 + k] * (unsigned)ldg16u(a.qt + comp * 64 + i * 8 + k);
    jidct_1d<11>(d, o);
#pragma unroll
    for (int i = 0; i < 8; i++) s_ws[wave][bsel * JPEG_WS_STRIDE + i * 8 + k] = o[i];
    __syncthreads();
    const uint4 r0 = *(const uint4 *)&s_ws[wave][bsel * JPEG_WS_STRIDE + k * 8], r1 = *(const uint4 *)&s_ws[wave][bsel * JPEG_WS_STRIDE + k * 8 + 4];
    d[0] = r0.x; d[1] = r0.y; d[2] = r0.z; d[3] = r0.w; d[4] = r1.x; d[5] = r1.y; d[6] = r1.z; d[7] = r1.w;
    jidct_1d<18>(d, o);
    uint2 v = make_uint2(jpeg_pack4(o[0] + 128, o[1] + 128, o[2] + 128, o[3] + 128), jpeg_pack4(o[4] + 128, o[5] + 128, o[6] + 128, o[7] + 128));
    if (!chroma) {
        if (live) jpeg_store<1, 8>(comp == 0 ? a.dst[0] : comp == 1 ? a.dst[1] : a.dst[2], a.stride, a.vw, a.vh, a.W, a.H, bx * 8, brow * 8 + k, v);
        return;
    }
    int cy = brow * 8 + k;
    bool mine = live;
    if (CMODE == 2) { // 4:2:2: the rounded mean of the two rows of a pair, which sit in neighbouring lanes
        v.x = avg4(v.x, (unsigned)__shfl_xor((int)v.x, 1));
        v.y = avg4(v.y, (unsigned)__shfl_xor((int)v.y, 1));
        mine = live && (k & 1) == 0;
        cy = brow * 4 + (k >> 1);
    }
    // U lanes keep samples 0 .. 3 of their row and take V's, V lanes keep samples 4 .. 7 and take U's: each lane stores four pairs
    const unsigned px = (unsigned)__shfl_xor((int)v.x, 32), py = (unsigned)__shfl_xor((int)v.y, 32);
    const int half = lane >> 5;
    const unsigned u = half ? py : v.x, w = half ? v.y : px;
    const uint2 out = make_uint2(__builtin_amdgcn_perm(w, u, 0x05010400u), __builtin_amdgcn_perm(w, u, 0x07030602u));
    if (mine) jpeg_store<2, 4>(a.dst[1], a.stride, a.vw >> 1, a.vh >> 1, a.W >> 1, a.H >> 1, bx * 8 + 4 * half, cy, out);
}

// A picture of vw x vh (even) with luma sampling hs x vs and `comps` components, coefficients and tables on the device as mi355enc_jpeg_entropy_decode lays them
// out, into NV12 surfaces of stride W, coded size W x H.  d_planar (4:4:4 only): scratch of 3 * ((vw + 15) & ~15) * vh bytes.  -1: not a sampling this file takes.
int k_launch_jpeg(const int16_t *d_coef, const uint16_t *d_qt, int hs, int vs, int comps, int vw, int vh, uint8_t *dy, uint8_t *duv, int W, int H,
                  uint8_t *d_planar, hipStream_t s) {
    const int mode = comps == 1 ? 0 : (hs == 2 && vs == 2) ? 1 : (hs == 2 && vs == 1) ? 2 : (hs == 1 && vs == 1) ? 3 : -1;
    if (mode < 0 || (comps != 1 && comps != 3) || (comps == 1 && (hs != 1 || vs != 1)) || vw < 2 || vh < 2 || ((vw | vh) & 1)) return -1;
    jpeg_args a = {};
    const int mcux = (vw + 8 * hs - 1) / (8 * hs), mcuy = (vh + 8 * vs - 1) / (8 * vs);
    a.coef = d_coef; a.qt = d_qt; a.vw = vw; a.vh = vh;
    a.bw[0] = mcux * hs; a.bw[1] = a.bw[2] = comps == 3 ? mcux : 0;
    a.first[0] = 0; a.first[1] = (unsigned)(mcux * hs) * (unsigned)(mcuy * vs); a.first[2] = a.first[1] + (unsigned)mcux * (unsigned)mcuy;
    const int lrows = (vh + 7) / 8;
    a.lgroups = ((vw + 7) / 8 + 7) / 8;
    a.ntask_l = lrows * a.lgroups;
    if (mode == 3) { // planes of the visible size, then the Y444 conversion
        if (!d_planar) return -1;
        const int ps = (vw + 15) & ~15;
        a.dst[0] = d_planar; a.dst[1] = d_planar + (size_t)ps * vh; a.dst[2] = d_planar + 2 * (size_t)ps * vh;
        a.stride = ps; a.W = vw; a.H = vh;
        a.ntask = 3 * a.ntask_l;
        hipLaunchKernelGGL(jpeg_idct_kernel<0>, dim3((a.ntask + 3) / 4), dim3(256), 0, s, a);
        return k_launch_csc2(5, a.dst[0], a.dst[1], a.dst[2], ps, ps, ps, dy, duv, vw, vh, W, H, nullptr, s);
    }
    a.dst[0] = dy; a.dst[1] = duv; a.stride = W; a.W = W; a.H = H;
    if (mode == 0) {
        a.ntask = a.ntask_l;
        hipLaunchKernelGGL(jpeg_idct_kernel<0>, dim3((a.ntask + 3) / 4), dim3(256), 0, s, a);
        return hipMemsetAsync(duv, 0x80, (size_t)W * (H / 2), s) == hipSuccess ? 0 : -1;
    }
    const int cw = vw / 2, crows = mode == 1 ? (vh / 2 + 7) / 8 : (vh + 7) / 8;
    a.cgroups = ((cw + 7) / 8 + 3) / 4;
    a.ntask = a.ntask_l + crows * a.cgroups;
    if (mode == 1) hipLaunchKernelGGL(jpeg_idct_kernel<1>, dim3((a.ntask + 3) / 4), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(jpeg_idct_kernel<2>, dim3((a.ntask + 3) / 4), dim3(256), 0, s, a);
    return 0;
}
