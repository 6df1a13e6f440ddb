// k_quality.hip -- per-picture quality metrics: the squared error of Y, Cb and Cr over the visible samples and x264's
// integer SSIM of the luma, source against deblocked reconstruction, in one flat launch.
//
// One workgroup of 256 threads per 64 x 64 luma tile (16 x 16 blocks of 4 x 4 samples, one block per thread) and the 64-byte x 32-row part of
// the interleaved chroma plane under it (two dwords per thread).  A thread's four row pairs give the block's sums s1 = sum(src), s2 = sum(rec),
// ss = sum(src^2) + sum(rec^2), s12 = sum(src * rec) by v_sad_u8 against zero and v_dot4_u32_u8, four samples per instruction; the squared error
// is ss - 2 s12 of the same sums.  An SSIM window is a 2 x 2 group of blocks at EVERY block position, so windows straddle tiles: the tile also
// computes the 33 blocks one block to the right of and below it (threads 0 .. 32), and all 17 x 17 sums go through LDS (4.6 KB).  No workgroup
// waits for another one.
// Samples beyond the visible width x height never count: a dword is loaded only where all four of its bytes are visible (and, for planes whose
// address or stride is not a multiple of four, byte by byte), the two visible bytes of a width = 2 (mod 4) by themselves, and a dword or row
// outside reads as zero on both sides, which adds nothing to any sum.
// Reduction: a __shfl_xor ladder over the wave, LDS over the four waves, then ONE 64-bit integer atomic add per accumulator and workgroup
// into one of the picture's 32 sets of five words (integers: the result does not depend on the order; sets on different memory channels, so that the
// adds do not queue up at one word).  The workgroup that draws the last ticket takes the sets out (atomic exchange with zero: the block is clear again
// for the slot's next picture, in stream order), sums them and writes the totals to `out` with ordinary vector stores -- pinned host memory in the encoder; no atomic ever targets host memory.
// Arithmetic of a window: 64-bit integers, then IEEE binary64 with one rounding per operation (two products, one quotient; the scaling by 2^30
// is exact) and round-half-even -- what tests/qualityref.py computes with numpy.  No fast-math, no reciprocal, no contraction in this file.
#include "kernels_common.hpp"
#pragma clang fp contract(off)

#define Q_BLOCKS 16                /* blocks per tile side */
#define Q_TILE (4 * Q_BLOCKS)      /* luma samples per tile side */
#define Q_LDS (Q_BLOCKS + 1)       /* ... and block sums per side with the halo */
#define Q_SSIM_C1 416              /* x264: (int)(.01 * .01 * 255 * 255 * 64 + .5) */
#define Q_SSIM_C2 235963           /* x264: (int)(.03 * .03 * 255 * 255 * 64 * 63 + .5) */

struct quality_args {
    const uint8_t *sy, *suv, *ry, *ruv; // source / reconstruction, NV12
    int ss, rs;                         // their strides
    int w, h;                           // visible size
    int s_al, r_al;                     // address and stride are multiples of four: dword loads
    unsigned long long *acc;            // QUALITY_SHARDS sets of {[0..2] SSE of Y, Cb, Cr, [3] sum of q, [4] windows}, and the ticket (a dword) at word QUALITY_TICKET_WORD
    unsigned long long *out;            // where the last workgroup leaves [0..4]
    unsigned nwg;
};

// four bytes of a row at x0 (a multiple of four; w even): the visible ones, zero for the rest
DEV unsigned q_ld4(const uint8_t *row, int x0, int w, bool al) {
    if (x0 + 4 <= w) {
        if (al) return ldg32(row + x0);
        return ldg8(row + x0) | (ldg8(row + x0 + 1) << 8) | (ldg8(row + x0 + 2) << 16) | (ldg8(row + x0 + 3) << 24);
    }
    if (x0 + 2 <= w) return ldg8(row + x0) | (ldg8(row + x0 + 1) << 8);
    return 0u;
}
// sums of luma block (bx, by) (picture block coordinates): {s1, s2, ss, s12}
DEV uint4 q_block(const quality_args &a, int bx, int by) {
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int y = 4 * by + i;
        if (y < a.h) {
            const unsigned p = q_ld4(a.sy + (size_t)y * a.ss, 4 * bx, a.w, a.s_al != 0), q = q_ld4(a.ry + (size_t)y * a.rs, 4 * bx, a.w, a.r_al != 0);
            r.x = __builtin_amdgcn_sad_u8(p, 0u, r.x);
            r.y = __builtin_amdgcn_sad_u8(q, 0u, r.y);
            r.z = __builtin_amdgcn_udot4(p, p, __builtin_amdgcn_udot4(q, q, r.z, false), false);
            r.w = __builtin_amdgcn_udot4(p, q, r.w, false);
        }
    }
    return r;
}
DEV long long q_window(const uint4 a, const uint4 b, const uint4 c, const uint4 d) {
    const long long s1 = (long long)(a.x + b.x + c.x + d.x), s2 = (long long)(a.y + b.y + c.y + d.y);
    const long long ss = (long long)(a.z + b.z + c.z + d.z), s12 = (long long)(a.w + b.w + c.w + d.w);
    const long long vars = 64 * ss - s1 * s1 - s2 * s2, covar = 64 * s12 - s1 * s2;
    const long long A = 2 * s1 * s2 + Q_SSIM_C1, B = 2 * covar + Q_SSIM_C2, C = s1 * s1 + s2 * s2 + Q_SSIM_C1, D = vars + Q_SSIM_C2;
    const double num = (double)A * (double)B, den = (double)C * (double)D; // every factor is an integer below 2^53: exact
    return (long long)__builtin_rint(num / den * 1073741824.0);
}

__global__ __launch_bounds__(256) void quality_kernel(const quality_args a) {
    __shared__ uint4 blk[Q_LDS * Q_LDS];
    __shared__ unsigned long long red[4][5];
    __shared__ int last;
    const int t = threadIdx.x, lx = t & (Q_BLOCKS - 1), ly = t >> 4;
    const int bx0 = blockIdx.x * Q_BLOCKS, by0 = blockIdx.y * Q_BLOCKS;
    const uint4 mine = q_block(a, bx0 + lx, by0 + ly);
    blk[ly * Q_LDS + lx] = mine;
    if (t < 2 * Q_BLOCKS + 1) { // the halo: column 16 (rows 0 .. 16), then row 16 (columns 0 .. 15)
        const int hx = t < Q_LDS ? Q_BLOCKS : t - Q_LDS, hy = t < Q_LDS ? t : Q_BLOCKS;
        blk[hy * Q_LDS + hx] = q_block(a, bx0 + hx, by0 + hy);
    }
    unsigned sse_y = mine.z - 2u * mine.w, sse_u = 0, sse_v = 0; // sum (p - q)^2 = sum p^2 + sum q^2 - 2 sum p q
    // chroma under the tile: 32 rows of 16 dwords {Cb Cr Cb Cr}; thread t takes dword lx of rows ly and ly + 16
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int y = (by0 * 4 >> 1) + ly + 16 * k, x0 = 4 * (bx0 + lx);
        if (y < (a.h >> 1)) {
            const unsigned p = q_ld4(a.suv + (size_t)y * a.ss, x0, a.w, a.s_al != 0), q = q_ld4(a.ruv + (size_t)y * a.rs, x0, a.w, a.r_al != 0);
            const unsigned pu = p & 0x00FF00FFu, qu = q & 0x00FF00FFu, pv = p & 0xFF00FF00u, qv = q & 0xFF00FF00u;
            sse_u += __builtin_amdgcn_udot4(pu, pu, 0u, false) + __builtin_amdgcn_udot4(qu, qu, 0u, false) - 2u * __builtin_amdgcn_udot4(pu, qu, 0u, false);
            sse_v += __builtin_amdgcn_udot4(pv, pv, 0u, false) + __builtin_amdgcn_udot4(qv, qv, 0u, false) - 2u * __builtin_amdgcn_udot4(pv, qv, 0u, false);
        }
    }
    __syncthreads();
    long long qsum = 0;
    unsigned nwin = 0;
    if (bx0 + lx < (a.w >> 2) - 1 && by0 + ly < (a.h >> 2) - 1) {
        const uint4 *b = &blk[ly * Q_LDS + lx];
        qsum = q_window(b[0], b[1], b[Q_LDS], b[Q_LDS + 1]);
        nwin = 1;
    }
    // per thread at most 16 * 255^2 < 2^21 per plane: 256 of them fit 32 bits
    for (int o = 32; o; o >>= 1) {
        sse_y += (unsigned)__shfl_xor((int)sse_y, o, 64); sse_u += (unsigned)__shfl_xor((int)sse_u, o, 64); sse_v += (unsigned)__shfl_xor((int)sse_v, o, 64);
        nwin += (unsigned)__shfl_xor((int)nwin, o, 64);
        qsum += __shfl_xor(qsum, o, 64);
    }
    if ((t & 63) == 0) {
        unsigned long long *r = red[t >> 6];
        r[0] = sse_y; r[1] = sse_u; r[2] = sse_v; r[3] = (unsigned long long)qsum; r[4] = nwin;
    }
    __syncthreads();
    GAS unsigned *ticket = (GAS unsigned *)(a.acc + QUALITY_TICKET_WORD);
    if (t == 0) {
        // hundreds of workgroups adding to ONE word queue up at that word's memory channel (measured: 43 us at 1080p with a single set of accumulators): the workgroups
        // spread over QUALITY_SHARDS sets, QUALITY_SHARD_STRIDE words apart
        GAS unsigned long long *acc = (GAS unsigned long long *)a.acc + (size_t)((blockIdx.y * gridDim.x + blockIdx.x) & (QUALITY_SHARDS - 1)) * QUALITY_SHARD_STRIDE;
#pragma unroll
        for (int i = 0; i < 5; i++)
            __hip_atomic_fetch_add(acc + i, red[0][i] + red[1][i] + red[2][i] + red[3][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the adds have been performed before the ticket is drawn
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.nwg - 1u ? 1 : 0;
    }
    __syncthreads();
    if (last && t < 64) { // the last workgroup of the picture, its first wave: lane k takes set k out and leaves it clear, then the sets are summed over the wave
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        unsigned long long v[5];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            v[i] = 0;
            if (t < QUALITY_SHARDS) v[i] = __hip_atomic_exchange((GAS unsigned long long *)a.acc + (size_t)t * QUALITY_SHARD_STRIDE + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int o = 32; o; o >>= 1) v[i] += (unsigned long long)__shfl_xor((long long)v[i], o, 64);
        }
        if (t == 0) {
#pragma unroll
            for (int i = 0; i < 5; i++) { const v2u w = {(unsigned)v[i], (unsigned)(v[i] >> 32)}; *((GAS v2u *)a.out + i) = w; }
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

void k_launch_quality(const uint8_t *src_y, const uint8_t *src_uv, int src_stride, const uint8_t *rec_y, const uint8_t *rec_uv, int rec_stride,
                      int width, int height, unsigned long long *d_acc, unsigned long long *out, hipStream_t s) {
    quality_args a;
    a.sy = src_y; a.suv = src_uv; a.ry = rec_y; a.ruv = rec_uv; a.ss = src_stride; a.rs = rec_stride; a.w = width; a.h = height;
    a.s_al = (((uintptr_t)src_y | (uintptr_t)src_uv | (uintptr_t)src_stride) & 3) == 0;
    a.r_al = (((uintptr_t)rec_y | (uintptr_t)rec_uv | (uintptr_t)rec_stride) & 3) == 0;
    a.acc = d_acc; a.out = out;
    const dim3 grid((unsigned)((width + Q_TILE - 1) / Q_TILE), (unsigned)((height + Q_TILE - 1) / Q_TILE));
    a.nwg = grid.x * grid.y;
    hipLaunchKernelGGL(quality_kernel, grid, dim3(256), 0, s, a);
}
