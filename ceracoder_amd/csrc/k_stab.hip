// k_stab.hip -- electronic image stabilisation: the projection launch (band-wise column and row sums of the submitted luma) and
// the match launch (votes of the eight projections against the previous picture's, both medians, the trajectory step).  All integers; the rule is
// stab_host.h's.  Hand-written HIP for gfx950 (CDNA4, wave64); part of libmi355enc (see kernels_common.hpp).
#include "kernels_common.hpp"
#include "stab_host.h"

#define STAB_TILE_COLS 1024 /* luma columns per workgroup: 256 threads x 4 */
#define STAB_TILE_ROWS 16   /* rows per workgroup, inside one horizontal band */

DEV unsigned stab_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}
DEV unsigned long long stab_wave_sum64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
    return v;
}

// four luma samples `step` (1 or 2) bytes apart from address p on, as one word: whole dwords at their natural alignment, shifted into place.  Every dword
// read holds at least one of the bytes asked for, so nothing is read from a page the samples do not lie in.
template <int STEP> DEV unsigned stab_load4(const uint8_t *p) {
    const uintptr_t A = (uintptr_t)p;
    const uint8_t *al = (const uint8_t *)(A & ~(uintptr_t)3);
    const unsigned sh = (unsigned)(A & 3);
    const unsigned d0 = ldg32(al);
    if (STEP == 1) {
        const unsigned d1 = sh ? ldg32(al + 4) : 0u;
        return __builtin_amdgcn_alignbyte(d1, d0, sh);
    }
    const unsigned d1 = ldg32(al + 4);              // (holds byte p[4])
    const unsigned d2 = sh >= 2 ? ldg32(al + 8) : 0u; // (p[6] lies there only then)
    const unsigned lo = __builtin_amdgcn_alignbyte(d1, d0, sh), hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
    return __builtin_amdgcn_perm(hi, lo, 0x06040200u); // bytes 0, 2 of lo, then 0, 2 of hi
}

struct stab_proj_args {
    const uint8_t *luma; // the first luma sample
    int stride, w, h;
    unsigned *sums;      // C_0 .. C_3 (w each), R_0 .. R_3 (h each): cleared in front of the launch
    int chunks;          // workgroups per horizontal band along y
};

// A workgroup owns STAB_TILE_COLS columns x STAB_TILE_ROWS rows inside horizontal band k.  A thread reads four neighbouring samples per row (a wave: 256
// contiguous samples): their column sums stay in registers over the rows and leave with one atomic each; the row's sum is v_sad_u8 against zero, reduced
// over the wave where the wave lies inside one vertical band (nearly always), and gathered in LDS per (row, vertical band); one atomic per such sum at the end.
template <int STEP> __global__ __launch_bounds__(256) void stab_project_kernel(const stab_proj_args a) {
    __shared__ unsigned racc[STAB_TILE_ROWS * STAB_BANDS];
    const int tid = threadIdx.x;
    const int k = (int)blockIdx.y / a.chunks, chunk = (int)blockIdx.y - k * a.chunks;
    const int r0 = stab_band(k, a.h) + chunk * STAB_TILE_ROWS;
    const int rend = stab_band(k + 1, a.h), r1 = r0 + STAB_TILE_ROWS < rend ? r0 + STAB_TILE_ROWS : rend;
    if (r0 >= r1) return; // (block-uniform: the bands' heights differ by one row)
    if (tid < STAB_TILE_ROWS * STAB_BANDS) racc[tid] = 0;
    __syncthreads();
    const int b1 = stab_band(1, a.w), b2 = stab_band(2, a.w), b3 = stab_band(3, a.w);
    auto vband = [&](int x) { return (x >= b1) + (x >= b2) + (x >= b3); };
    const int x0 = (int)blockIdx.x * STAB_TILE_COLS + 4 * tid;
    const int nvalid = a.w - x0 >= 4 ? 4 : a.w - x0 > 0 ? a.w - x0 : 0;
    const int kb0 = vband(x0);
    const bool whole = nvalid == 4 && vband(x0 + 3) == kb0;
    const int wx0 = (int)blockIdx.x * STAB_TILE_COLS + 4 * (tid & ~63);
    const bool wave_uni = wx0 + 255 < a.w && vband(wx0) == vband(wx0 + 255); // (wave-uniform)
    unsigned col[4] = {0, 0, 0, 0};
    for (int r = r0; r < r1; r++) {
        const uint8_t *rp = a.luma + (size_t)r * a.stride + (size_t)x0 * STEP;
        unsigned px = 0;
        if (nvalid == 4) px = stab_load4<STEP>(rp);
        else for (int b = 0; b < nvalid; b++) px |= ldg8(rp + b * STEP) << (8 * b); // the row's tail, byte by byte
#pragma unroll
        for (int b = 0; b < 4; b++) col[b] += (px >> (8 * b)) & 255u;
        unsigned *ra = racc + (r - r0) * STAB_BANDS;
        if (wave_uni) {
            const unsigned s = stab_wave_sum(__builtin_amdgcn_sad_u8(px, 0u, 0u));
            if ((tid & 63) == 0) atomicAdd(ra + kb0, s);
        } else if (whole) {
            const unsigned s = __builtin_amdgcn_sad_u8(px, 0u, 0u);
            if (s) atomicAdd(ra + kb0, s);
        } else
            for (int b = 0; b < nvalid; b++) atomicAdd(ra + vband(x0 + b), (px >> (8 * b)) & 255u); // a vertical band's edge inside the four, or the tail
    }
    for (int b = 0; b < nvalid; b++) if (col[b]) atomicAdd(a.sums + (size_t)k * a.w + x0 + b, col[b]);
    __syncthreads();
    if (tid < STAB_TILE_ROWS * STAB_BANDS) {
        const int y = r0 + (tid >> 2), kb = tid & 3;
        if (y < r1 && racc[tid]) atomicAdd(a.sums + (size_t)STAB_BANDS * a.w + (size_t)kb * a.h + y, racc[tid]);
    }
}

int k_launch_stab_project(const uint8_t *luma, int stride, int step, int w, int h, unsigned *sums, hipStream_t s) {
    if (!luma || !sums || w < 1 || h < 1 || w > 8192 || h > 8192 || (step != 1 && step != 2)) return -1;
    stab_proj_args a;
    a.luma = luma; a.stride = stride; a.w = w; a.h = h; a.sums = sums;
    a.chunks = ((h + STAB_BANDS - 1) / STAB_BANDS + STAB_TILE_ROWS - 1) / STAB_TILE_ROWS; // (the tallest band: ceil(h / 4) rows)
    const dim3 grid((w + STAB_TILE_COLS - 1) / STAB_TILE_COLS, STAB_BANDS * a.chunks), blk(256);
    if (step == 1) hipLaunchKernelGGL((stab_project_kernel<1>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((stab_project_kernel<2>), grid, blk, 0, s, a);
    return 0;
}

struct stab_match_args {
    const unsigned *prev, *cur; // the sums of the previous and of this picture
    int w, h, range, leak, prime;
    int lo_x, hi_x, lo_y, hi_y; // this picture's bounds
    int *state;                 // {Sx, Sy}: the trajectory, read and written
    int *rec;                   // STAB_REC_WORDS words: the slot's record
};

// One workgroup, a wave per projection (0 .. 3 the column sums of the horizontal bands, 4 .. 7 the row sums of the vertical ones); nothing waits for another
// workgroup.  A lane owns the positions x = range + 64 c + lane and keeps one partial cost per shift in registers (at most 128 terms of at most 2048 * 255:
// 32 bits hold it); the previous picture's sums around a chunk go through LDS once.  The shifts' totals are 64-bit sums over the wave.  Every index stays in
// [0, n): x - d with x in [range, n - range), and the window's loads are guarded.  Thread 0 takes the medians and the trajectory step.
__global__ __launch_bounds__(512) void stab_match_kernel(const stab_match_args a) {
    __shared__ unsigned win[2 * STAB_BANDS][64 + 2 * STAB_RANGE_MAX];
    __shared__ int vote[2 * STAB_BANDS], ok[2 * STAB_BANDS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int R = a.range;
    if (!a.prime) {
        const int n = wave < STAB_BANDS ? a.w : a.h;
        const size_t at = wave < STAB_BANDS ? (size_t)wave * a.w : (size_t)STAB_BANDS * a.w + (size_t)(wave - STAB_BANDS) * a.h;
        const unsigned *p = a.cur + at, *q = a.prev + at;
        const int nmax = a.w > a.h ? a.w : a.h, chunks = (nmax - 2 * R + 63) >> 6; // (the same count for every wave: the barriers below are the workgroup's)
        unsigned acc[2 * STAB_RANGE_MAX + 1];
#pragma unroll
        for (int j = 0; j <= 2 * STAB_RANGE_MAX; j++) acc[j] = 0;
        for (int c = 0; c < chunks; c++) {
            const int xs = R + 64 * c; // the chunk's first position; its window: q[xs - R .. xs + 63 + R]
            for (int i = lane; i < 64 + 2 * R; i += 64) { const int idx = xs - R + i; win[wave][i] = idx < n ? ldg32(q + idx) : 0u; }
            const int x = xs + lane;
            const bool valid = x < n - R;
            const unsigned pv = valid ? ldg32(p + x) : 0u;
            __syncthreads();
#pragma unroll
            for (int j = 0; j <= 2 * STAB_RANGE_MAX; j++)
                if (j <= 2 * R) { // d = j - R: q[x - d] is the window's entry lane + 2 R - j
                    const unsigned qv = win[wave][lane + 2 * R - j];
                    acc[j] += valid ? (pv > qv ? pv - qv : qv - pv) : 0u;
                }
            __syncthreads();
        }
        unsigned long long best = 0;
        int d_at = 0, ties = 0;
#pragma unroll
        for (int j = 0; j <= 2 * STAB_RANGE_MAX; j++)
            if (j <= 2 * R) {
                const unsigned long long t = stab_wave_sum64(acc[j]);
                if (j == 0 || t < best) { best = t; d_at = j - R; ties = 0; }
                else if (t == best) ties++;
            }
        if (lane == 0) { vote[wave] = d_at; ok[wave] = !ties && d_at > -R && d_at < R; }
    }
    __syncthreads();
    if (tid != 0) return;
    int rec[STAB_REC_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!a.prime) {
        int v[STAB_BANDS], nx = 0, ny = 0;
        for (int k = 0; k < STAB_BANDS; k++) if (ok[k]) v[nx++] = vote[k];
        rec[0] = stab_median(v, nx);
        for (int k = 0; k < STAB_BANDS; k++) if (ok[STAB_BANDS + k]) v[ny++] = vote[STAB_BANDS + k];
        rec[1] = stab_median(v, ny);
        rec[2] = nx; rec[3] = ny;
        stab_step(a.state[0], rec[0], a.leak, a.lo_x, a.hi_x, &rec[6], &rec[4]);
        stab_step(a.state[1], rec[1], a.leak, a.lo_y, a.hi_y, &rec[7], &rec[5]);
    }
    a.state[0] = rec[6]; a.state[1] = rec[7];
    for (int i = 0; i < STAB_REC_WORDS; i++) a.rec[i] = rec[i];
}

int k_launch_stab_match(const unsigned *prev, const unsigned *cur, int w, int h, int range, int leak, int prime, const int bounds[4], int *state, int *rec, hipStream_t s) {
    if (!prev || !cur || !state || !rec || !bounds || range < 1 || range > STAB_RANGE_MAX || w < 4 * range || h < 4 * range || w > 8192 || h > 8192) return -1;
    stab_match_args a;
    a.prev = prev; a.cur = cur; a.w = w; a.h = h; a.range = range; a.leak = leak; a.prime = prime;
    a.lo_x = bounds[0]; a.hi_x = bounds[1]; a.lo_y = bounds[2]; a.hi_y = bounds[3]; a.state = state; a.rec = rec;
    hipLaunchKernelGGL(stab_match_kernel, dim3(1), dim3(512), 0, s, a);
    return 0;
}
