// k_autolevel.hip -- automatic levels and white balance on the coded NV12 surfaces of a slot (the rule: autolevel_host.h).  Three launches
// on one stream:
//
//   measure   k_adjust.hip's ownership: a thread owns an 8 x 2 luma patch and its four chroma pairs (8-byte loads), so a chroma sample and its co-sited luma
//             sit in one thread and the vote needs no second pass.  At most AL_SLABS_MAX workgroups walk the patches of the rectangle's visible part in a
//             grid-stride loop; each keeps one histogram per wave in LDS (4 x 256 words, ds_add_u32) and stores its sum and {n, su, sv} as a slab with plain
//             stores: no global atomic, no clear in front of the launch, and the result does not depend on the order the workgroups ran in.
//             Equal codes are folded before they reach an LDS counter, twice: inside a lane, a run of equal codes in the lane's 16 samples is one add of its
//             length; across the wave, the lanes that flush the code of the first flushing lane are summed (DPP) and added once, by that lane, and -- where
//             that took at least a quarter of them -- the same again for the lanes that are left; what still remains adds for itself.  A flat picture is
//             one add of 1024 per wave and trip of the loop, a picture of two codes one or two per flush, whatever their order; noise pays one round and
//             then adds lane by lane.
//   decide    one workgroup of 256: thread v sums bin v over the slabs, the prefix sum runs through LDS, lo / hi are an LDS min / max over the threads whose
//             code qualifies, thread 0 takes the state step and the divisions (al_decide, the host's own function), all threads write A[v].  Writes the state,
//             the slot's record and the slot's table; waits for nothing but its own loads.
//   apply     k_adjust.hip's pointwise form, in place; its 256-byte table and two offsets come from the record the decide launch wrote: the first wave brings
//             the table into LDS, a look-up is one ds_read_u8.  A plane whose correction is neutral (levels 0; both offsets 0, which only the device knows) is
//             neither read nor written.
// No scratch, no global atomics, no wait on another workgroup.
#include "kernels_common.hpp"
#include "autolevel_host.h"

// ------------------------------------------------------------------ measure
struct al_measure_args {
    const uint8_t *y, *uv;
    int W;
    int px0, pcols, py0, total; // the patches that meet the measured part: first patch column, their count per row, first patch row, their number
    int mx0, mx1, my0, my1;     // the measured part: the rectangle's visible samples (mx0, my0 even)
    int lb, ub, reach;          // the vote's luma bounds and chroma reach
    unsigned *slabs;
};

// the lanes with `have` add cnt to hist[v]: up to two rounds of folding on the first such lane's code, then lane by lane.  Every lane of the wave calls.
DEV void al_flush(unsigned *hist, int lane, int v, unsigned cnt, bool have) {
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const unsigned long long pend = __ballot(have);
        if (!pend) return; // (uniform)
        const int leader = __ffsll((long long)pend) - 1, lv = __builtin_amdgcn_readlane(v, leader);
        const bool m = have && v == lv;
        const unsigned total = (unsigned)wave64_sum(m ? (int)cnt : 0);
        if (lane == leader) atomicAdd(&hist[lv], total);
        have = have && !m;
        if (4 * __popcll(__ballot(m)) < __popcll(pend)) break; // (uniform) the first code took less than a quarter of the lanes: many codes, a second round folds little
    }
    if (have) atomicAdd(&hist[v], cnt);
}

__global__ __launch_bounds__(256) void al_measure_kernel(al_measure_args a) {
    __shared__ unsigned hist[4][256];
    __shared__ unsigned tot[3];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int w = 0; w < 4; w++) hist[w][tid] = 0;
    if (tid < 3) tot[tid] = 0;
    __syncthreads();
    unsigned *mine = hist[wave];
    unsigned n = 0, su = 0, sv = 0;
    const int step = (int)gridDim.x * 256;
    for (int base = (int)blockIdx.x * 256; base < a.total; base += step) { // (the same trips for every lane of a workgroup: al_flush is the wave's)
        const int p = base + tid;
        const bool have = p < a.total;
        const int pr = have ? p / a.pcols : 0, pc = have ? p - pr * a.pcols : 0;
        const int x0 = (a.px0 + pc) * 8, yy = 2 * (a.py0 + pr);
        uint2 s0 = make_uint2(0, 0), s1 = s0, sc = s0;
        if (have) {
            const uint8_t *py = a.y + (size_t)yy * a.W + x0;
            s0 = ldg64(py); s1 = ldg64(py + a.W); sc = ldg64(a.uv + (size_t)(yy >> 1) * a.W + x0);
        }
        const unsigned lw[4] = {s0.x, s0.y, s1.x, s1.y};
        int cur = 0;
        unsigned cnt = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r = i >> 3, k = i & 7, v = byte_of(lw[i >> 2], i & 3);
            const bool ok = have && x0 + k >= a.mx0 && x0 + k < a.mx1 && yy + r < a.my1;
            const bool same = ok && cnt && v == cur;
            al_flush(mine, lane, cur, cnt, ok && cnt && !same);
            if (ok) { cnt = same ? cnt + 1 : 1; cur = v; }
        }
        al_flush(mine, lane, cur, cnt, cnt != 0);
        const unsigned cw[2] = {sc.x, sc.y};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int cb = byte_of(cw[k >> 1], 2 * (k & 1)), cr = byte_of(cw[k >> 1], 2 * (k & 1) + 1), yv = byte_of(lw[k >> 1], 2 * (k & 1));
            const bool vote = have && x0 + 2 * k >= a.mx0 && x0 + 2 * k < a.mx1 && yv >= a.lb && yv <= a.ub && iabs(cb - 128) <= a.reach && iabs(cr - 128) <= a.reach;
            n += vote ? 1u : 0u; su += vote ? (unsigned)cb : 0u; sv += vote ? (unsigned)cr : 0u;
        }
    }
    const unsigned wn = (unsigned)wave64_sum((int)n), wu = (unsigned)wave64_sum((int)su), wv = (unsigned)wave64_sum((int)sv);
    if (lane == 0) { atomicAdd(&tot[0], wn); atomicAdd(&tot[1], wu); atomicAdd(&tot[2], wv); }
    __syncthreads();
    unsigned *slab = a.slabs + (size_t)blockIdx.x * AL_SLAB_WORDS;
    stg32(slab + tid, hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid]);
    if (tid < 4) stg32(slab + 256 + tid, tid < 3 ? tot[tid] : 0u);
}

// y, uv: NV12 surfaces of W x H (W a multiple of 8, H even) at stride W, 8-byte aligned; rect: x0, x1, y0, y1 (even, inside the surfaces); vw x vh: the visible
// size, which the rectangle meets; slabs: room for AL_SLABS_MAX slabs.  Returns the number of slabs written (1 .. AL_SLABS_MAX), -1: arguments outside that.
int k_launch_autolevel_measure(const uint8_t *y, const uint8_t *uv, int W, int H, const int rect[4], int vw, int vh, int full_range, int reach, unsigned *slabs, hipStream_t s) {
    if (!y || !uv || !rect || !slabs || W <= 0 || H <= 0 || W > 8192 || H > 8192 || (W & 7) || (H & 1) || ((((uintptr_t)y) | ((uintptr_t)uv)) & 7) || reach < 0 || reach > 127) return -1;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return -1;
    if (vw < 1 || vh < 1 || vw > W || vh > H || rect[0] >= vw || rect[2] >= vh) return -1;
    al_measure_args a;
    a.y = y; a.uv = uv; a.W = W;
    a.mx0 = rect[0]; a.mx1 = rect[1] < vw ? rect[1] : vw; a.my0 = rect[2]; a.my1 = rect[3] < vh ? rect[3] : vh;
    a.px0 = a.mx0 >> 3; a.pcols = ((a.mx1 + 7) >> 3) - a.px0; a.py0 = a.my0 >> 1;
    a.total = a.pcols * (((a.my1 + 1) >> 1) - a.py0);
    const int B = al_black(full_range), S = al_scale(full_range);
    a.lb = al_vote_lo(B, S); a.ub = al_vote_hi(B, S); a.reach = reach;
    a.slabs = slabs;
    int g = (a.total + 255) / 256;
    g = g > AL_SLABS_MAX ? AL_SLABS_MAX : g;
    hipLaunchKernelGGL(al_measure_kernel, dim3(g), dim3(256), 0, s, a);
    return g;
}

// ------------------------------------------------------------------ decide
struct al_decide_args {
    const unsigned *slabs;
    int nslabs;
    unsigned NC;
    int set[7];
    int B, S, prime;
    int *state, *rec;
};

__global__ __launch_bounds__(256) void al_decide_kernel(al_decide_args a) {
    __shared__ unsigned cum[2][256];
    __shared__ unsigned part[3][4];
    __shared__ int s_lo, s_hi;
    __shared__ al_interval_t s_iv;
    __shared__ unsigned tabw[64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned c = 0;
    for (int g0 = 0; g0 < a.nslabs; g0 += 32) { // 32 loads in flight per round: the launch's time is these round trips
        unsigned t[32];
#pragma unroll
        for (int k = 0; k < 32; k++) { const int g = g0 + k < a.nslabs ? g0 + k : a.nslabs - 1; t[k] = ldg32(a.slabs + (size_t)g * AL_SLAB_WORDS + tid); }
#pragma unroll
        for (int k = 0; k < 32; k++) c += g0 + k < a.nslabs ? t[k] : 0u;
    }
    // {n, su, sv}: slab tid's in thread tid; a wave's 64 stay below 2^32 (a slab's share of 2^24 chroma samples), the four waves are added in 64 bits
    unsigned pn = 0, pu = 0, pv = 0;
    if (tid < a.nslabs) { const unsigned *t = a.slabs + (size_t)tid * AL_SLAB_WORDS + 256; pn = ldg32(t); pu = ldg32(t + 1); pv = ldg32(t + 2); }
    pn = (unsigned)wave64_sum((int)pn); pu = (unsigned)wave64_sum((int)pu); pv = (unsigned)wave64_sum((int)pv);
    if (lane == 0) { part[0][wave] = pn; part[1][wave] = pu; part[2][wave] = pv; }
    cum[0][tid] = c;
    if (tid == 0) { s_lo = 255; s_hi = 0; }
    __syncthreads();
    int src = 0;
    for (int d = 1; d < 256; d <<= 1) {
        unsigned x = cum[src][tid];
        if (tid >= d) x += cum[src][tid - d];
        cum[src ^ 1][tid] = x;
        __syncthreads();
        src ^= 1;
    }
    const unsigned incl = cum[src][tid], N = cum[src][255];
    if (al_is_lo(incl, N, a.set[3])) atomicMin(&s_lo, tid);
    if (al_is_hi(incl - c, N, a.set[4])) atomicMax(&s_hi, tid);
    __syncthreads();
    if (tid == 0) {
        int st[4], rec[AL_REC_WORDS];
#pragma unroll
        for (int i = 0; i < 4; i++) st[i] = (int)ldg32(a.state + i);
        const unsigned n = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const uint64_t su = (uint64_t)part[1][0] + part[1][1] + part[1][2] + part[1][3], sv = (uint64_t)part[2][0] + part[2][1] + part[2][2] + part[2][3];
        s_iv = al_decide(s_lo, s_hi, n, su, sv, a.NC, a.set, a.B, a.S, a.prime, st, rec);
#pragma unroll
        for (int i = 0; i < 4; i++) stg32(a.state + i, (unsigned)st[i]);
#pragma unroll
        for (int i = 0; i < AL_REC_WORDS; i++) stg32(a.rec + i, (unsigned)rec[i]);
    }
    __syncthreads();
    ((uint8_t *)tabw)[tid] = (uint8_t)al_table(tid, s_iv, a.B, a.S);
    __syncthreads();
    if (tid < 64) stg32(a.rec + AL_TAB_AT + tid, tabw[tid]);
}

// slabs: nslabs (1 .. AL_SLABS_MAX) slabs of a measure launch; NC: the visible chroma samples; set: the checked setting's seven fields; state: 4 words, read
// (unless prime) and written; rec: AL_SLOT_WORDS words -- the record, room, the table.  -1: arguments outside that.
int k_launch_autolevel_decide(const unsigned *slabs, int nslabs, unsigned NC, const int set[7], int full_range, int prime, int *state, int *rec, hipStream_t s) {
    if (!slabs || !set || !state || !rec || nslabs < 1 || nslabs > AL_SLABS_MAX) return -1;
    al_decide_args a;
    a.slabs = slabs; a.nslabs = nslabs; a.NC = NC;
    for (int i = 0; i < 7; i++) a.set[i] = set[i];
    a.B = al_black(full_range); a.S = al_scale(full_range); a.prime = prime ? 1 : 0;
    a.state = state; a.rec = rec;
    hipLaunchKernelGGL(al_decide_kernel, dim3(1), dim3(256), 0, s, a);
    return 0;
}

// ------------------------------------------------------------------ apply
struct al_apply_args {
    uint8_t *y, *uv;
    int W, H, x0, x1, y0, y1; // the picture rectangle (even)
    const int *rec;           // the decide launch's: offsets at words 9 / 10, the table from word AL_TAB_AT on
};

DEV unsigned al_lut4(const uint8_t *t, unsigned w) { return (unsigned)t[w & 255u] | ((unsigned)t[(w >> 8) & 255u] << 8) | ((unsigned)t[(w >> 16) & 255u] << 16) | ((unsigned)t[w >> 24] << 24); }

template <bool LUMA, bool CHROMA>
__global__ __launch_bounds__(256) void al_apply_kernel(al_apply_args a) {
    __shared__ unsigned tab[64];
    if (LUMA) {
        if (threadIdx.x < 64) tab[threadIdx.x] = ldg32(a.rec + AL_TAB_AT + threadIdx.x);
        __syncthreads();
    }
    int ou = 0, ov = 0;
    if (CHROMA) { ou = (int)ldg32(a.rec + 9); ov = (int)ldg32(a.rec + 10); }
    const bool chroma = CHROMA && (ou | ov) != 0; // (uniform: the whole launch takes one side)
    if (!LUMA && !chroma) return;
    const int tx = blockIdx.x * 256 + threadIdx.x, per_row = a.W >> 3, rows2 = a.H >> 1;
    if (tx >= per_row * rows2) return;
    const int ry = tx / per_row, cx = tx - ry * per_row, x0 = cx * 8;
    if (2 * ry < a.y0 || 2 * ry >= a.y1 || x0 + 8 <= a.x0 || x0 >= a.x1) return;
    uint8_t *py = a.y + (size_t)(2 * ry) * a.W + x0, *puv = a.uv + (size_t)ry * a.W + x0;
    uint2 s0 = make_uint2(0, 0), s1 = s0, sc = s0;
    if (LUMA) { s0 = ldg64(py); s1 = ldg64(py + a.W); }
    if (chroma) sc = ldg64(puv);
    uint2 o0 = s0, o1 = s1, ouv = sc;
    if (LUMA) {
        const uint8_t *t = (const uint8_t *)tab;
        o0 = make_uint2(al_lut4(t, s0.x), al_lut4(t, s0.y));
        o1 = make_uint2(al_lut4(t, s1.x), al_lut4(t, s1.y));
    }
    if (chroma) {
        ouv.x = csc_pack4(byte_of(sc.x, 0) - ou, byte_of(sc.x, 1) - ov, byte_of(sc.x, 2) - ou, byte_of(sc.x, 3) - ov);
        ouv.y = csc_pack4(byte_of(sc.y, 0) - ou, byte_of(sc.y, 1) - ov, byte_of(sc.y, 2) - ou, byte_of(sc.y, 3) - ov);
    }
    if (x0 < a.x0 || x0 + 8 > a.x1) { // straddles an edge of the picture rectangle: per column pair, corrected inside, the original bytes outside
        unsigned m[2];
#pragma unroll
        for (int k = 0; k < 2; k++) m[k] = (x0 + 4 * k >= a.x0 && x0 + 4 * k < a.x1 ? 0x0000ffffu : 0u) | (x0 + 4 * k + 2 >= a.x0 && x0 + 4 * k + 2 < a.x1 ? 0xffff0000u : 0u);
        o0 = make_uint2((o0.x & m[0]) | (s0.x & ~m[0]), (o0.y & m[1]) | (s0.y & ~m[1]));
        o1 = make_uint2((o1.x & m[0]) | (s1.x & ~m[0]), (o1.y & m[1]) | (s1.y & ~m[1]));
        ouv = make_uint2((ouv.x & m[0]) | (sc.x & ~m[0]), (ouv.y & m[1]) | (sc.y & ~m[1]));
    }
    if (LUMA) { stg64(py, o0); stg64(py + a.W, o1); }
    if (chroma) stg64(puv, ouv);
}

// y, uv, W, H, rect as k_launch_adjust's; luma / chroma: whether the setting's levels / balance are above 0 (one of them is); rec: what the decide launch wrote.
// -1: arguments outside that.
int k_launch_autolevel_apply(uint8_t *y, uint8_t *uv, int W, int H, const int rect[4], int luma, int chroma, const int *rec, hipStream_t s) {
    if (!y || !uv || !rect || !rec || (!luma && !chroma) || W <= 0 || H <= 0 || (W & 7) || (H & 1) || ((((uintptr_t)y) | ((uintptr_t)uv)) & 7)) return -1;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return -1;
    al_apply_args a;
    a.y = y; a.uv = uv; a.W = W; a.H = H; a.x0 = rect[0]; a.x1 = rect[1]; a.y0 = rect[2]; a.y1 = rect[3]; a.rec = rec;
    const dim3 g(((W >> 3) * (H >> 1) + 255) / 256), b(256);
    if (luma && chroma) hipLaunchKernelGGL((al_apply_kernel<true, true>), g, b, 0, s, a);
    else if (luma) hipLaunchKernelGGL((al_apply_kernel<true, false>), g, b, 0, s, a);
    else hipLaunchKernelGGL((al_apply_kernel<false, true>), g, b, 0, s, a);
    return 0;
}
