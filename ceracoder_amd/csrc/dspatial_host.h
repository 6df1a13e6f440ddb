/* dspatial_host.h -- the rule of the spatial noise filter and its noise estimate in plain C, all integers: what the host entry points of
 * the ABI (mi355enc_denoise_spatial_*), the handle (enc_dspatial.cpp) and the kernels (k_dspatial.hip) share.  No device needed. */
#ifndef MI355_DSPATIAL_HOST_H
#define MI355_DSPATIAL_HOST_H
#include <stdint.h>

#define DS_MAX 32          /* the largest strength */
#define DS_REC_WORDS 8     /* a record: candidates, voters, v, valid, X, s_luma, s_chroma and a word of room */
#define DS_SLAB_WORDS 256  /* a workgroup's slab: the 256 counts of its histogram */
#define DS_SLABS_MAX 256   /* one workgroup per compute unit */
#define DS_X_MAX 65280     /* the state's ceiling: bin 255 in 1/256 bin */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DS_FN static __host__ __device__ inline
#else
#define DS_FN static inline
#endif

/* v >> s as a floor, whatever the compiler makes of a negative left operand */
DS_FN int ds_floor_shr(int v, int s) { return v >= 0 ? v >> s : -((-v + (1 << s) - 1) >> s); }
/* R_s[a] = clip(0, 16, floor(16 (3 s - a) / (2 s))), s > 0: 16 up to a = s, 0 from 3 s on; R_0 = 0 */
DS_FN int ds_weight(int s, int a) {
    if (s <= 0) return 0;
    const int n = 16 * (3 * s - a), d = 2 * s, q = n >= 0 ? n / d : -((-n + d - 1) / d);
    return q < 0 ? 0 : q > 16 ? 16 : q;
}
/* black level and scale of the output range, and the bounds of a block's sample sum that lets it vote */
DS_FN int ds_black(int full_range) { return full_range ? 0 : 16; }
DS_FN int ds_scale(int full_range) { return full_range ? 255 : 219; }
DS_FN int ds_vote_lo(int B, int S) { return 64 * (B + (S >> 4)); }
DS_FN int ds_vote_hi(int B, int S) { return 64 * (B + S - (S >> 4)); }
/* a block's bin from A, the sum of |L| over its 36 interior samples: Immerkaer's sigma in eighths of a code */
DS_FN int ds_bin(int A) { const int b = (95 * A + 1024) >> 11; return b > 255 ? 255 : b; }
/* the candidates: the aligned 8 x 8 blocks wholly inside the visible part of rect {x0, x1, y0, y1} of a picture of vw x vh -- first block column, their count
 * per row, first block row, their rows (counts 0 where there is none) */
DS_FN void ds_blocks(const int *rect, int vw, int vh, int *bx0, int *bcols, int *by0, int *brows) {
    const int x1 = rect[1] < vw ? rect[1] : vw, y1 = rect[3] < vh ? rect[3] : vh;
    *bx0 = (rect[0] + 7) >> 3; *by0 = (rect[2] + 7) >> 3;
    *bcols = (x1 >> 3) - *bx0; *brows = (y1 >> 3) - *by0;
    if (*bcols < 0) *bcols = 0;
    if (*brows < 0) *brows = 0;
}
/* whether bin v is at or above the percentile: cum = the inclusive prefix sum at v */
DS_FN int ds_is_v(uint64_t cum, uint64_t N, int percentile) { return 100u * cum >= (uint64_t)percentile * N; }

/* A picture's decision: NC candidates, N voters, v the percentile's bin.  set: luma, chroma, auto_gain, percentile, speed (checked, auto_gain > 0).  *X: the
 * state in 1/256 bin, stepped in place (prime: set).  rec: DS_REC_WORDS words. */
DS_FN void ds_decide(uint32_t NC, uint32_t N, int v, const int *set, int prime, int *X, int *rec) {
    const int valid = N > 0 && 16ull * N >= NC;
    int x = *X;
    if (prime) x = valid ? 256 * v : 0;
    else if (valid) x += ds_floor_shr((256 * v - x) * set[4], 8);
    x = x < 0 ? 0 : x > DS_X_MAX ? DS_X_MAX : x; /* (a no-op on a state this rule made) */
    const int s = (int)(((int64_t)x * set[2] + 1024000) / 2048000);
    *X = x;
    rec[0] = (int)NC; rec[1] = (int)N; rec[2] = v; rec[3] = valid; rec[4] = x;
    rec[5] = set[0] < s ? set[0] : s; rec[6] = set[1] < s ? set[1] : s; rec[7] = 0;
}
#endif
