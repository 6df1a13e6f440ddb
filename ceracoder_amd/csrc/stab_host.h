/* stab_host.h -- the electronic image stabiliser's rule in plain C, all integers: what the host entry points of the ABI
 * (mi355enc_stabilize_*), the handle (enc_stab.cpp) and the match kernel (k_stab.hip) share.  No device needed. */
#ifndef MI355_STAB_HOST_H
#define MI355_STAB_HOST_H
#include <stdint.h>

#define STAB_BANDS 4      /* bands per axis */
#define STAB_RANGE_MAX 32 /* = MI355ENC_STABILIZE_RANGE_MAX */
#define STAB_REC_WORDS 8  /* a record: mx, my, votes_x, votes_y, ox, oy, Sx, Sy */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STAB_FN static __host__ __device__ inline
#else
#define STAB_FN static inline
#endif

/* v >> s with the shift arithmetic (floor), whatever the compiler makes of a negative left operand */
STAB_FN int stab_floor_shr(int v, int s) { return v >= 0 ? v >> s : -((-v + (1 << s) - 1) >> s); }
STAB_FN int stab_clip(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
/* first row (column) of band k of n rows */
STAB_FN int stab_band(int k, int n) { return (int)((long long)k * n / STAB_BANDS); }
/* the bounds of an axis: the crop of `size` at `origin` inside `input`, the margin; both even, towards zero */
STAB_FN void stab_bounds(int margin, int origin, int size, int input, int *lo, int *hi) {
    const int a = margin < origin ? margin : origin, room = input - origin - size, b = margin < room ? margin : room;
    *lo = -((a > 0 ? a : 0) & ~1);
    *hi = (b > 0 ? b : 0) & ~1;
}
/* the lower median of count (0 .. 4) votes: sorted v[(count - 1) / 2]; 0 with none.  v is sorted in place */
STAB_FN int stab_median(int *v, int count) {
    for (int i = 1; i < count; i++)
        for (int j = i; j > 0 && v[j - 1] > v[j]; j--) { const int t = v[j]; v[j] = v[j - 1]; v[j - 1] = t; }
    return count > 0 ? v[(count - 1) / 2] : 0;
}
/* one trajectory step of an axis: the state S (1/256 sample) and the offset o that follow from motion m under bounds [lo, hi] */
STAB_FN void stab_step(int S, int m, int leak, int lo, int hi, int *S_out, int *o) {
    S = stab_floor_shr(S * (256 - leak), 8) + 256 * m;
    S = stab_clip(S, 256 * lo, 256 * hi);
    *S_out = S;
    *o = stab_clip(2 * stab_floor_shr(S + 256, 9), lo, hi);
}
#endif
