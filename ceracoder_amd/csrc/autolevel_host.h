/* autolevel_host.h -- the rule of automatic levels and white balance in plain C, all integers: what the host entry points of the ABI
 * (mi355enc_autolevel_*), the handle (enc_autolevel.cpp) and the decide kernel (k_autolevel.hip) share.  No device needed. */
#ifndef MI355_AUTOLEVEL_HOST_H
#define MI355_AUTOLEVEL_HOST_H
#include <stdint.h>

#define AL_REC_WORDS 12    /* a record: lo, hi, voters, du, dv, Lo, Hi, Du, Dv, off_u, off_v, valid */
#define AL_SLAB_WORDS 260  /* a workgroup's slab: 256 counts, then n, su, sv and a word of room */
#define AL_SLABS_MAX 256   /* one workgroup per compute unit */
#define AL_TAB_AT 16       /* a slot's block: the record, room up to word 16, then the table's 64 words */
#define AL_SLOT_WORDS 80

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AL_FN static __host__ __device__ inline
#else
#define AL_FN static inline
#endif

/* v >> s and a / b as floors, whatever the compiler makes of a negative left operand (b > 0) */
AL_FN int al_floor_shr(int v, int s) { return v >= 0 ? v >> s : -((-v + (1 << s) - 1) >> s); }
AL_FN int al_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
AL_FN int al_clip(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
/* black level and scale of the output range */
AL_FN int al_black(int full_range) { return full_range ? 0 : 16; }
AL_FN int al_scale(int full_range) { return full_range ? 255 : 219; }
/* the luma bounds of a chroma vote */
AL_FN int al_vote_lo(int B, int S) { return B + (S >> 3); }
AL_FN int al_vote_hi(int B, int S) { return B + S - (S >> 3); }
/* NC: the chroma samples whose co-sited luma lies in the visible part of rect {x0, x1, y0, y1} (x0, y0 even) of a picture of vw x vh */
AL_FN uint32_t al_chroma_count(const int *rect, int vw, int vh) {
    const int x1 = rect[1] < vw ? rect[1] : vw, y1 = rect[3] < vh ? rect[3] : vh;
    return x1 > rect[0] && y1 > rect[2] ? (uint32_t)((x1 - rect[0] + 1) >> 1) * (uint32_t)((y1 - rect[2] + 1) >> 1) : 0u;
}
/* whether code v is at or above the black point / at or below the white point: cum = the inclusive prefix sum at v, below = cum(v - 1) */
AL_FN int al_is_lo(uint64_t cum, uint64_t N, int clip_low) { return 10000u * cum > (uint64_t)clip_low * N; }
AL_FN int al_is_hi(uint64_t below, uint64_t N, int clip_high) { return 10000u * (N - below) > (uint64_t)clip_high * N; }
/* one step of a state word towards the measurement m256 (1/256 code) */
AL_FN int al_follow(int X, int m256, int speed) { return X + al_floor_shr((m256 - X) * speed, 8); }

/* what the table is made from */
typedef struct { int L, span; } al_interval_t;

/* A picture's decision from its measurement: lo / hi the black and white point found in the histogram (255 / 0 where no code qualifies; clipped here), n, su, sv
 * the chroma vote, NC the visible chroma samples.  set: levels, balance, speed, clip_low, clip_high, max_gain, reach (checked).  st: Lo, Hi, Du, Dv, stepped in
 * place (prime: set).  rec: AL_REC_WORDS words.  Returns the interval of the table. */
AL_FN al_interval_t al_decide(int lo, int hi, uint32_t n, uint64_t su, uint64_t sv, uint32_t NC, const int *set, int B, int S, int prime, int *st, int *rec) {
    const int levels = set[0], balance = set[1], speed = set[2], max_gain = set[5];
    const int b256 = 256 * B, t256 = 256 * (B + S);
    lo = al_clip(lo, B, B + S); hi = al_clip(hi, B, B + S);
    const int valid = n > 0 && 16ull * n >= NC;
    const int du = valid ? (int)((256ull * su) / n) - 32768 : 0, dv = valid ? (int)((256ull * sv) / n) - 32768 : 0;
    if (prime) { st[0] = 256 * lo; st[1] = 256 * hi; st[2] = du; st[3] = dv; }
    else {
        st[0] = al_follow(st[0], 256 * lo, speed); st[1] = al_follow(st[1], 256 * hi, speed);
        if (valid) { st[2] = al_follow(st[2], du, speed); st[3] = al_follow(st[3], dv, speed); }
    }
    /* (a state from another output range, or from a caller: back into this one's) */
    st[0] = al_clip(st[0], b256, t256); st[1] = al_clip(st[1], b256, t256);
    int L = b256 + ((st[0] - b256) * levels) / 1000, T = t256 - ((t256 - st[1]) * levels) / 1000;
    int span = T - L;
    const int smin = (256000 * S + max_gain - 1) / max_gain;
    if (span < smin) {
        L = al_floor_shr(L + T, 1) - (smin >> 1); T = L + smin;
        if (L < b256) { L = b256; T = L + smin; }
        if (T > t256) { T = t256; L = T - smin; }
        span = smin;
    }
    rec[0] = lo; rec[1] = hi; rec[2] = (int)n; rec[3] = du; rec[4] = dv;
    rec[5] = st[0]; rec[6] = st[1]; rec[7] = st[2]; rec[8] = st[3];
    rec[9] = al_floor_div(st[2] * balance + 128000, 256000); rec[10] = al_floor_div(st[3] * balance + 128000, 256000);
    rec[11] = valid;
    al_interval_t iv; iv.L = L; iv.span = span;
    return iv;
}
/* entry v of the table */
AL_FN int al_table(int v, al_interval_t iv, int B, int S) {
    const int t = al_clip(256 * v - iv.L, 0, iv.span);
    return B + (2 * t * S + iv.span) / (2 * iv.span);
}
#endif
