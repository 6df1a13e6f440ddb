/* san_stab_driver.c -- the stabiliser's rule (stab_host.c) under ASan + UBSan (make san/san_stab; tests/test_stabilize_san_cpu.py): the setting's range
 * edges, projections of planes at every byte step, stride slack and odd size into buffers of exactly their size, votes at n = 4 range and at the ceiling of
 * the sums (the 33-bit cost), the trajectory over the whole state range for every leak edge (negative states: a floor, not a truncation).  Prints a JSON
 * count.  Host code only. */
#include "stab_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355enc.h"

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static long floor_div(long a, long b) { long q = a / b; if ((a % b) && ((a < 0) != (b < 0))) q--; return q; }

int main(void) {
    long bad = 0, edges = 0, planes = 0, votes = 0, steps = 0;
    mi355enc_stabilize_t s;
    mi355enc_stabilize_default(NULL);
    mi355enc_stabilize_default(&s);
    if (s.range != 0 || s.leak != 16 || mi355enc_stabilize_check(&s) || mi355enc_stabilize_check(NULL) != MI355ENC_ERR_ARG) bad++;
    /* every edge of every field, one step inside and one outside (the margins: the odd neighbours are outside too) */
    const int lo[4] = {0, 0, 0, 0}, hi[4] = {32, 255, 1024, 1024};
    for (int i = 0; i < 4; i++)
        for (int e = 0; e < 2; e++)
            for (int d = -2; d <= 2; d++) {
                mi355enc_stabilize_default(&s);
                const int v = (e ? hi[i] : lo[i]) + d;
                int *f = i == 0 ? &s.range : i == 1 ? &s.leak : i == 2 ? &s.margin_x : &s.margin_y;
                *f = v;
                const int ok = v >= lo[i] && v <= hi[i] && (i < 2 || !(v & 1));
                if ((mi355enc_stabilize_check(&s) == MI355ENC_OK) != ok) bad++;
                edges++;
            }
    /* projections: exactly-sized plane and sums; the band sums of an axis add up to the picture's sum */
    for (int n = 0; n < 200; n++) {
        const int w = 1 + (int)(rnd() % 97), h = 1 + (int)(rnd() % 61), step = 1 + (int)(rnd() & 1), slack = (int)(rnd() % 4);
        const int stride = (w - 1) * step + 1 + slack;
        const size_t bytes = (size_t)stride * (h - 1) + (size_t)(w - 1) * step + 1;
        uint8_t *p = (uint8_t *)malloc(bytes);
        uint32_t *sums = (uint32_t *)malloc(4 * (size_t)(w + h) * sizeof *sums);
        if (!p || !sums) return 2;
        for (size_t i = 0; i < bytes; i++) p[i] = (uint8_t)rnd();
        if (mi355enc_stabilize_project(p, stride, step, w, h, sums)) bad++;
        unsigned long total = 0, c = 0, r = 0;
        for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) total += p[(size_t)y * stride + (size_t)x * step];
        for (int i = 0; i < 4 * w; i++) c += sums[i];
        for (int i = 0; i < 4 * h; i++) r += sums[4 * w + i];
        if (c != total || r != total) bad++;
        if (mi355enc_stabilize_project(p, stride - slack - 1, step, w, h, sums) != MI355ENC_ERR_ARG || mi355enc_stabilize_project(p, stride, 3, w, h, sums) != MI355ENC_ERR_ARG) bad++;
        free(p); free(sums);
        planes++;
    }
    /* votes: n = 4 range exactly for every range, a known shift; and the ceiling -- 8192 entries alternating 0 / 2048 * 255 against their complement */
    for (int range = 1; range <= 32; range++) {
        const int n = 4 * range, shift = range > 1 ? (int)(rnd() % (unsigned)(2 * range - 1)) - (range - 1) : 0;
        uint32_t *p = (uint32_t *)malloc((size_t)n * sizeof *p), *q = (uint32_t *)malloc((size_t)n * sizeof *q);
        if (!p || !q) return 2;
        for (int i = 0; i < n; i++) q[i] = rnd() % 522241u;
        for (int i = 0; i < n; i++) p[i] = i - shift >= 0 && i - shift < n ? q[i - shift] : rnd() % 522241u;
        int d = 99;
        const int r = mi355enc_stabilize_vote(p, q, n, range, &d);
        if (r < 0 || (r == 1 && d != shift) || (range > 1 && r != 1)) bad++;
        if (mi355enc_stabilize_vote(p, q, n - 1, range, &d) != MI355ENC_ERR_ARG || mi355enc_stabilize_vote(p, q, n, range + 33, &d) != MI355ENC_ERR_ARG) bad++;
        free(p); free(q);
        votes++;
    }
    {
        const int n = 8192;
        uint32_t *p = (uint32_t *)malloc((size_t)n * sizeof *p), *q = (uint32_t *)malloc((size_t)n * sizeof *q);
        if (!p || !q) return 2;
        for (int i = 0; i < n; i++) { p[i] = (i & 1) ? 2048u * 255u : 0u; q[i] = (i & 1) ? 0u : 2048u * 255u; }
        int d = 99;
        /* even shifts cost (n - 64) * 522240 > 2^32, odd ones 0: a tie of 32 zeros -- no vote */
        if (mi355enc_stabilize_vote(p, q, n, 32, &d) != 0 || d != -31) bad++;
        free(p); free(q);
        votes++;
    }
    /* the trajectory against long arithmetic with an explicit floor, over negative and positive states, every leak edge, one-sided and empty bounds */
    const int leaks[6] = {0, 1, 16, 128, 254, 255};
    const int bl[5] = {0, -16, 0, -1024, -2}, bh[5] = {0, 0, 16, 1024, 6};
    for (int li = 0; li < 6; li++)
        for (int bi = 0; bi < 5; bi++)
            for (int n = 0; n < 2000; n++) {
                const int S = (int)(rnd() % (2u * 256u * 1024u + 1u)) - 256 * 1024, m = (int)(rnd() % 65u) - 32;
                int S2 = 0, o = 0;
                if (mi355enc_stabilize_step(S, m, leaks[li], bl[bi], bh[bi], &S2, &o)) { bad++; continue; }
                long t = floor_div((long)S * (256 - leaks[li]), 256) + 256L * m;
                t = t < 256L * bl[bi] ? 256L * bl[bi] : t > 256L * bh[bi] ? 256L * bh[bi] : t;
                long want = 2 * floor_div(t + 256, 512);
                want = want < bl[bi] ? bl[bi] : want > bh[bi] ? bh[bi] : want;
                if (S2 != t || o != want || (o & 1)) bad++;
                steps++;
            }
    int S2, o, m;
    if (mi355enc_stabilize_step(0, 0, 16, 1, 0, &S2, &o) != MI355ENC_ERR_ARG || mi355enc_stabilize_step(0, 0, 256, 0, 0, &S2, &o) != MI355ENC_ERR_ARG) bad++;
    const int v4[4] = {5, -3, 7, 0};
    if (mi355enc_stabilize_motion(v4, 4, &m) || m != 0 || mi355enc_stabilize_motion(v4, 3, &m) || m != 5 || mi355enc_stabilize_motion(NULL, 0, &m) || m != 0 ||
        mi355enc_stabilize_motion(v4, 5, &m) != MI355ENC_ERR_ARG) bad++;
    printf("{\"bad\": %ld, \"edges\": %ld, \"planes\": %ld, \"votes\": %ld, \"steps\": %ld}\n", bad, edges, planes, votes, steps);
    return bad ? 1 : 0;
}
