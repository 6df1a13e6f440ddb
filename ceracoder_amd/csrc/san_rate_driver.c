/* san_rate_driver.c -- the rule of the frame-rate conversion (rate_host.c) under ASan + UBSan, stand-alone (Makefile: san/san_rate): the plan over seeded pts
 * sequences -- anchors near +-2^62, pts_per_second from 1 to 10^9, rates from 1/1 to 240000/1001, jitter, holes and backward steps, both modes, every max_fill.
 * Checks what must hold whatever the input: the count stays within 0 .. max_fill + 1, the pts of the pictures never decrease between resyncs, weights stay in
 * 0 .. 256.  Prints the counts as JSON; exit status 1 when a check fails. */
#include <stdint.h>
#include <stdio.h>

#include "rate_host.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng(void) { /* xorshift64* */
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

int main(void) {
    static const int64_t pps_tab[] = {1, 25, 1000, 90000, 1000000, 1000000000};
    static const int fps_tab[][2] = {{1, 1}, {24000, 1001}, {25, 1}, {30000, 1001}, {30, 1}, {50, 1}, {60, 1}, {7013, 234}, {240000, 1001}};
    unsigned long long sequences = 0, in = 0, out = 0, dropped = 0, multi = 0, blended = 0, resyncs = 0, bad = 0;
    for (int seq = 0; seq < 3000; seq++) {
        const int64_t pps = pps_tab[rng() % 6];
        const int *fo = fps_tab[rng() % 9], *fi = fps_tab[rng() % 9];
        const int mode = 1 + (int)(rng() % 2), max_fill = (int)(rng() % MI355ENC_RATE_MAX_OUT);
        const int where = (int)(rng() % 4);
        const int64_t big = (int64_t)1 << 62;
        int64_t base = where == 0 ? 0 : where == 1 ? big - 5000 : where == 2 ? -big + 5000 : (int64_t)(rng() % 1000000);
        mi355enc_rate_plan_t pl;
        mi355enc_rate_plan_init(&pl, mode, pps, fo[0], fo[1], max_fill, 0, -1);
        const int64_t step = pps * fi[1] / fi[0]; /* the input's period, truncated (0 at pps 1: every input at the same instant) */
        int64_t last_out = 0;
        int have_out = 0;
        /* near +-2^62 the sequence stays short enough never to leave the range of int64 */
        const int len = 40 + (int)(rng() % 60);
        for (int i = 0; i < len; i++) {
            int64_t p = base + (int64_t)i * step;
            const unsigned ev = (unsigned)(rng() % 32);
            if (step > 4 && ev < 8) p += (int64_t)(rng() % (uint64_t)(step / 2)) - step / 4; /* jitter */
            if (ev == 8 && where == 0) base += step * (int64_t)(rng() % 50);                  /* a hole */
            if (ev == 9 && where != 2) base -= step * (int64_t)(rng() % 5);                   /* a backward step */
            int n = -1, rs = -1, w[MI355ENC_RATE_MAX_OUT];
            int64_t t[MI355ENC_RATE_MAX_OUT];
            if (mi355enc_rate_plan_step(&pl, p, &n, t, w, &rs) != MI355ENC_OK) { bad++; continue; }
            if (n < 0 || n > max_fill + 1 || (rs && n != 1)) { bad++; continue; }
            if (rs) have_out = 0;
            for (int k = 0; k < n; k++) {
                if (w[k] < 0 || w[k] > 256) bad++;
                if (have_out && t[k] < last_out) bad++;
                last_out = t[k]; have_out = 1;
                blended += w[k] > 0 && w[k] < 256;
            }
            in++; out += (unsigned)n; dropped += n == 0; multi += n > 1; resyncs += (unsigned)rs;
        }
        sequences++;
    }
    /* the argument checks */
    {
        mi355enc_rate_t r = {1, 90000, 2};
        int n, rs, w[MI355ENC_RATE_MAX_OUT];
        int64_t t[MI355ENC_RATE_MAX_OUT];
        mi355enc_rate_plan_t pl;
        mi355enc_rate_plan_init(&pl, 2, 90000, 30, 1, 99, 0, -1);
        bad += mi355enc_rate_check(&r) != MI355ENC_OK || mi355enc_rate_check(0) != MI355ENC_ERR_ARG || pl.max_fill != MI355ENC_RATE_MAX_OUT - 1;
        bad += mi355enc_rate_plan_step(0, 0, &n, t, w, &rs) != MI355ENC_ERR_ARG || mi355enc_rate_plan_step(&pl, 0, 0, t, w, &rs) != MI355ENC_ERR_ARG;
        mi355enc_rate_plan_init(0, 1, 1, 1, 1, 0, 0, -1);
    }
    printf("{\"sequences\": %llu, \"in\": %llu, \"out\": %llu, \"dropped\": %llu, \"multi\": %llu, \"blended\": %llu, \"resyncs\": %llu, \"bad\": %llu}\n",
           sequences, in, out, dropped, multi, blended, resyncs, bad);
    return bad ? 1 : 0;
}
