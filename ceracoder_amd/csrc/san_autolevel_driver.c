/* san_autolevel_driver.c -- the rule of automatic levels and white balance (autolevel_host.c) under ASan + UBSan (make san/san_autolevel;
 * tests/test_autolevel_san_cpu.py): every range edge of the setting, one step inside and one outside; decisions at every range edge of every field and at the
 * ceilings of the measurement (2^26 samples in one bin, 2^24 voters of 255, states at the ends of their ranges with every speed edge), into a state, a record
 * and a table of exactly their size on the heap; and seeded decisions checked for what the rule promises.  Prints a JSON count.  Host code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355enc.h"

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static const int LO[7] = {0, 0, 1, 0, 0, 1000, 0}, HI[7] = {1000, 1000, 256, 2000, 2000, 8000, 127};
static int *field(mi355enc_autolevel_t *a, int i) {
    return i == 0 ? &a->levels : i == 1 ? &a->balance : i == 2 ? &a->speed : i == 3 ? &a->clip_low : i == 4 ? &a->clip_high : i == 5 ? &a->max_gain : &a->reach;
}

/* one decision into exactly-sized heap buffers; returns the code, counts what the rule promises as bad */
static int decide(const mi355enc_autolevel_meas_t *m, const mi355enc_autolevel_t *a, int full, int prime, const int32_t st_in[4], long *bad) {
    mi355enc_autolevel_meas_t *mm = (mi355enc_autolevel_meas_t *)malloc(sizeof *mm);
    int32_t *st = (int32_t *)malloc(4 * sizeof *st);
    mi355enc_autolevel_info_t *info = (mi355enc_autolevel_info_t *)malloc(sizeof *info);
    uint8_t *table = (uint8_t *)malloc(256);
    if (!mm || !st || !info || !table) exit(2);
    *mm = *m;
    memcpy(st, st_in, 4 * sizeof *st);
    const int r = mi355enc_autolevel_decide(mm, a, full, prime, st, info, table);
    if (r == MI355ENC_OK) {
        const int B = full ? 0 : 16, S = full ? 255 : 219;
        if (table[0] < B || table[255] > B + S) (*bad)++;
        for (int v = 1; v < 256; v++) if (table[v] < table[v - 1]) { (*bad)++; break; }
        if (info->lo < B || info->lo > B + S || info->hi < B || info->hi > B + S) (*bad)++;
        if (st[0] != info->s_lo || st[1] != info->s_hi || st[2] != info->s_du || st[3] != info->s_dv) (*bad)++;
        if (st[0] < 256 * B || st[0] > 256 * (B + S) || st[1] < 256 * B || st[1] > 256 * (B + S) || st[2] < -32768 || st[2] > 32767 || st[3] < -32768 || st[3] > 32767) (*bad)++;
        if (info->off_u < -128 || info->off_u > 128 || info->off_v < -128 || info->off_v > 128) (*bad)++;
        if (a->speed == 256 && info->valid && (info->s_du != info->du || info->s_dv != info->dv)) (*bad)++;
    }
    free(mm); free(st); free(info); free(table);
    return r;
}

int main(void) {
    long bad = 0, edges = 0, refused = 0, decisions = 0, sets = 0;
    mi355enc_autolevel_t a;
    mi355enc_autolevel_default(NULL);
    mi355enc_autolevel_default(&a);
    if (a.levels != 0 || a.balance != 0 || a.speed != 16 || a.clip_low != 50 || a.clip_high != 50 || a.max_gain != 2000 || a.reach != 48) bad++;
    if (mi355enc_autolevel_check(&a) || mi355enc_autolevel_check(NULL) != MI355ENC_ERR_ARG) bad++;
    /* the ceilings of a measurement: all of 2^26 samples in one bin at either end, 2^24 chroma samples that all vote with 255 */
    mi355enc_autolevel_meas_t top, low;
    memset(&top, 0, sizeof top); memset(&low, 0, sizeof low);
    top.hist[255] = 1u << 26; top.chroma = 1u << 24; top.voters = 1u << 24; top.su = 255ull << 24; top.sv = 255ull << 24;
    low.hist[0] = 1u << 26; low.chroma = 1u << 24; low.voters = 1u << 20; /* (16 n == NC exactly; su = sv = 0) */
    const int32_t ends[4][4] = {{0, 0, -32768, -32768}, {65280, 65280, 32767, 32767}, {65280, 0, -32768, 32767}, {0, 65280, 32767, -32768}};
    /* every edge of every field, one step inside and one outside: the check, and a decision at both ceilings from every end of the state */
    for (int i = 0; i < 7; i++)
        for (int e = 0; e < 2; e++)
            for (int d = -1; d <= 1; d++) {
                mi355enc_autolevel_default(&a);
                a.levels = 1000; a.balance = 1000;
                const int v = (e ? HI[i] : LO[i]) + d, ok = v >= LO[i] && v <= HI[i];
                *field(&a, i) = v;
                if ((mi355enc_autolevel_check(&a) == MI355ENC_OK) != ok) bad++;
                edges++;
                for (int full = 0; full < 2; full++)
                    for (int k = 0; k < 4; k++)
                        for (int prime = 0; prime < 2; prime++) {
                            const int r1 = decide(&top, &a, full, prime, ends[k], &bad), r2 = decide(&low, &a, full, prime, ends[k], &bad);
                            if ((r1 == MI355ENC_OK) != ok || (r2 == MI355ENC_OK) != ok) bad++;
                            if (!ok) refused += 2; else decisions += 2;
                        }
            }
    /* what the decision refuses: null pointers, a measurement or a state outside the rule */
    {
        int32_t st[4] = {0, 0, 0, 0};
        mi355enc_autolevel_info_t info;
        uint8_t table[256];
        mi355enc_autolevel_default(&a);
        a.levels = 500;
        mi355enc_autolevel_meas_t m = low;
        if (mi355enc_autolevel_decide(NULL, &a, 0, 1, st, &info, table) != MI355ENC_ERR_ARG || mi355enc_autolevel_decide(&m, NULL, 0, 1, st, &info, table) != MI355ENC_ERR_ARG ||
            mi355enc_autolevel_decide(&m, &a, 0, 1, NULL, &info, table) != MI355ENC_ERR_ARG || mi355enc_autolevel_decide(&m, &a, 0, 1, st, NULL, table) != MI355ENC_ERR_ARG ||
            mi355enc_autolevel_decide(&m, &a, 0, 1, st, &info, NULL) != MI355ENC_ERR_ARG) bad++;
        m = low; m.hist[1] = 1; if (mi355enc_autolevel_decide(&m, &a, 0, 1, st, &info, table) != MI355ENC_ERR_ARG) bad++; /* 2^26 + 1 samples */
        m = low; m.chroma = (1u << 24) + 1; if (mi355enc_autolevel_decide(&m, &a, 0, 1, st, &info, table) != MI355ENC_ERR_ARG) bad++;
        m = low; m.voters = m.chroma + 1; if (mi355enc_autolevel_decide(&m, &a, 0, 1, st, &info, table) != MI355ENC_ERR_ARG) bad++;
        m = low; m.su = 255ull * m.voters + 1; if (mi355enc_autolevel_decide(&m, &a, 0, 1, st, &info, table) != MI355ENC_ERR_ARG) bad++;
        m = low; m.sv = ~0ull; if (mi355enc_autolevel_decide(&m, &a, 0, 1, st, &info, table) != MI355ENC_ERR_ARG) bad++;
        const int32_t outside[8][4] = {{-1, 0, 0, 0}, {65281, 0, 0, 0}, {0, -1, 0, 0}, {0, 65281, 0, 0}, {0, 0, -32769, 0}, {0, 0, 32768, 0}, {0, 0, 0, -32769}, {0, 0, 0, 32768}};
        for (int k = 0; k < 8; k++) {
            memcpy(st, outside[k], sizeof st);
            if (mi355enc_autolevel_decide(&low, &a, 0, 0, st, &info, table) != MI355ENC_ERR_ARG) bad++;
            refused++;
        }
        refused += 10;
    }
    /* seeded: any histogram, any setting, any state */
    for (int n = 0; n < 4000; n++) {
        mi355enc_autolevel_meas_t m;
        memset(&m, 0, sizeof m);
        const int kind = (int)(rnd() % 3u);
        if (kind == 0) for (int v = 0; v < 256; v++) m.hist[v] = rnd() % 200000u;
        else if (kind == 1) for (int k = 0; k < 3; k++) m.hist[rnd() & 255u] += rnd() % 1000000u;
        else m.hist[rnd() & 255u] = 1u + rnd() % 1000u;
        m.chroma = 1u + rnd() % (1u << 24);
        m.voters = rnd() % (m.chroma + 1u);
        if (rnd() & 1u) m.voters /= 17u;
        m.su = m.voters ? (uint64_t)rnd() % (255ull * m.voters + 1) : 0; m.sv = m.voters ? (uint64_t)rnd() % (255ull * m.voters + 1) : 0;
        for (int i = 0; i < 7; i++) *field(&a, i) = LO[i] + (int)(rnd() % (unsigned)(HI[i] - LO[i] + 1));
        const int32_t st[4] = {(int32_t)(rnd() % 65281u), (int32_t)(rnd() % 65281u), (int32_t)(rnd() % 65536u) - 32768, (int32_t)(rnd() % 65536u) - 32768};
        if (decide(&m, &a, (int)(rnd() & 1u), (rnd() & 3u) == 0, st, &bad)) bad++;
        sets++;
    }
    printf("{\"bad\": %ld, \"edges\": %ld, \"refused\": %ld, \"decisions\": %ld, \"sets\": %ld}\n", bad, edges, refused, decisions, sets);
    return bad ? 1 : 0;
}
