/* san_roi_driver.c -- the host side of region-of-interest quantisation (roi_host.c) under ASan + UBSan (make san/san_roi; tests/test_roi_san_cpu.py): the check
 * at both edges of every field's range and one step outside; the map -- into a heap buffer of exactly mbw mbh bytes, the caller's map from one of exactly that
 * size -- with every field at its edges, with rectangles beyond every picture edge, at 1 x 1 and 512 x 512 macroblocks, and over seeded random
 * configurations; the parser on its own strings, on every truncation of one and on junk.  Prints a JSON line with an FNV-1a checksum over every map it made
 * (bytes, then active and background), which tests/roiref.py reproduces from the same seed.  Host code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355enc.h"

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static uint32_t fnv = 2166136261u;
static void mix(unsigned b) { fnv = (fnv ^ (b & 255u)) * 16777619u; }
static long maps = 0, bad = 0;

/* one map into exactly mbw mbh bytes; user: 0 none, 1 seeded noise of -12 .. +12 from exactly mbw mbh bytes */
static void one_map(const mi355enc_roi_t *cfg, int mbw, int mbh, int with_user) {
    const size_t n = (size_t)mbw * mbh;
    int8_t *out = (int8_t *)malloc(n), *user = with_user ? (int8_t *)malloc(n) : NULL;
    if (!out || (with_user && !user)) exit(2);
    for (size_t m = 0; user && m < n; m++) user[m] = (int8_t)rnd_in(-12, 12);
    int active = -1, bg = -1;
    if (mi355enc_roi_map(cfg, user, mbw, mbh, out, &active, &bg) != MI355ENC_OK) bad++;
    for (size_t m = 0; m < n; m++) { mix((unsigned)out[m]); if (out[m] < -12 || out[m] > 12) bad++; }
    mix((unsigned)active); mix((unsigned)bg);
    if (user) { /* one value outside: refused */
        user[n - 1] = 13;
        if (mi355enc_roi_map(cfg, user, mbw, mbh, out, NULL, NULL) != MI355ENC_ERR_ARG) bad++;
        user[n - 1] = -13;
        if (mi355enc_roi_map(cfg, user, mbw, mbh, out, NULL, NULL) != MI355ENC_ERR_ARG) bad++;
    }
    maps++;
    free(out); free(user);
}

static mi355enc_roi_t base(void) {
    mi355enc_roi_t c;
    mi355enc_roi_default(&c);
    c.n_rects = 1; c.balance = 6;
    c.rect[0].x = 16; c.rect[0].y = 16; c.rect[0].w = 40; c.rect[0].h = 20; c.rect[0].delta = -6; c.rect[0].feather = 2;
    return c;
}

int main(void) {
    long checks = 0, parses = 0;
    /* every field: lo - 1 and hi + 1 are refused, lo and hi accepted and mapped (delta: 0 is refused as well) */
    static const int lo[8] = {0, -65536, -65536, 1, 1, -12, 0, 0}, hi[8] = {8, 65536, 65536, 65536, 65536, 12, 8, 12};
    for (int f = 0; f < 8; f++)
        for (int k = 0; k < 4; k++) {
            mi355enc_roi_t c = base();
            const int v = k == 0 ? lo[f] - 1 : k == 1 ? lo[f] : k == 2 ? hi[f] : hi[f] + 1;
            int *field = f == 0 ? &c.n_rects : f == 1 ? &c.rect[0].x : f == 2 ? &c.rect[0].y : f == 3 ? &c.rect[0].w : f == 4 ? &c.rect[0].h : f == 5 ? &c.rect[0].delta :
                         f == 6 ? &c.rect[0].feather : &c.balance;
            *field = v;
            if (f == 0 && v == 8) for (int j = 1; j < 8; j++) { c.rect[j] = c.rect[0]; c.rect[j].x += 16 * j; c.rect[j].delta = j & 1 ? 5 : -5; }
            const int want = (k == 0 || k == 3) ? MI355ENC_ERR_ARG : MI355ENC_OK;
            if (mi355enc_roi_check(&c) != want) bad++;
            checks++;
            if (want == MI355ENC_OK) { one_map(&c, 5, 3, 0); one_map(&c, 21, 12, 1); }
            else { int8_t o[15]; if (mi355enc_roi_map(&c, NULL, 5, 3, o, NULL, NULL) != MI355ENC_ERR_ARG) bad++; }
        }
    { mi355enc_roi_t c = base(); c.rect[0].delta = 0; if (mi355enc_roi_check(&c) != MI355ENC_ERR_ARG) bad++; checks++; }
    if (mi355enc_roi_check(NULL) != MI355ENC_ERR_ARG) bad++;
    /* rectangles beyond every picture edge (21 x 12 macroblocks: 336 x 192 samples), partly and wholly, with the feather reaching back in */
    static const int beyond[12][4] = {{-40, 40, 60, 60}, {-100, 40, 100, 60}, {-100, 40, 99, 60}, {300, 40, 100, 60}, {336, 40, 100, 60}, {335, 40, 1, 60},
                                      {40, -30, 60, 50}, {40, -50, 60, 50}, {40, 170, 60, 50}, {40, 192, 60, 50}, {-65536, -65536, 65536, 65536}, {-65535, -65535, 65536, 65536}};
    for (int i = 0; i < 12; i++)
        for (int fe = 0; fe <= 8; fe += 4) {
            mi355enc_roi_t c = base();
            c.rect[0].x = beyond[i][0]; c.rect[0].y = beyond[i][1]; c.rect[0].w = beyond[i][2]; c.rect[0].h = beyond[i][3]; c.rect[0].feather = fe;
            c.rect[0].delta = i & 1 ? 12 : -12;
            one_map(&c, 21, 12, 0);
        }
    /* the smallest and the largest picture */
    { mi355enc_roi_t c = base(); one_map(&c, 1, 1, 0); one_map(&c, 1, 1, 1); one_map(NULL, 1, 1, 1); }
    {
        mi355enc_roi_t c = base();
        c.n_rects = 2; c.balance = 12;
        c.rect[0].x = 1000; c.rect[0].y = 2000; c.rect[0].w = 3000; c.rect[0].h = 1500; c.rect[0].delta = -12; c.rect[0].feather = 8;
        c.rect[1].x = 8000; c.rect[1].y = 8100; c.rect[1].w = 65536; c.rect[1].h = 65536; c.rect[1].delta = 7; c.rect[1].feather = 3;
        one_map(&c, 512, 512, 0); one_map(&c, 512, 512, 1); one_map(NULL, 512, 512, 0);
    }
    { int8_t o[1]; if (mi355enc_roi_map(NULL, NULL, 0, 1, o, NULL, NULL) != MI355ENC_ERR_ARG || mi355enc_roi_map(NULL, NULL, 1, 513, o, NULL, NULL) != MI355ENC_ERR_ARG || mi355enc_roi_map(NULL, NULL, 1, 1, NULL, NULL, NULL) != MI355ENC_ERR_ARG) bad++; }
    /* seeded random configurations */
    static const int sizes[5][2] = {{1, 1}, {4, 3}, {5, 3}, {21, 12}, {45, 25}};
    for (int i = 0; i < 200; i++) {
        const int mbw = sizes[i % 5][0], mbh = sizes[i % 5][1];
        mi355enc_roi_t c;
        mi355enc_roi_default(&c);
        c.n_rects = rnd_in(0, 8); c.balance = rnd_in(0, 12);
        for (int k = 0; k < c.n_rects; k++) {
            mi355enc_roi_rect_t *r = &c.rect[k];
            r->x = rnd_in(-64, 16 * mbw + 32); r->y = rnd_in(-64, 16 * mbh + 32); r->w = rnd_in(1, 16 * mbw + 64); r->h = rnd_in(1, 16 * mbh + 64);
            r->delta = rnd_in(1, 12); if (rnd() & 1) r->delta = -r->delta;
            r->feather = rnd_in(0, 8);
        }
        one_map(&c, mbw, mbh, (int)(rnd() & 1));
    }
    /* the parser: its own strings round-trip, every truncation of one is parsed or refused (and a refusal leaves the output alone), junk is refused */
    {
        static const char *good = "16,32,640,360,-6,2;-20,0,64,64,12;1000,1000,1,1,-1,8";
        mi355enc_roi_t c;
        mi355enc_roi_default(&c);
        c.balance = 5;
        if (mi355enc_roi_parse(good, &c) != MI355ENC_OK || c.n_rects != 3 || c.balance != 5 || c.rect[0].delta != -6 || c.rect[0].feather != 2 || c.rect[1].x != -20 ||
            c.rect[1].feather != 0 || c.rect[2].feather != 8)
            bad++;
        parses++;
        const size_t len = strlen(good);
        for (size_t k = 0; k <= len; k++) {
            char *copy = (char *)malloc(k + 1); /* exactly its length and the terminator */
            if (!copy) return 2;
            memcpy(copy, good, k); copy[k] = 0;
            mi355enc_roi_t t, before;
            memset(&t, 0x5a, sizeof t); t.balance = 3; before = t;
            const int r = mi355enc_roi_parse(copy, &t);
            if (r == MI355ENC_OK) { if (mi355enc_roi_check(&t) || t.balance != 3) bad++; }
            else if (r != MI355ENC_ERR_ARG || memcmp(&t, &before, sizeof t)) bad++;
            parses++;
            free(copy);
        }
        static const char *junk[] = {"x", "1,2,3,4", "1,2,3,4,0", "1,2,3,4,13", "1,2,3,4,5,9", "1,2,3,4,5,6,7", "1,2,3,4,5;", ";1,2,3,4,5", "1,2,3,4,5;;1,2,3,4,5", "1,,3,4,5",
                                     "1,2,0,4,5", "1 2,3,4,5,6", "1,2,3,4,5x", "99999999999999999999,2,3,4,5", "1,2,3,4,-", "1.5,2,3,4,5",
                                     "1,1,1,1,1;1,1,1,1,1;1,1,1,1,1;1,1,1,1,1;1,1,1,1,1;1,1,1,1,1;1,1,1,1,1;1,1,1,1,1;1,1,1,1,1"};
        for (size_t i = 0; i < sizeof junk / sizeof junk[0]; i++) {
            mi355enc_roi_t t, before;
            memset(&t, 0x5a, sizeof t); before = t;
            if (mi355enc_roi_parse(junk[i], &t) != MI355ENC_ERR_ARG || memcmp(&t, &before, sizeof t)) bad++;
            parses++;
        }
        mi355enc_roi_t t = base();
        if (mi355enc_roi_parse("", &t) != MI355ENC_OK || t.n_rects != 0 || t.balance != 6 || mi355enc_roi_parse(" \t", &t) != MI355ENC_OK) bad++;
        if (mi355enc_roi_parse(" 1 , 2 ,3,4, +5 , 6 ", &t) != MI355ENC_OK || t.n_rects != 1 || t.rect[0].delta != 5 || t.rect[0].feather != 6) bad++;
        if (mi355enc_roi_parse(NULL, &t) != MI355ENC_ERR_ARG || mi355enc_roi_parse("", NULL) != MI355ENC_ERR_ARG) bad++;
        parses += 5;
    }
    printf("{\"bad\": %ld, \"checks\": %ld, \"maps\": %ld, \"parses\": %ld, \"checksum\": %lu}\n", bad, checks, maps, parses, (unsigned long)fnv);
    return bad ? 1 : 0;
}
