/* san_mask_driver.c -- the host side of the privacy masks (mask_host.c) under ASan + UBSan (make san/san_mask; tests/test_mask_san_cpu.py): the check at both
 * edges of every field's range and one step outside; the scalar rule -- on heap planes of exactly the visible size -- with every field at its edges, with
 * regions beyond every picture edge, on 16 x 16 and 8192 x 16 pictures and over 200 seeded random configurations; the parser on its own strings, on every
 * truncation of one and on junk.  Prints a JSON line with an FNV-1a checksum over a digest of every picture it made, which tests/maskref.py reproduces from
 * the same seed.  Host code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355enc.h"

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static const int32_t coef[10] = {16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681, 16}; /* mi355enc_csc_coefficients(6, 0) */
static uint32_t fnv = 2166136261u;
static long pictures = 0, bad = 0;

static mi355enc_mask_region_t reg(int x, int y, int w, int h, int mode, int param, int shape, unsigned colour) {
    mi355enc_mask_region_t r;
    r.x = x; r.y = y; r.w = w; r.h = h; r.mode = mode; r.param = param; r.shape = shape; r.colour = colour;
    return r;
}
static mi355enc_mask_region_t base(void) { return reg(3, 5, 9, 7, 3, 2, 0, 0x204060u); }

/* one picture of exactly w h and w h / 2 bytes, byte i a hash of i and a seed drawn here, through the rule; its digest goes into the checksum */
static void one(int w, int h, const mi355enc_mask_t *cfg) {
    const uint32_t seed = rnd();
    const size_t ny = (size_t)w * h, nc = ny / 2;
    uint8_t *y = (uint8_t *)malloc(ny), *uv = (uint8_t *)malloc(nc);
    if (!y || !uv) exit(2);
    for (size_t i = 0; i < ny + nc; i++) {
        uint32_t v = (uint32_t)i * 2654435761u + seed;
        v ^= v >> 15; v *= 2246822519u; v ^= v >> 13;
        *(i < ny ? &y[i] : &uv[i - ny]) = (uint8_t)v;
    }
    if (mi355enc_mask_apply_host(cfg, coef, w, h, y, uv) != MI355ENC_OK) bad++;
    uint64_t d = 0;
    for (size_t i = 0; i < ny + nc; i++) d += (uint64_t)(i < ny ? y[i] : uv[i - ny]) * (uint64_t)((uint32_t)i * 2654435761u + 12345u);
    for (int k = 0; k < 4; k++) fnv = (fnv ^ (uint32_t)((d >> (8 * k)) & 255u)) * 16777619u;
    pictures++;
    free(y); free(uv);
}
static void one1(int w, int h, mi355enc_mask_region_t r) {
    mi355enc_mask_t c;
    memset(&c, 0, sizeof c);
    c.n = 1; c.region[0] = r;
    one(w, h, &c);
}
static void refused(mi355enc_mask_region_t r) {
    mi355enc_mask_t c;
    memset(&c, 0, sizeof c);
    c.n = 1; c.region[0] = r;
    uint8_t y[4] = {1, 2, 3, 4}, uv[2] = {5, 6};
    if (mi355enc_mask_check(&c) != MI355ENC_ERR_ARG || mi355enc_mask_apply_host(&c, coef, 2, 2, y, uv) != MI355ENC_ERR_ARG || y[0] != 1 || uv[1] != 6) bad++;
}

int main(void) {
    long checks = 0, parses = 0;
    /* every field: lo - 1 and hi + 1 are refused, lo and hi accepted and applied */
    static const long lo[6] = {-16384, -16384, 1, 1, 0, 0}, hi[6] = {16384, 16384, 16384, 16384, 1, 0xFFFFFF};
    for (int f = 0; f < 6; f++)
        for (int k = 0; k < 4; k++) {
            mi355enc_mask_region_t r = base();
            const long v = k == 0 ? lo[f] : k == 1 ? hi[f] : k == 2 ? lo[f] - 1 : hi[f] + 1;
            if (f == 5 && k == 2) continue; /* (an unsigned field has nothing below 0) */
            switch (f) { case 0: r.x = (int)v; break; case 1: r.y = (int)v; break; case 2: r.w = (int)v; break; case 3: r.h = (int)v; break; case 4: r.shape = (int)v; break; default: r.colour = (unsigned)v; }
            if (k < 2) one1(16, 16, r); else refused(r);
            checks++;
        }
    /* mode and param together: every mode at both edges of its param, on the small picture and as an ellipse over most of a larger one */
    static const int modes[5][2] = {{1, 0}, {2, 4}, {2, 64}, {3, 1}, {3, 32}};
    for (int i = 0; i < 5; i++) {
        mi355enc_mask_region_t r = base();
        r.mode = modes[i][0]; r.param = modes[i][1];
        one1(16, 16, r);
        one1(70, 50, reg(1, 1, 67, 47, modes[i][0], modes[i][1], 1, 0x808080u));
        checks++;
    }
    static const int wrong[10][2] = {{0, 0}, {4, 1}, {1, -1}, {1, 1}, {2, 2}, {2, 5}, {2, 66}, {3, 0}, {3, 33}, {-1, 4}};
    for (int i = 0; i < 10; i++) { mi355enc_mask_region_t r = base(); r.mode = wrong[i][0]; r.param = wrong[i][1]; refused(r); checks++; }
    {   /* eight regions and none; nine and minus one are refused */
        mi355enc_mask_t c;
        memset(&c, 0, sizeof c);
        for (int k = 0; k < 8; k++) c.region[k] = base();
        c.n = 8; one(16, 16, &c);
        c.n = 0; one(16, 16, &c);
        c.n = 9; if (mi355enc_mask_check(&c) != MI355ENC_ERR_ARG) bad++;
        c.n = -1; if (mi355enc_mask_check(&c) != MI355ENC_ERR_ARG) bad++;
        if (mi355enc_mask_check(NULL) != MI355ENC_ERR_ARG) bad++;
        checks += 5;
    }
    /* regions beyond every picture edge of 42 x 26, partly and wholly, as rectangles and as ellipses */
    static const int beyond[13][4] = {{-40, 4, 60, 12}, {-100, 4, 100, 12}, {-100, 4, 99, 12}, {30, 4, 100, 12}, {42, 4, 10, 12}, {41, 4, 1, 12}, {4, -30, 12, 50}, {4, -50, 12, 50},
                                      {4, 20, 12, 50}, {4, 26, 12, 50}, {-16384, -16384, 16384, 16384}, {-16383, -16383, 16384, 16384}, {-16384, -16384, 16384 + 20, 16384 + 12}};
    static const int bparam[3] = {0, 6, 5};
    for (int i = 0; i < 13; i++)
        for (int shape = 0; shape < 2; shape++) {
            mi355enc_mask_region_t r = reg(beyond[i][0], beyond[i][1], beyond[i][2], beyond[i][3], 1 + i % 3, bparam[i % 3], shape, 0x10F0A0u);
            if (i == 12) { refused(r); r.w = 16384; r.h = 16384; r.x = -16384 + 20; r.y = -16384 + 12; } /* (w beyond its range; then the same reach inside it) */
            one1(42, 26, r);
        }
    /* the smallest picture of the tests and the widest strip */
    static const int sizes2[2][2] = {{16, 16}, {8192, 16}};
    for (int i = 0; i < 2; i++) {
        const int w = sizes2[i][0], h = sizes2[i][1];
        one1(w, h, reg(0, 0, w, h, 3, 32, 0, 0));
        one1(w, h, reg(-5, -3, w + 9, h + 7, 2, 64, 1, 0));
        mi355enc_mask_t c;
        memset(&c, 0, sizeof c);
        c.n = 3; c.region[0] = reg(w - 3, h - 3, 3, 3, 1, 0, 0, 0xFF0000u); c.region[1] = reg(1, 1, w - 2, h - 2, 3, 7, 1, 0); c.region[2] = reg(0, 0, w, h, 2, 6, 0, 0);
        one(w, h, &c);
    }
    /* seeded random configurations */
    static const int sizes[4][2] = {{16, 16}, {42, 26}, {70, 50}, {18, 34}};
    for (int i = 0; i < 200; i++) {
        const int w = sizes[i % 4][0], h = sizes[i % 4][1];
        mi355enc_mask_t c;
        memset(&c, 0, sizeof c);
        c.n = rnd_in(0, 8);
        for (int k = 0; k < c.n; k++) {
            mi355enc_mask_region_t *r = &c.region[k];
            r->x = rnd_in(-20, w + 10); r->y = rnd_in(-20, h + 10); r->w = rnd_in(1, w + 30); r->h = rnd_in(1, h + 30);
            r->mode = rnd_in(1, 3);
            r->param = r->mode == 1 ? 0 : r->mode == 2 ? 2 * rnd_in(2, 32) : rnd_in(1, 32);
            r->shape = rnd_in(0, 1); r->colour = rnd() & 0xFFFFFFu;
        }
        one(w, h, &c);
    }
    /* sizes the rule refuses */
    { uint8_t y[4] = {0}, uv[2] = {0}; mi355enc_mask_t c; memset(&c, 0, sizeof c);
      if (mi355enc_mask_apply_host(&c, coef, 3, 2, y, uv) != MI355ENC_ERR_ARG || mi355enc_mask_apply_host(&c, coef, 2, 0, y, uv) != MI355ENC_ERR_ARG ||
          mi355enc_mask_apply_host(&c, coef, 2, 2, NULL, uv) != MI355ENC_ERR_ARG || mi355enc_mask_apply_host(&c, NULL, 2, 2, y, uv) != MI355ENC_ERR_ARG) bad++; }
    /* the parts of the rule on their own */
    for (int r = 1; r <= 32; r++) for (int s = 0; s <= 255 * (2 * r + 1); s++) if (mi355enc_mask_mean(s, r) != (s + r) / (2 * r + 1)) bad++;
    if (mi355enc_mask_mean(-1, 1) != MI355ENC_ERR_ARG || mi355enc_mask_mean(766, 1) != MI355ENC_ERR_ARG || mi355enc_mask_mean(0, 0) != MI355ENC_ERR_ARG || mi355enc_mask_mean(0, 33) != MI355ENC_ERR_ARG) bad++;
    if (mi355enc_mask_ellipse(2, 2, 0, 0) != 1 || mi355enc_mask_ellipse(32770, 32770, 0, 0) != 0 || mi355enc_mask_ellipse(32770, 32770, 8192, 8192) != 1 || mi355enc_mask_ellipse(32770, 2, 0, 0) != 1 ||
        mi355enc_mask_ellipse(32772, 2, 0, 0) != MI355ENC_ERR_ARG || mi355enc_mask_ellipse(4, 4, 2, 0) != MI355ENC_ERR_ARG || mi355enc_mask_ellipse(3, 4, 0, 0) != MI355ENC_ERR_ARG) bad++;
    /* the parser: its own strings round-trip, every truncation of one is parsed or refused (and a refusal leaves the output alone), junk is refused */
    {
        static const char *good = "16,32,640,360,3,16,1;-20,0,64,64,2,8;1000,1000,1,1,1,0,0";
        mi355enc_mask_t c;
        memset(&c, 0, sizeof c);
        if (mi355enc_mask_parse(good, 0x123456u, &c) != MI355ENC_OK || c.n != 3 || c.region[0].mode != 3 || c.region[0].param != 16 || c.region[0].shape != 1 || c.region[1].x != -20 ||
            c.region[1].shape != 0 || c.region[2].mode != 1 || c.region[2].colour != 0x123456u)
            bad++;
        parses++;
        const size_t len = strlen(good);
        for (size_t k = 0; k <= len; k++) {
            char *copy = (char *)malloc(k + 1); /* exactly its length and the terminator */
            if (!copy) return 2;
            memcpy(copy, good, k); copy[k] = 0;
            mi355enc_mask_t t, before;
            memset(&t, 0x5a, sizeof t); before = t;
            const int r = mi355enc_mask_parse(copy, 0, &t);
            if (r == MI355ENC_OK) { if (mi355enc_mask_check(&t)) bad++; }
            else if (r != MI355ENC_ERR_ARG || memcmp(&t, &before, sizeof t)) bad++;
            parses++;
            free(copy);
        }
        static const char *junk[] = {"x", "1,2,3,4,3", "1,2,3,4,0,4", "1,2,3,4,4,4", "1,2,3,4,2,5", "1,2,3,4,3,33", "1,2,3,4,1,1", "1,2,3,4,3,4,2", "1,2,3,4,3,4,0,7", "1,2,3,4,3,4;", ";1,2,3,4,3,4",
                                     "1,2,3,4,3,4;;1,2,3,4,3,4", "1,,3,4,3,4", "1,2,0,4,3,4", "1 2,3,4,3,4,0", "1,2,3,4,3,4x", "99999999999999999999,2,3,4,3,4", "1,2,3,4,3,-", "1.5,2,3,4,3,4",
                                     "1,1,1,1,1,0;1,1,1,1,1,0;1,1,1,1,1,0;1,1,1,1,1,0;1,1,1,1,1,0;1,1,1,1,1,0;1,1,1,1,1,0;1,1,1,1,1,0;1,1,1,1,1,0"};
        for (size_t i = 0; i < sizeof junk / sizeof junk[0]; i++) {
            mi355enc_mask_t t, before;
            memset(&t, 0x5a, sizeof t); before = t;
            if (mi355enc_mask_parse(junk[i], 0, &t) != MI355ENC_ERR_ARG || memcmp(&t, &before, sizeof t)) bad++;
            parses++;
        }
        mi355enc_mask_t t;
        memset(&t, 0x5a, sizeof t);
        if (mi355enc_mask_parse("", 0, &t) != MI355ENC_OK || t.n != 0 || mi355enc_mask_parse(" \t", 0, &t) != MI355ENC_OK) bad++;
        if (mi355enc_mask_parse(" 1 , 2 ,3,4, +3 , 6 ", 0, &t) != MI355ENC_OK || t.n != 1 || t.region[0].mode != 3 || t.region[0].param != 6) bad++;
        if (mi355enc_mask_parse(NULL, 0, &t) != MI355ENC_ERR_ARG || mi355enc_mask_parse("", 0, NULL) != MI355ENC_ERR_ARG || mi355enc_mask_parse("", 0x1000000u, &t) != MI355ENC_ERR_ARG) bad++;
        parses += 6;
    }
    printf("{\"bad\": %ld, \"checks\": %ld, \"pictures\": %ld, \"parses\": %ld, \"checksum\": %lu}\n", bad, checks, pictures, parses, (unsigned long)fnv);
    return bad ? 1 : 0;
}
