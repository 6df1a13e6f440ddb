/* san_lut3d_driver.c -- the host side of the 3D colour LUT (lut3d_host.c) under ASan + UBSan (make san/san_lut3d; tests/test_lut3d_san_cpu.py): the parser on
 * the file named on the command line, on every truncation of it and on over-long variants, each from a heap copy of exactly its length into a buffer of exactly
 * N^3 words; the host rule at N = 2 and 65 on seeded noise, and at the ends of every clamp (samples 0 and 255 against tables of all zeros, all ones and seeded
 * noise, every matrix and range, strengths 1 and 256), into planes of exactly their size.  Prints a JSON count.  Host code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355enc.h"

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

/* one parse of len bytes from an exactly-sized heap copy into cap words on the heap */
static int parse(const char *text, size_t len, size_t cap, int *N, uint32_t *first) {
    char *copy = (char *)malloc(len ? len : 1);
    uint32_t *nodes = (uint32_t *)malloc((cap ? cap : 1) * sizeof *nodes);
    if (!copy || !nodes) exit(2);
    memcpy(copy, text, len);
    const int r = mi355enc_lut3d_parse_cube(copy, len, nodes, cap, N);
    if (r == MI355ENC_OK && first) *first = nodes[0];
    free(copy); free(nodes);
    return r;
}

/* the rule on planes of exactly w x h; returns the code */
static int apply(const uint32_t *nodes, int N, int strength, int matrix, int full, int w, int h, int fill, long *bad) {
    uint8_t *y = (uint8_t *)malloc((size_t)w * h), *uv = (uint8_t *)malloc((size_t)w * h / 2);
    if (!y || !uv) exit(2);
    for (int i = 0; i < w * h; i++) y[i] = fill < 0 ? (uint8_t)rnd() : fill == 256 ? (uint8_t)((rnd() & 1) * 255) : (uint8_t)fill;
    for (int i = 0; i < w * h / 2; i++) uv[i] = fill < 0 ? (uint8_t)rnd() : fill == 256 ? (uint8_t)((rnd() & 1) * 255) : (uint8_t)fill;
    const int rect[4] = {0, w, 0, h};
    const int r = mi355enc_lut3d_apply_host(nodes, N, strength, matrix, full, y, uv, w, h, rect);
    if (r != MI355ENC_OK) (*bad)++;
    free(y); free(uv);
    return r;
}

int main(int argc, char **argv) {
    long bad = 0, parses = 0, accepted = 0, pictures = 0;
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    char *text = (char *)malloc(1 << 16);
    if (!text) return 2;
    const size_t len = fread(text, 1, 1 << 16, f);
    fclose(f);
    /* the file itself, into exactly N^3 words; one word less is refused */
    int N = 0;
    uint32_t first = 0;
    if (parse(text, len, 27, &N, &first) != MI355ENC_OK || N != 3) bad++;
    if (parse(text, len, 26, &N, NULL) != MI355ENC_ERR_ARG) bad++;
    parses += 2; accepted++;
    /* every truncation: refused (rows are missing) or, where only the comments behind the last row are cut, the same table */
    for (size_t k = 0; k < len; k++) {
        uint32_t w0 = 0;
        const int r = parse(text, k, 27, &N, &w0);
        parses++;
        if (r == MI355ENC_OK) { accepted++; if (N != 3 || w0 != first) bad++; }
        else if (r != MI355ENC_ERR_ARG) bad++;
    }
    /* over-long variants: a row more, a number more in the last line, a digit string of 400 digits, an exponent of 400 digits, a line of 4000 blanks */
    {
        char *v = (char *)malloc(len + 8192);
        if (!v) return 2;
        memcpy(v, text, len);
        size_t n = len + (size_t)sprintf(v + len, "0.5 0.5 0.5\r\n");
        if (parse(v, n, 27, &N, NULL) != MI355ENC_ERR_ARG || parse(v, n, 28, &N, NULL) != MI355ENC_ERR_ARG) bad++;
        n = len; while (n && (v[n - 1] == '\n' || v[n - 1] == '\r')) n--;
        const char *head = "LUT_3D_SIZE 2\n0 0 0\n0 0 0\n0 0 0\n0 0 0\n0 0 0\n0 0 0\n0 0 0\n";
        size_t h = strlen(head);
        memcpy(v, head, h);
        n = h; memcpy(v + n, "0 0 0.", 6); n += 6; memset(v + n, '9', 400); n += 400; v[n++] = '\n';
        if (parse(v, n, 8, &N, NULL) != MI355ENC_OK) bad++;
        n = h; memcpy(v + n, "0 0 ", 4); n += 4; memset(v + n, '9', 400); n += 400; v[n++] = '\n';
        if (parse(v, n, 8, &N, NULL) != MI355ENC_ERR_ARG) bad++;
        n = h; memcpy(v + n, "0 0 1e", 6); n += 6; memset(v + n, '9', 400); n += 400; v[n++] = '\n';
        if (parse(v, n, 8, &N, NULL) != MI355ENC_ERR_ARG) bad++;
        n = h; memcpy(v + n, "0 0 1e-", 7); n += 7; memset(v + n, '9', 400); n += 400; v[n++] = '\n';
        if (parse(v, n, 8, &N, NULL) != MI355ENC_OK) bad++;
        n = h; memset(v + n, ' ', 4000); n += 4000; memcpy(v + n, "0 0 0", 5); n += 5;
        if (parse(v, n, 8, &N, NULL) != MI355ENC_OK) bad++;
        if (parse(v, 0, 8, &N, NULL) != MI355ENC_ERR_ARG) bad++;
        parses += 8;
        free(v);
    }
    free(text);
    /* the rule: N = 2 and 65 on noise, and the ends of every clamp */
    static const int mats[4] = {1, 5, 6, 9};
    for (int big = 0; big < 2; big++) {
        const int n = big ? 65 : 2, words = n * n * n;
        uint32_t *nodes = (uint32_t *)malloc((size_t)words * sizeof *nodes);
        if (!nodes) return 2;
        for (int kind = 0; kind < 4; kind++) { /* zeros, ones, noise, the identity */
            for (int k = 0; k < words; k++) nodes[k] = kind == 0 ? 0u : kind == 1 ? 0x3fffffffu : rnd() & 0x3fffffffu;
            if (kind == 3 && mi355enc_lut3d_identity(n, nodes)) bad++;
            if (mi355enc_lut3d_check(nodes, n)) bad++;
            for (int m = 0; m < 4; m++) for (int full = 0; full < 2; full++) for (int s = 0; s < 2; s++) {
                static const int fills[5] = {-1, 0, 255, 256, 128}; /* noise, all 0, all 255, 0 / 255 mixed, grey */
                for (int c = 0; c < 5; c++) { apply(nodes, n, s ? 256 : 1, mats[m], full, c ? 16 : 48, c ? 4 : 34, fills[c], &bad); pictures++; }
            }
        }
        nodes[words - 1] |= 0x40000000u;
        if (mi355enc_lut3d_check(nodes, n) != MI355ENC_ERR_ARG) bad++;
        free(nodes);
    }
    printf("{\"bad\": %ld, \"parses\": %ld, \"accepted\": %ld, \"pictures\": %ld}\n", bad, parses, accepted, pictures);
    return bad ? 1 : 0;
}
