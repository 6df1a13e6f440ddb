/* san_snapshot_driver.c -- drives snapshot_host.c under ASan + UBSan (make san/san_snapshot; tests/test_snapshot_san_cpu.py).  Host code only.
 * The writer of the JPEG stills gets random level sets (sparse, dense, with long zero runs), extreme ones (every AC +-1023, DC differences of 11 bits, all
 * bits set) and sets it must refuse, for stills of 16 x 16, 50 x 34 and 9 x 5, with a hint per block and without.  Levels, hints and the output live in heap
 * blocks of exactly their size, and every case is written into every capacity from 0 to its length: a read or write outside is a sanitizer report, a
 * capacity below the length must return MI355ENC_ERR_OVERFLOW with the length.  Files of even sizes go back through the product's own entropy decoder and
 * must return the levels.  Prints how many files were written, how many sets were refused and how many capacities were tried. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "snapshot_host.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd(void) { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(rng_state >> 33); }

static long files, refused, caps;
static const uint8_t zz_of[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                  10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

/* kind 0: sparse small levels; 1: dense random up to the limits; 2: extreme, alternating signs; 3: all -1; 4: a level that cannot be coded */
static void fill(int16_t *lv, size_t nblk, int kind) {
    for (size_t b = 0; b < nblk; b++) {
        int16_t *k = lv + b * 64;
        for (int i = 0; i < 64; i++) {
            if (kind == 0) k[i] = (rnd() % 8 == 0) ? (int16_t)((int)(rnd() % 9) - 4) : 0;
            else if (kind == 1) k[i] = (rnd() % 3 == 0) ? 0 : (int16_t)((int)(rnd() % 2047) - 1023);
            else if (kind == 2) k[i] = (int16_t)((i & 1) ? -1023 : 1023);
            else k[i] = -1;
        }
        if (kind == 0 && rnd() % 4 == 0) { memset(k + 1, 0, 63 * sizeof *k); if (rnd() % 2) k[63] = 1; } /* a run of 62 zeros, two ZRLs */
        k[0] = kind == 2 ? (int16_t)((b & 1) ? -1020 : 1020) : kind == 1 ? (int16_t)((int)(rnd() % 1021) - 510) : k[0];
    }
    if (kind == 4) lv[(rnd() % nblk) * 64 + 1 + rnd() % 63] = (int16_t)(rnd() % 2 ? 1024 : -2000);
}

static int run_case(int ow, int oh, int kind, int with_hint, int quality, int all_caps) {
    int bw[3], bh[3];
    size_t first[3];
    const size_t nblk = snapshot_host_blocks(ow, oh, bw, bh, first);
    int16_t *lv = (int16_t *)malloc(nblk * 64 * sizeof *lv);
    uint8_t *hint = (uint8_t *)malloc(nblk);
    uint16_t qt[2][64];
    if (!lv || !hint || mi355enc_snapshot_tables(quality, qt)) return -100;
    fill(lv, nblk, kind);
    for (size_t b = 0; b < nblk; b++) {
        int last = 0;
        for (int i = 1; i < 64; i++) if (lv[b * 64 + i] && zz_of[i] > last) last = zz_of[i];
        hint[b] = (uint8_t)last;
    }
    size_t len = 0;
    int r = snapshot_host_write(lv, with_hint ? hint : NULL, qt, ow, oh, NULL, 0, &len);
    if (kind == 4) { free(lv); free(hint); if (r != MI355ENC_ERR_ARG) return -101; refused++; return 0; }
    if (r != MI355ENC_ERR_OVERFLOW || len < 625 || len > mi355enc_snapshot_max_bytes(ow, oh)) return -102;
    uint8_t *ref = (uint8_t *)malloc(len);
    if (!ref) return -100;
    size_t n = 0;
    if (mi355enc_snapshot_write(lv, qt, ow, oh, ref, len, &n) || n != len) return -103; /* (without hints: the same file) */
    const size_t step = all_caps ? 1 : len / 97 + 1;
    for (size_t cap = 0; cap <= len; cap += (cap + step > len && cap < len) ? len - cap : step) {
        uint8_t *out = (uint8_t *)malloc(cap ? cap : 1);
        if (!out) return -100;
        n = 0;
        r = snapshot_host_write(lv, with_hint ? hint : NULL, qt, ow, oh, cap ? out : NULL, cap, &n);
        if (n != len || r != (cap < len ? MI355ENC_ERR_OVERFLOW : MI355ENC_OK) || memcmp(out, ref, cap < len ? cap : len)) return -104;
        free(out);
        caps++;
    }
    if (!((ow | oh) & 1)) { /* back through the product's decoder */
        int16_t *back = (int16_t *)malloc(nblk * 64 * sizeof *back);
        uint16_t q3[3][64];
        mi355enc_jpeg_info_t info;
        if (!back) return -100;
        if (mi355enc_jpeg_entropy_decode(ref, len, back, nblk * 64, q3, &info) || info.width != ow || info.height != oh) return -105;
        if (memcmp(back, lv, nblk * 64 * sizeof *lv) || memcmp(q3[0], qt[0], sizeof qt[0]) || memcmp(q3[2], qt[1], sizeof qt[1])) return -106;
        free(back);
    }
    free(ref); free(lv); free(hint);
    files++;
    return 0;
}

int main(void) {
    static const int sizes[3][2] = {{16, 16}, {50, 34}, {9, 5}};
    for (int s = 0; s < 3; s++)
        for (int kind = 0; kind <= 4; kind++)
            for (int with_hint = 0; with_hint < 2; with_hint++)
                for (int rep = 0; rep < 3; rep++) {
                    const int all_caps = sizes[s][0] != 50 || kind == 0; /* every capacity, except for the long files of the larger still: 98 of them */
                    const int r = run_case(sizes[s][0], sizes[s][1], kind, with_hint, rep == 0 ? 100 : rep == 1 ? 50 : 1, all_caps && rep == 0);
                    if (r) { fprintf(stderr, "san_snapshot: case %dx%d kind %d hint %d failed (%d)\n", sizes[s][0], sizes[s][1], kind, with_hint, r); return 3; }
                }
    /* arguments */
    uint16_t qt[2][64];
    int16_t lv[6 * 64] = {0};
    size_t n;
    uint8_t out[8];
    if (mi355enc_snapshot_tables(0, qt) != MI355ENC_ERR_ARG || mi355enc_snapshot_tables(101, qt) != MI355ENC_ERR_ARG || mi355enc_snapshot_tables(75, NULL) != MI355ENC_ERR_ARG) return 4;
    mi355enc_snapshot_tables(75, qt);
    if (mi355enc_snapshot_write(NULL, qt, 16, 16, out, 8, &n) != MI355ENC_ERR_ARG || mi355enc_snapshot_write(lv, qt, 0, 16, out, 8, &n) != MI355ENC_ERR_ARG ||
        mi355enc_snapshot_write(lv, qt, 16, 65536, out, 8, &n) != MI355ENC_ERR_ARG || mi355enc_snapshot_write(lv, qt, 16, 16, NULL, 8, &n) != MI355ENC_ERR_ARG) return 4;
    if (mi355enc_snapshot_reciprocal(0) || mi355enc_snapshot_reciprocal(256) || mi355enc_snapshot_reciprocal(1) != 0x20000000u) return 4;
    printf("{\"files\":%ld,\"refused\":%ld,\"caps\":%ld}\n", files, refused, caps);
    return 0;
}
