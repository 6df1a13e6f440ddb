/* san_image_driver.c -- drives image_host.c under ASan + UBSan (make san/san_image; tests/test_image_san_cpu.py).  Host code only.
 * Two valid PAM files are made here (RGB_ALPHA 5 x 3 with a comment line, RGB 4 x 2); the loader gets every prefix of each, and each with every header
 * byte replaced by each of 0, '9', ' ', '\n', 0xFF.  Every input lives in a heap block of exactly its length and the pixel buffer has exactly the
 * size offered, so a read or write outside either is a sanitizer report.  Prints how many cases returned OK and how many an error; a case that
 * returns OK has to report sizes the offered buffer holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355enc.h"

static int ok, err;

static int run_case(const uint8_t *data, size_t len) {
    uint8_t *in = (uint8_t *)malloc(len ? len : 1);
    if (!in) return -100;
    memcpy(in, data, len);
    int w = -1, h = -1;
    int r = mi355enc_image_load_pam(in, len, &w, &h, NULL, 0);
    if (!r) {
        if (w < 1 || h < 1 || w > MI355ENC_IMAGE_MAX_DIM || h > MI355ENC_IMAGE_MAX_DIM) { free(in); return -101; }
        const size_t cap = (size_t)w * (size_t)h * 4;
        uint8_t *px = (uint8_t *)malloc(cap);
        if (!px) { free(in); return -100; }
        int w2 = -1, h2 = -1;
        r = mi355enc_image_load_pam(in, len, &w2, &h2, px, cap);
        if (r || w2 != w || h2 != h) r = -101; /* the size-only call and the real one disagree */
        else if (cap > 4 && mi355enc_image_load_pam(in, len, &w2, &h2, px, cap - 1) != MI355ENC_ERR_OVERFLOW) r = -101;
        free(px);
    }
    free(in);
    if (r == -100 || r == -101) return r;
    if (r) err++; else ok++;
    return 0;
}

static int sweep(const char *header, int depth, int w, int h) {
    const size_t hl = strlen(header), n = hl + (size_t)w * h * depth;
    uint8_t *f = (uint8_t *)malloc(n);
    if (!f) return -100;
    memcpy(f, header, hl);
    for (size_t i = hl; i < n; i++) f[i] = (uint8_t)(i * 37 + 11);
    const int before = ok;
    for (size_t k = 0; k <= n; k++) { const int r = run_case(f, k); if (r) { free(f); return r; } }
    if (ok != before + 1) { free(f); return -102; } /* only the whole file is one */
    static const uint8_t vals[5] = {0, '9', ' ', '\n', 0xFF};
    for (size_t p = 0; p < hl; p++)
        for (int v = 0; v < 5; v++) {
            const uint8_t old = f[p];
            f[p] = vals[v];
            const int r = run_case(f, n);
            f[p] = old;
            if (r) { free(f); return r; }
        }
    free(f);
    return 0;
}

int main(void) {
    int r = sweep("P7\n# a comment\nWIDTH 5\nHEIGHT 3\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n", 4, 5, 3);
    if (!r) r = sweep("P7\nHEIGHT 2\nWIDTH 4\nMAXVAL 255\nDEPTH 3\nTUPLTYPE RGB\nENDHDR\n", 3, 4, 2);
    if (r) { fprintf(stderr, "san_image: case failed (%d)\n", r); return 3; }
    printf("{\"ok\":%d,\"err\":%d}\n", ok, err);
    return 0;
}
