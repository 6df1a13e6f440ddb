/* san_jpeg_driver.c -- drives jpeg_host.c under ASan + UBSan (make sanitize; tests/test_jpeg_cpu.py).  Host code only.
 *   san_jpeg decode FILE            the picture as it is: prints the return code and a checksum of what was decoded
 *   san_jpeg trunc  FILE            the picture cut at every length 0 .. size
 *   san_jpeg fuzz   FILE SEED N     N single-byte corruptions: position and value from a 64-bit LCG seeded with SEED
 * Every input lives in a heap block of exactly its length and every coefficient buffer has exactly the size offered, so a read or write
 * outside either is a sanitizer report.  trunc / fuzz print how many cases returned OK and how many an error. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpeg_host.h"

#define CAP_MAX ((size_t)1 << 22) /* int16 offered at most: a corrupt header may announce any size */

static int run_case(const uint8_t *data, size_t len, unsigned long long *sum) {
    uint8_t *in = (uint8_t *)malloc(len ? len : 1);
    if (!in) return -100;
    memcpy(in, data, len);
    mi355enc_jpeg_info_t info;
    int r = mi355enc_jpeg_info(in, len, &info);
    if (!r) {
        int bw[3], bh[3];
        size_t first[3];
        size_t cap = jpeg_host_layout(&info, bw, bh, first) * 64;
        if (cap > CAP_MAX) cap = CAP_MAX;
        int16_t *coef = (int16_t *)malloc(cap * sizeof(int16_t));
        uint16_t(*qt)[64] = (uint16_t(*)[64])malloc(3 * 64 * sizeof(uint16_t));
        if (!coef || !qt) { free(in); free(coef); free(qt); return -100; }
        r = mi355enc_jpeg_entropy_decode(in, len, coef, cap, qt, &info);
        if (!r && sum) {
            unsigned long long s = 1469598103934665603ull;
            for (size_t i = 0; i < cap; i++) s = (s ^ (uint16_t)coef[i]) * 1099511628211ull;
            const uint16_t *q = (const uint16_t *)qt;
            for (int i = 0; i < 192; i++) s = (s ^ q[i]) * 1099511628211ull;
            *sum = s;
        }
        free(coef); free(qt);
    }
    free(in);
    return r;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s decode|trunc|fuzz FILE [SEED N]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *data = (uint8_t *)malloc(size > 0 ? (size_t)size : 1);
    if (!data || size < 0 || fread(data, 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    fclose(f);
    int ok = 0, err = 0;
    if (!strcmp(argv[1], "decode")) {
        unsigned long long sum = 0;
        const int r = run_case(data, (size_t)size, &sum);
        printf("{\"rc\":%d,\"sum\":\"%016llx\"}\n", r, sum);
    } else if (!strcmp(argv[1], "trunc")) {
        for (long n = 0; n <= size; n++) { const int r = run_case(data, (size_t)n, NULL); if (r == -100) return 3; if (r) err++; else ok++; }
        printf("{\"ok\":%d,\"err\":%d}\n", ok, err);
    } else if (!strcmp(argv[1], "fuzz") && argc >= 5) {
        unsigned long long x = strtoull(argv[3], NULL, 0);
        const int n = atoi(argv[4]);
        for (int i = 0; i < n && size > 0; i++) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const size_t pos = (size_t)((x >> 33) % (unsigned long long)size);
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const uint8_t val = (uint8_t)(x >> 56), old = data[pos];
            data[pos] = val;
            const int r = run_case(data, (size_t)size, NULL);
            data[pos] = old;
            if (r == -100) return 3;
            if (r) err++; else ok++;
        }
        printf("{\"ok\":%d,\"err\":%d}\n", ok, err);
    } else return 2;
    free(data);
    return 0;
}
