/* san_warp_driver.c -- the mesh warp's rule (warp_host.c) under ASan + UBSan (make san/san_warp; tests/test_warp_san_cpu.py): the coefficient table, the
 * builder at every range edge of every parameter at the sizes 2 x 2, 64 x 48 and 8192 x 16 into meshes of exactly their size (a mesh it accepts holds valid
 * nodes only), and the whole warp of seeded noise through the six named sets, a folded mesh and meshes pinned to the node range's ends, both filters, into
 * planes of exactly their size.  Prints a JSON count.  Host code only. */
#include "warp_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355enc.h"

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static const mi355enc_warp_params_t k_sets[6] = {
    {-13107, 1966, 65536, 65536, 0, 0, 0},          /* barrel */
    {0, 0, 65536, 65454, 3276, 0, 0},               /* roll */
    {0, 0, 65536, 65536, 0, 8192, -8192},           /* keystone */
    {-13107, 1966, 60000, 65454, 3276, 8192, -4096}, /* all */
    {0, 0, 65536, 0, 65536, 0, 0},                  /* quarter turn */
    {0, 0, 163840, 65536, 0, 0, 0},                 /* shrink */
};

/* builds into a mesh of exactly its size; 1: accepted (and every node valid) */
static int build_exact(const mi355enc_warp_params_t *p, int w, int h, long *bad) {
    int nx, ny;
    if (mi355enc_warp_mesh_size(w, h, &nx, &ny)) { (*bad)++; return 0; }
    const size_t n = (size_t)2 * nx * ny;
    int32_t *m = (int32_t *)malloc(n * sizeof *m);
    if (!m) { (*bad)++; return 0; }
    const int r = mi355enc_warp_build(p, w, h, m, n);
    if (r == MI355ENC_OK && mi355enc_warp_mesh_check(m, nx, ny)) (*bad)++;
    if (r != MI355ENC_OK && r != MI355ENC_ERR_ARG) (*bad)++;
    if (mi355enc_warp_build(p, w, h, m, n - 1) != MI355ENC_ERR_ARG) (*bad)++;
    free(m);
    return r == MI355ENC_OK;
}

int main(void) {
    long bad = 0, coeffs = 0, edges = 0, built = 0, pictures = 0;
    for (int kind = 0; kind < 2; kind++)
        for (int f = 0; f < 32; f++) {
            int16_t c[4];
            if (mi355enc_warp_coeff(kind, f, c) || c[0] + c[1] + c[2] + c[3] != 128) bad++;
            coeffs++;
        }
    /* every edge of every parameter, two steps to either side, alone and with every other parameter at an edge of its own */
    const int lo[7] = {-65536, -65536, 16384, -65536, -65536, -32768, -32768}, hi[7] = {65536, 65536, 262144, 65536, 65536, 32768, 32768};
    const int sizes[3][2] = {{2, 2}, {64, 48}, {8192, 16}};
    for (int z = 0; z < 3; z++)
        for (int i = 0; i < 7; i++)
            for (int e = 0; e < 2; e++)
                for (int d = -2; d <= 2; d++)
                    for (int others = 0; others < 3; others++) {
                        mi355enc_warp_params_t p;
                        mi355enc_warp_params_default(&p);
                        int *f = &p.k1;
                        for (int k = 0; k < 7 && others; k++) f[k] = others == 1 ? lo[k] : hi[k];
                        f[i] = (e ? hi[i] : lo[i]) + d;
                        const int ok = build_exact(&p, sizes[z][0], sizes[z][1], &bad);
                        if (ok && (f[i] < lo[i] || f[i] > hi[i])) bad++;
                        built += ok;
                        edges++;
                    }
    mi355enc_warp_params_default(NULL);
    /* the whole warp: planes and mesh of exactly their size */
    const int pics[4][2] = {{72, 40}, {64, 48}, {96, 96}, {160, 96}};
    for (int z = 0; z < 4; z++) {
        const int w = pics[z][0], h = pics[z][1];
        int nx, ny;
        if (mi355enc_warp_mesh_size(w, h, &nx, &ny)) { bad++; continue; }
        const size_t n = (size_t)2 * nx * ny, ysz = (size_t)w * h, csz = ysz / 2;
        int32_t *m = (int32_t *)malloc(n * sizeof *m);
        uint8_t *y = (uint8_t *)malloc(ysz), *uv = (uint8_t *)malloc(csz), *oy = (uint8_t *)malloc(ysz), *ouv = (uint8_t *)malloc(csz);
        if (!m || !y || !uv || !oy || !ouv) return 2;
        for (size_t k = 0; k < ysz; k++) y[k] = (uint8_t)rnd();
        for (size_t k = 0; k < csz; k++) uv[k] = (uint8_t)rnd();
        for (int set = 0; set < 10; set++) {
            if (set < 6) { if (mi355enc_warp_build(&k_sets[set], w, h, m, n)) { bad++; continue; } }
            else if (set == 6) for (size_t k = 0; k < n; k++) m[k] = (int32_t)(rnd() % (unsigned)(w * 256 + 48 * 256)) - 24 * 256; /* folded */
            else if (set == 7) for (size_t k = 0; k < n; k++) m[k] = WARP_NODE_MIN;
            else if (set == 8) for (size_t k = 0; k < n; k++) m[k] = WARP_NODE_MAX;
            else for (size_t k = 0; k < n; k++) m[k] = (rnd() & 1) ? WARP_NODE_MAX : WARP_NODE_MIN; /* the interpolation at its ceiling */
            for (int kind = 0; kind < 2; kind++) {
                const mi355enc_warp_t s = {kind, {16, 128, 128}};
                if (mi355enc_warp_apply_host(&s, m, w, h, y, w, uv, w, oy, w, ouv, w)) bad++;
                if (set == 7 || set == 8) /* wholly outside: the fill */
                    for (size_t k = 0; k < ysz; k++) if (oy[k] != 16) { bad++; break; }
                pictures++;
            }
        }
        m[n - 1] = WARP_NODE_MAX + 1;
        const mi355enc_warp_t s = {1, {0, 0, 0}};
        if (mi355enc_warp_apply_host(&s, m, w, h, y, w, uv, w, oy, w, ouv, w) != MI355ENC_ERR_ARG) bad++;
        free(m); free(y); free(uv); free(oy); free(ouv);
    }
    printf("{\"bad\": %ld, \"coeffs\": %ld, \"edges\": %ld, \"built\": %ld, \"pictures\": %ld}\n", bad, coeffs, edges, built, pictures);
    return bad ? 1 : 0;
}
