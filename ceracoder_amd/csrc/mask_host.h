/* mask_host.h -- the rule of the privacy masks in plain C, all integers: what the host entry points of the ABI (mi355enc_mask_*),
 * the handle (enc_mask.cpp) and the kernels (k_mask.hip) share.  No device needed. */
#ifndef MI355_MASK_HOST_H
#define MI355_MASK_HOST_H
#include <stdint.h>

#include "../../include/mi355enc.h"

#define MASK_REGIONS_MAX 8
#define MASK_COORD_MAX 16384
#define MASK_MODE_FILL 1
#define MASK_MODE_PIXELATE 2
#define MASK_MODE_BLUR 3
#define MASK_CELL_MIN 4
#define MASK_CELL_MAX 64
#define MASK_RADIUS_MAX 32
#define MASK_DIV_SHIFT 23

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MASK_FN static __host__ __device__ inline
#else
#define MASK_FN static inline
#endif

/* a region as the rule reads it: the even rectangle (x0, y0, W2 x H2, rule 1), its intersection C with the visible picture (cx0 >= cx1 or cy0 >= cy1: empty),
 * mode, param and shape as set, and the fill colour in the output's Y, Cb, Cr */
typedef struct {
    int32_t x0, y0, W2, H2;
    int32_t cx0, cy0, cx1, cy1;
    int32_t mode, param, shape;
    int32_t cy, ccb, ccr;
} mask_reg_t;
typedef struct {
    int32_t n;
    mask_reg_t r[MASK_REGIONS_MAX];
} mask_tab_t;

/* rule 6's division: (sum + r) / (2r + 1) as a multiplication by m = mask_recip(2r + 1) and a shift.  With e = m n - 2^23 in 1 .. n the product is exact while
 * x e < 2^23; x <= 255 * 65 + 32 and n <= 65 give x e < 2^21, and x m < 2^31 (tests/test_mask_cpu.py goes through every sum of every radius) */
MASK_FN uint32_t mask_recip(int n) { return (1u << MASK_DIV_SHIFT) / (uint32_t)n + 1u; }
MASK_FN uint32_t mask_div(uint32_t x, uint32_t m) { return (x * m) >> MASK_DIV_SHIFT; }

MASK_FN int mask_empty(const mask_reg_t *r) { return r->cx0 >= r->cx1 || r->cy0 >= r->cy1; }

/* rule 2: whether the 2 x 2 quad whose first luma sample is (px, py) -- both even, picture coordinates -- belongs to the region */
MASK_FN int mask_inside(const mask_reg_t *r, int px, int py) {
    if (px < r->cx0 || px >= r->cx1 || py < r->cy0 || py >= r->cy1) return 0;
    if (!r->shape) return 1;
    const int64_t W2 = r->W2, H2 = r->H2; /* (2 qx + 1 = px - x0 + 1 for the quad at region-local qx = (px - x0) / 2) */
    const int64_t dx = 2 * (int64_t)(px - r->x0 + 1) - W2, dy = 2 * (int64_t)(py - r->y0 + 1) - H2;
    return dx * dx * H2 * H2 + dy * dy * W2 * W2 <= W2 * W2 * H2 * H2;
}
/* rule 3: region k owns the quad iff it contains it and no region in front of it does */
MASK_FN int mask_owns(const mask_tab_t *t, int k, int px, int py) {
    if (!mask_inside(&t->r[k], px, py)) return 0;
    for (int j = 0; j < k; j++)
        if (mask_inside(&t->r[j], px, py)) return 0;
    return 1;
}

#ifdef __cplusplus
extern "C" {
#endif
/* a checked configuration, the ten words of mi355enc_csc_coefficients and the visible size (even) -> the table: every region keeps its index, one with an empty
 * C stays in it and contains nothing.  MI355ENC_ERR_ARG for a configuration mi355enc_mask_check refuses or a size that is not even and 2 .. 16384 */
int mask_resolve(const mi355enc_mask_t *cfg, const int32_t coef[10], int vw, int vh, mask_tab_t *tab);
#ifdef __cplusplus
}
#endif

#endif
