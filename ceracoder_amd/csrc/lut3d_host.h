/* lut3d_host.h -- the rule of the 3D colour LUT step in plain C, all integers: what the host entry points of the ABI
 * (mi355enc_lut3d_*), the handle (enc_lut3d.cpp) and the kernel (k_lut3d.hip) share.  No device needed. */
#ifndef MI355_LUT3D_HOST_H
#define MI355_LUT3D_HOST_H
#include <stdint.h>

#define LUT3D_N_MIN 2
#define LUT3D_N_MAX 65
#define LUT3D_STAGED_FIT 34 /* the largest N whose table a workgroup can hold in LDS: 34^3 words are 157 216 of the CU's 163 840 bytes */
#define LUT3D_STAGED_TO 34  /* mi355enc_lut3d_plan: up to this N the staged form runs (profiles/lut3d_price.md) */
#define LUT3D_COEF_WORDS 19/* Minv (9, row-major: R, G, B from Y - yoff, Cb - 128, Cr - 128), Mf (9: Y, Cb, Cr from R, G, B), yoff */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LUT3D_FN static __host__ __device__ inline
#else
#define LUT3D_FN static inline
#endif

LUT3D_FN int lut3d_clip(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
/* v >> s as a floor: on the host whatever the compiler makes of a negative left operand, on the device the arithmetic shift it is */
#if defined(__HIP_DEVICE_COMPILE__)
LUT3D_FN int lut3d_shr(int v, int s) { return v >> s; }
#else
LUT3D_FN int lut3d_shr(int v, int s) { return v >= 0 ? v >> s : -((-v + (1 << s) - 1) >> s); }
#endif

/* step 1: one of R', G', B' in Q12 (0 .. 4096) from a row of Minv and v = (Y - yoff, Cb - 128, Cr - 128) */
LUT3D_FN int lut3d_rgb(const int *row, int vy, int vu, int vv) { return lut3d_clip(lut3d_shr(row[0] * vy + row[1] * vu + row[2] * vv + (1 << 13), 14), 0, 4096); }

/* steps 2 and 3.  lut3d_cell: from R', G', B' in Q12 the four nodes of the tetrahedron (indices into the table) and their weights (sum 4096).  The walk goes
 * from the cell's lowest node one step at a time along the axes in the order of the fractions, largest first; with equal fractions the node between them has
 * weight 0, so the order among equals (stated as R, G, B) never shows in the result.  lut3d_blend: the graded sample as a packed word (R | G << 10 | B << 20) */
LUT3D_FN void lut3d_cell(int N, int cr, int cg, int cb, int *idx, int *w) {
    const int pr = cr * (N - 1), pg = cg * (N - 1), pb = cb * (N - 1);
    const int ir = (pr >> 12) < N - 2 ? (pr >> 12) : N - 2, ig = (pg >> 12) < N - 2 ? (pg >> 12) : N - 2, ib = (pb >> 12) < N - 2 ? (pb >> 12) : N - 2;
    const int fr = pr - (ir << 12), fg = pg - (ig << 12), fb = pb - (ib << 12);
    const int base = ir + N * (ig + N * ib), sg = N, sb = N * N;
    int f0, f1, f2, s0, s1;
    if (fr >= fg) {
        if (fg >= fb) { f0 = fr; f1 = fg; f2 = fb; s0 = 1; s1 = sg; }
        else if (fr >= fb) { f0 = fr; f1 = fb; f2 = fg; s0 = 1; s1 = sb; }
        else { f0 = fb; f1 = fr; f2 = fg; s0 = sb; s1 = 1; }
    } else {
        if (fr >= fb) { f0 = fg; f1 = fr; f2 = fb; s0 = sg; s1 = 1; }
        else if (fg >= fb) { f0 = fg; f1 = fb; f2 = fr; s0 = sg; s1 = sb; }
        else { f0 = fb; f1 = fg; f2 = fr; s0 = sb; s1 = sg; }
    }
    idx[0] = base; idx[1] = base + s0; idx[2] = base + s0 + s1; idx[3] = base + 1 + sg + sb;
    w[0] = 4096 - f0; w[1] = f0 - f1; w[2] = f1 - f2; w[3] = f2;
}
LUT3D_FN uint32_t lut3d_blend(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const int *w) {
    uint32_t o = 0;
    for (int k = 0; k < 30; k += 10)
        o |= ((((a >> k) & 1023u) * (uint32_t)w[0] + ((b >> k) & 1023u) * (uint32_t)w[1] + ((c >> k) & 1023u) * (uint32_t)w[2] + ((d >> k) & 1023u) * (uint32_t)w[3] + 2048u) >> 12) << k;
    return o;
}

/* step 4, per graded sample g (packed): one of Mf's rows . g, without offset and shift */
LUT3D_FN int lut3d_dot(const int *row, uint32_t g) { return row[0] * (int)(g & 1023u) + row[1] * (int)((g >> 10) & 1023u) + row[2] * (int)(g >> 20); }
/* ... the luma sample, and a chroma sample from the sum over the quad's four samples */
LUT3D_FN int lut3d_luma(const int *coef, uint32_t g) { return lut3d_clip(lut3d_shr(lut3d_dot(coef + 9, g) + (coef[18] << 20) + (1 << 19), 20), 0, 255); }
LUT3D_FN int lut3d_chroma(int sum) { return lut3d_clip(lut3d_shr(sum + (128 << 22) + (1 << 21), 22), 0, 255); }
/* step 5 */
LUT3D_FN int lut3d_mix(int in, int graded, int strength) { return in + lut3d_shr((graded - in) * strength + 128, 8); }

#endif
