/* adjust_host.c -- the rule of the picture controls: argument ranges, the luma table and the chroma rotation of a parameter set.
 * Host only, no device needed; tests/adjustref.py restates it in numpy integers. */
#include "adjust_host.h"

#include <math.h>
#include <stddef.h>

static int clip255(long v) { return v < 0 ? 0 : v > 255 ? 255 : (int)v; }
/* floor(n / d), d > 0 */
static long floor_div(long n, long d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }

void mi355enc_adjust_default(mi355enc_adjust_t *a) {
    if (!a) return;
    a->brightness = 0; a->contrast = 1000; a->saturation = 1000; a->hue = 0; a->gamma = 1000; a->sharpen = 0; a->sharpen_threshold = 0;
}

int mi355enc_adjust_check(const mi355enc_adjust_t *a) {
    if (!a) return MI355ENC_ERR_ARG;
    if (a->brightness < -1000 || a->brightness > 1000 || a->contrast < 0 || a->contrast > 2000 || a->saturation < 0 || a->saturation > 2000 ||
        a->hue < -1000 || a->hue > 1000 || a->gamma < 100 || a->gamma > 10000 || a->sharpen < -16 || a->sharpen > 64 ||
        a->sharpen_threshold < 0 || a->sharpen_threshold > 32) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

int adjust_parts(const mi355enc_adjust_t *a) {
    /* (hue +-1000 turns the chroma plane by half a turn: not neutral; the threshold alone does nothing) */
    return (a->brightness != 0 || a->contrast != 1000 || a->gamma != 1000 ? ADJUST_LUMA : 0) | (a->saturation != 1000 || a->hue != 0 ? ADJUST_CHROMA : 0) |
           (a->sharpen != 0 ? ADJUST_SHARPEN : 0);
}

int mi355enc_adjust_tables(const mi355enc_adjust_t *a, int full_range, uint8_t luma[256], int32_t chroma[2]) {
    if (mi355enc_adjust_check(a) || (full_range | 1) != 1 || !luma || !chroma) return MI355ENC_ERR_ARG;
    const int B = full_range ? 0 : 16, S = full_range ? 255 : 219;
    if (a->gamma == 1000) { /* integers only */
        for (int v = 0; v < 256; v++)
            luma[v] = (uint8_t)clip255(B + floor_div(2L * ((long)(v - B) * a->contrast + (long)a->brightness * S) + 1000, 2000));
    } else {
        const double e = 1000.0 / (double)a->gamma;
        for (int v = 0; v < 256; v++) {
            double t = (double)(v - B) / (double)S;
            if (t >= 0.0 && t <= 1.0) t = pow(t, e); /* (foot- and headroom stay linear) */
            const double y = (double)B + (double)S * (t * (double)a->contrast / 1000.0 + (double)a->brightness / 1000.0);
            const double r = floor(y + 0.5);
            luma[v] = (uint8_t)(r < 0.0 ? 0 : r > 255.0 ? 255 : (int)r);
        }
        for (int v = 1; v < 256; v++) if (luma[v] < luma[v - 1]) luma[v] = luma[v - 1]; /* non-decreasing whatever pow()'s last bit does at a rounding tie */
    }
    const double g = 4096.0 * (double)a->saturation / 1000.0, ang = 3.14159265358979323846 * (double)a->hue / 1000.0;
    chroma[0] = (int32_t)lround(g * cos(ang));
    chroma[1] = (int32_t)lround(g * sin(ang));
    return MI355ENC_OK;
}
