/* hdr_host.c -- the parameter block of the HDR tone map: the fixed-point matrices and the four tables the device's integer
 * rule reads, built once per handle in IEEE double.  tests/hdrref.py builds the same block in numpy from the model, operation for operation where the
 * words must be identical (the matrices: + - * / and floor only) and within one unit where libm's pow / exp / log10 take part.
 * No device, no allocation: the shim uploads the block, tests and the stand-alone driver look at it. */
#include "hdr_host.h"

#include <math.h>

/* no fused multiply-adds: the matrix words are bit for bit the restatement's */
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

static const double M1 = 2610.0 / 16384.0, M2 = 2523.0 / 4096.0 * 128.0, C1 = 3424.0 / 4096.0, C2 = 2413.0 / 4096.0 * 32.0, C3 = 2392.0 / 4096.0 * 32.0;
static const double HLG_A = 0.17883277, HLG_B = 0.28466892, HLG_C = 0.55991073;
static const double KR = 0.2627, KB = 0.0593; /* BT.2020: the matrix's and the scene luminance's weights (green: what is left of one) */

static double r_(double x) { return floor(x + 0.5); }
static double pq_eotf(double e) { /* non-linear signal -> cd/m^2 */
    const double p = pow(e, 1.0 / M2), n = p - C1;
    return 10000.0 * pow((n > 0.0 ? n : 0.0) / (C2 - C3 * p), 1.0 / M1);
}
static double pq_inv(double l) {
    const double y = pow(l / 10000.0, M1);
    return pow((C1 + C2 * y) / (1.0 + C3 * y), M2);
}
static double hlg_inv_oetf(double x) {
    const double e = x <= 0.5 ? x * x / 3.0 : (exp((x - HLG_C) / HLG_A) + HLG_B) / 12.0;
    return e < 1.0 ? e : 1.0;
}
/* BT.2390 section 5.4.1 with Lmin = 0, as a gain on display light: EETF(n) / n */
static double tone_gain(double n, double lp, double lt) {
    if (!(n > 0.0) || lt >= lp) return 1.0;
    const double pw = pq_inv(lp), maxlum = pq_inv(lt) / pw, ks = 1.5 * maxlum - 0.5, e1 = pq_inv(n) / pw;
    if (e1 < ks) return 1.0;
    const double t = (e1 - ks) / (1.0 - ks), t2 = t * t, t3 = t2 * t;
    double p = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (-2.0 * t3 + 3.0 * t2) * maxlum;
    if (p > maxlum) p = maxlum;
    return pq_eotf(p * pw) / n;
}
static double oetf709(double l) { return l < 0.018 ? 4.5 * l : 1.099 * pow(l, 0.45) - 0.099; }

static void inv3(const double m[3][3], double o[3][3]) {
    const double a = m[0][0], b = m[0][1], c = m[0][2], d = m[1][0], e = m[1][1], f = m[1][2], g = m[2][0], h = m[2][1], i = m[2][2];
    const double co[3][3] = {{e * i - f * h, c * h - b * i, b * f - c * e}, {f * g - d * i, a * i - c * g, c * d - a * f}, {d * h - e * g, b * g - a * h, a * e - b * d}};
    const double det = a * co[0][0] + b * co[1][0] + c * co[2][0];
    for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) o[r][k] = co[r][k] / det;
}
/* RGB -> XYZ of a set of primaries (x, y of R, G, B) with white D65 */
static void xyz_of(const double p[6], double o[3][3]) {
    const double xw = 0.3127, yw = 0.3290;
    const double m[3][3] = {{p[0] / p[1], p[2] / p[3], p[4] / p[5]}, {1.0, 1.0, 1.0}, {(1.0 - p[0] - p[1]) / p[1], (1.0 - p[2] - p[3]) / p[3], (1.0 - p[4] - p[5]) / p[5]}};
    const double w[3] = {xw / yw, 1.0, (1.0 - xw - yw) / yw};
    double inv[3][3], s[3];
    inv3(m, inv);
    for (int i = 0; i < 3; i++) s[i] = inv[i][0] * w[0] + inv[i][1] * w[1] + inv[i][2] * w[2];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) o[i][j] = m[i][j] * s[j];
}
static void gamut_matrix(double o[3][3]) {
    static const double p2020[6] = {0.708, 0.292, 0.170, 0.797, 0.131, 0.046}, p709[6] = {0.64, 0.33, 0.30, 0.60, 0.15, 0.06};
    double a[3][3], b0[3][3], b[3][3];
    xyz_of(p2020, a);
    xyz_of(p709, b0);
    inv3(b0, b);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) o[i][j] = b[i][0] * a[0][j] + b[i][1] * a[1][j] + b[i][2] * a[2][j];
}

int hdr_check(int transfer, int full_range, int peak, int target) {
    if ((transfer != 16 && transfer != 18) || (full_range | 1) != 1) return MI355ENC_ERR_ARG;
    if (peak != 0 && (peak < 400 || peak > (transfer == 16 ? 10000 : 2000))) return MI355ENC_ERR_ARG;
    if (target != 0 && (target < 100 || target > 400)) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

void hdr_build(int transfer, int full, int peak, int target, int out_matrix, int out_full, int32_t *b) {
    if (!peak) peak = 1000;
    if (!target) target = 203;
    for (int i = 0; i < HDR_HEAD; i++) b[i] = 0;
    b[0] = 1; b[1] = transfer; b[2] = full; b[3] = peak; b[4] = target; b[5] = out_matrix; b[6] = out_full; b[7] = HDR_WORDS;
    /* the input matrix, 2^-28 per code */
    const double ysc = full ? 1023.0 : 876.0, csc = full ? 1023.0 : 896.0, kg = 1.0 - KR - KB;
    b[8] = full ? 0 : 64;
    b[9] = (int32_t)r_(268435456.0 / ysc);
    b[10] = (int32_t)r_(2.0 * (1.0 - KR) * 268435456.0 / csc);
    b[11] = -(int32_t)r_(2.0 * (1.0 - KB) * KB / kg * 268435456.0 / csc);
    b[12] = -(int32_t)r_(2.0 * (1.0 - KR) * KR / kg * 268435456.0 / csc);
    b[13] = (int32_t)r_(2.0 * (1.0 - KB) * 268435456.0 / csc);
    /* the HLG scene luminance, 2^-16 */
    b[14] = (int32_t)r_(KR * 65536.0); b[16] = (int32_t)r_(KB * 65536.0); b[15] = 65536 - b[14] - b[16];
    /* BT.2020 -> BT.709 primaries, 2^-20, every row summing to one */
    double m[3][3];
    gamut_matrix(m);
    for (int i = 0; i < 3; i++) {
        int32_t off = 0;
        for (int j = 0; j < 3; j++) if (i != j) { b[17 + 3 * i + j] = (int32_t)r_(m[i][j] * 1048576.0); off += b[17 + 3 * i + j]; }
        b[17 + 4 * i] = 1048576 - off;
    }
    /* R'G'B' -> Y'CbCr, 2^-14 of a code per unit */
    const double kr = out_matrix == 1 ? 0.2126 : 0.299, kb = out_matrix == 1 ? 0.0722 : 0.114, ys = out_full ? 255.0 : 219.0, cs = out_full ? 255.0 : 224.0;
    b[26] = (int32_t)r_(kr * ys * 16384.0); b[28] = (int32_t)r_(kb * ys * 16384.0); b[27] = (int32_t)r_(ys * 16384.0) - b[26] - b[28];
    b[31] = (int32_t)r_(0.5 * cs * 16384.0); b[29] = -(int32_t)r_(kr / (2.0 * (1.0 - kb)) * cs * 16384.0); b[30] = -b[31] - b[29];
    b[32] = (int32_t)r_(0.5 * cs * 16384.0); b[34] = -(int32_t)r_(kb / (2.0 * (1.0 - kr)) * cs * 16384.0); b[33] = -b[32] - b[34];
    b[35] = out_full ? 0 : 16;
    /* linearisation over the non-linear code: display light over Lp (PQ), scene light (HLG), 2^-28 */
    const double lp = (double)peak, lt = (double)target;
    for (int i = 0; i < HDR_LIN_N; i++) {
        const double x = (double)i / 4096.0;
        double l;
        if (transfer == 16) { l = pq_eotf(x); l = (l < lp ? l : lp) / lp; }
        else l = hlg_inv_oetf(x);
        b[HDR_LIN_AT + i] = (int32_t)floor(l * 268435456.0 + 0.5);
    }
    /* the gains, by octaves: entry 64 o + m stands for s = (64 + m) << (o + 2) */
    const double gm1 = 1.2 + 0.42 * log10(lp / 1000.0) - 1.0;
    for (int i = 0; i < HDR_GAIN_N; i++) {
        const double s = (i >= 1280 ? 268435456.0 : (double)((int64_t)(64 + (i & 63)) << ((i >> 6) + 2))) / 268435456.0;
        b[HDR_GA_AT + i] = transfer == 18 ? (int32_t)floor(pow(s, gm1) * 1073741824.0 + 0.5) : 1 << 30;
        b[HDR_GB_AT + i] = (int32_t)floor(tone_gain(s * lp, lp, lt) * (lp / lt) * 16777216.0 + 0.5);
    }
    for (int i = 0; i < HDR_OE_N; i++) b[HDR_OE_AT + i] = (int32_t)floor(oetf709((double)i / 1024.0) * 65536.0 + 0.5);
}

int mi355enc_hdr_tables(int transfer, int full_range, int peak_nits, int target_nits, int out_matrix, int out_full, int32_t *out, size_t cap, size_t *n) {
    if (!n || hdr_check(transfer, full_range, peak_nits, target_nits) || (out_matrix != 1 && out_matrix != 5 && out_matrix != 6) || (out_full | 1) != 1) return MI355ENC_ERR_ARG;
    *n = HDR_WORDS;
    if (!out || cap < HDR_WORDS) return out ? MI355ENC_ERR_OVERFLOW : MI355ENC_OK; /* (out null: the size alone) */
    hdr_build(transfer, full_range, peak_nits, target_nits, out_matrix, out_full, out);
    return MI355ENC_OK;
}
