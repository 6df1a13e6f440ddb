"""numpy restatement of DESIGN.md section 22: HDR input (PQ / HLG, BT.2020 non-constant luminance, 10 bits) tone-mapped to 8-bit SDR Y'CbCr.

Two things live here.  The MODEL, in IEEE double: what the conversion means (model_rgb, model_out).  The RULE, in numpy integers: what the device computes
(rule_rgb, rule_out, tone_map_nv12), driven by the parameter block that mi355enc_hdr_tables exports, so that "kernel == rule" is exact even where the C
library's pow and numpy's differ in the last place.  build_block makes the same block in numpy from the model, for comparison with the exported one.

The model.  Input codes (Y, Cb, Cr), limited range: ey = (Y - 64) / 876, eb = (Cb - 512) / 896, er = (Cr - 512) / 896 (full range: Y / 1023, (C - 512) / 1023);
R' = ey + 2 (1 - Kr) er, B' = ey + 2 (1 - Kb) eb, G' = (ey - Kr R' - Kb B') / Kg with Kr = 0.2627, Kb = 0.0593; each clipped to [0, 1].
  PQ:  L = min(Lp, 10000 (max(p - c1, 0) / (c2 - c3 p))^(1 / m1)), p = E'^(1 / m2)                                  (SMPTE ST 2084)
  HLG: E = E'^2 / 3 for E' <= 1/2, else (exp((E' - c) / a) + b) / 12, clipped to 1; Ys = 0.2627 R + 0.6780 G + 0.0593 B;
       L = Lw Ys^(g - 1) E, g = 1.2 + 0.42 log10(Lw / 1000), Lw = Lp                                                 (BT.2100)
  tone curve on n = max(R, G, B) of L: e1 = PQ^-1(n) / PQ^-1(Lp), maxLum = PQ^-1(Lt) / PQ^-1(Lp), KS = 1.5 maxLum - 0.5,
       e2 = e1 below KS, else the Hermite spline (2t^3 - 3t^2 + 1) KS + (t^3 - 2t^2 + t)(1 - KS) + (-2t^3 + 3t^2) maxLum, t = (e1 - KS) / (1 - KS);
       EETF(n) = PQ(e2 PQ^-1(Lp)); every component times EETF(n) / n; identity when Lt >= Lp                         (BT.2390 section 5.4.1, Lmin = 0)
  gamut: the 3 x 3 matrix BT.2020 -> BT.709 (gamut_matrix), the result over Lt, clipped to [0, 1]
  OETF: 4.5 L below 0.018, else 1.099 L^0.45 - 0.099                                                                  (BT.709)
  out: Y' = oy + Ys (Kr' R' + Kg' G' + Kb' B'), Cb = 128 + Cs (B' - Y'lin) / (2 (1 - Kb')), Cr likewise; Ys = 219 | 255, Cs = 224 | 255, oy = 16 | 0;
       a 4:2:0 chroma pair from the mean R'G'B' of its four samples.

The rule (every word of the block is an int32; r(x) = floor(x + 0.5) in double).  Header, word index: 0 layout version (1), 1 transfer, 2 input full range,
3 Lp, 4 Lt, 5 output matrix, 6 output full range, 7 words in all, 8 oy_in, 9 cy, 10 rv, 11 gu, 12 gv, 13 bu (2^-28 per code), 14-16 the HLG luminance
weights (2^-16), 17-25 the gamut matrix by rows (2^-20), 26-28 yr yg yb, 29-31 br bg bb, 32-34 rr rg rb (2^-14 of a code per unit), 35 oy_out, 36-39 zero.
Then LIN (4097 words, 2^-28 of Lp or of scene 1.0 over the non-linear code in 2^-12 steps), GA (1282 words, the HLG OOTF gain Ys^(g - 1) in 2^-30),
GB (1282 words, the tone gain EETF(n) / n Lp / Lt in 2^-24), OE (1025 words, the OETF in 2^-16 over 2^-10 steps).  GA and GB are spaced by octaves:
entry 64 o + m stands for s = (64 + m) << (o + 2), o = 0 .. 19, entry 1280 for 2^28, entry 1281 repeats it.
  y = Y - oy_in, u = Cb - 512, v = Cr - 512
  tR = cy y + rv v, tG = cy y + gu u + gv v, tB = cy y + bu u                          (int32)
  x = clip((t + 8) >> 4, 0, 2^24); k = min(x >> 12, 4095), f = x - (k << 12)
  l = LIN[k] + (((LIN[k + 1] - LIN[k]) f + 2^11) >> 12)                               (the product in int64, l int32)
  HLG: ys = (lr lR + lg lG + lb lB + 2^15) >> 16 (int64 sum); g1 = gain(GA, ys); v_i = (l_i g1 + 2^29) >> 30.   PQ: v_i = l_i
  n = max v_i; g2 = gain(GB, n); w_i = (v_i g2 + 2^23) >> 24                           (products int64, w int32)
  u_i = clip((sum_j M_ij w_j + 2^19) >> 20, 0, 2^28)                                   (sum int64)
  k = min(u >> 18, 1023), f = u - (k << 18); E_i = OE[k] + (((OE[k + 1] - OE[k]) f + 2^17) >> 18)   (int32)
  Y8 = clip255((yr R + yg G + yb B + (oy_out << 30) + 2^29) >> 30)                     (int64)
  with S_i the sum of E_i over the four samples of a chroma pair: Cb8 = clip255((br SR + bg SG + bb SB + (128 << 32) + 2^31) >> 32), Cr8 likewise
  gain(T, s): s = min(s, 2^28); below 256: T[0]; else e = floor(log2 s), sh = e - 6, q = s >> sh, i = 64 (e - 8) + q - 64, f = s - (q << sh),
              T[i] + (((T[i + 1] - T[i]) f + (1 << (sh - 1))) >> sh)                   (product int64)
A luma sample uses the chroma pair of its own 2 x 2 block; v210's 4:2:2 chroma is first averaged over the block's two rows, (a + b + 1) >> 1.
"""
import math

import numpy as np

from oracle.csc import _pad
from tests import yuvref as YR

FMT_P010, FMT_I420_10, FMT_V210 = 14, 15, 16
PQ, HLG = 16, 18
M1, M2, C1, C2, C3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
HLG_A, HLG_B, HLG_C = 0.17883277, 0.28466892, 0.55991073
KR, KB = 0.2627, 0.0593
LUMA2020 = (0.2627, 0.6780, 0.0593)
OUT_K = {1: (0.2126, 0.0722), 5: (0.299, 0.114), 6: (0.299, 0.114)}

HDR_WORDS, LIN_N, GAIN_N, OE_N = 40, 4097, 1282, 1025
LIN_AT, GA_AT, GB_AT, OE_AT = HDR_WORDS, HDR_WORDS + LIN_N, HDR_WORDS + LIN_N + GAIN_N, HDR_WORDS + LIN_N + 2 * GAIN_N
BLOCK_WORDS = OE_AT + OE_N
ONE28, ONE24 = 1 << 28, 1 << 24


# ---------------------------------------------------------------- the model
def pq_eotf(e):
    """non-linear PQ signal [0, 1] -> cd/m^2"""
    p = np.power(np.asarray(e, np.float64), 1.0 / M2)
    return 10000.0 * np.power(np.maximum(p - C1, 0.0) / (C2 - C3 * p), 1.0 / M1)


def pq_inv(l):
    """cd/m^2 -> non-linear PQ signal"""
    y = np.power(np.asarray(l, np.float64) / 10000.0, M1)
    return np.power((C1 + C2 * y) / (1.0 + C3 * y), M2)


def hlg_inv_oetf(x):
    x = np.asarray(x, np.float64)
    return np.minimum(1.0, np.where(x <= 0.5, x * x / 3.0, (np.exp((x - HLG_C) / HLG_A) + HLG_B) / 12.0))


def hlg_gamma(lw):
    return 1.2 + 0.42 * math.log10(lw / 1000.0)


def eetf(n, lp, lt):
    """the tone curve: display light of a source with peak lp -> display light of a target with peak lt"""
    n = np.asarray(n, np.float64)
    if lt >= lp:
        return n
    pw = float(pq_inv(lp))
    maxlum = float(pq_inv(lt)) / pw
    ks = 1.5 * maxlum - 0.5
    e1 = pq_inv(n) / pw
    t = np.maximum((e1 - ks) / (1.0 - ks), 0.0)
    p = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1.0 - ks) + (-2 * t ** 3 + 3 * t ** 2) * maxlum
    return np.where(e1 < ks, n, pq_eotf(np.minimum(p, maxlum) * pw))


def tone_gain(n, lp, lt):
    n = np.asarray(n, np.float64)
    safe = np.where(n > 0, n, 1.0)
    return np.where(n > 0, eetf(safe, lp, lt) / safe, 1.0)


def _xyz(prim):
    """RGB -> XYZ of a set of primaries with white D65, by rows (plain scalar arithmetic, the order ceracoder_amd/csrc/hdr_host.c follows)"""
    (xr, yr), (xg, yg), (xb, yb) = prim
    xw, yw = 0.3127, 0.3290
    X = [xr / yr, xg / yg, xb / yb]
    Z = [(1.0 - xr - yr) / yr, (1.0 - xg - yg) / yg, (1.0 - xb - yb) / yb]
    m = [X, [1.0, 1.0, 1.0], Z]
    w = [xw / yw, 1.0, (1.0 - xw - yw) / yw]
    inv = _inv3(m)
    s = [inv[i][0] * w[0] + inv[i][1] * w[1] + inv[i][2] * w[2] for i in range(3)]
    return [[m[i][j] * s[j] for j in range(3)] for i in range(3)]


def _inv3(m):
    a, b, c = m[0]
    d, e, f = m[1]
    g, h, i = m[2]
    co = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * co[0][0] + b * co[1][0] + c * co[2][0]
    return [[co[r][k] / det for k in range(3)] for r in range(3)]


def gamut_matrix():
    """linear BT.2020 RGB -> linear BT.709 RGB, from the chromaticities of the two sets of primaries and D65"""
    a = _xyz(((0.708, 0.292), (0.170, 0.797), (0.131, 0.046)))
    b = _inv3(_xyz(((0.64, 0.33), (0.30, 0.60), (0.15, 0.06))))
    return [[b[i][0] * a[0][j] + b[i][1] * a[1][j] + b[i][2] * a[2][j] for j in range(3)] for i in range(3)]


def oetf709(l):
    l = np.asarray(l, np.float64)
    return np.where(l < 0.018, 4.5 * l, 1.099 * np.power(np.maximum(l, 0.018), 0.45) - 0.099)


def resolve(peak, target):
    return (peak or 1000), (target or 203)


def model_light(transfer, full, peak, y, cb, cr):
    """10-bit codes -> display light (R, G, B) in cd/m^2, before the tone curve"""
    y, cb, cr = (np.asarray(v, np.float64) for v in (y, cb, cr))
    ey, eb, er = (y / 1023.0, (cb - 512.0) / 1023.0, (cr - 512.0) / 1023.0) if full else ((y - 64.0) / 876.0, (cb - 512.0) / 896.0, (cr - 512.0) / 896.0)
    r = ey + 2.0 * (1.0 - KR) * er
    b = ey + 2.0 * (1.0 - KB) * eb
    g = (ey - KR * r - KB * b) / (1.0 - KR - KB)
    r, g, b = (np.clip(v, 0.0, 1.0) for v in (r, g, b))
    if transfer == PQ:
        return tuple(np.minimum(pq_eotf(v), float(peak)) for v in (r, g, b))
    e = [hlg_inv_oetf(v) for v in (r, g, b)]
    ys = LUMA2020[0] * e[0] + LUMA2020[1] * e[1] + LUMA2020[2] * e[2]
    gain = float(peak) * np.power(ys, hlg_gamma(peak) - 1.0)
    return tuple(gain * v for v in e)


def model_rgb(transfer, full, peak, target, y, cb, cr):
    """10-bit codes -> non-linear BT.709 R'G'B' in [0, 1]"""
    peak, target = resolve(peak, target)
    l = model_light(transfer, full, peak, y, cb, cr)
    t = tone_gain(np.maximum(np.maximum(l[0], l[1]), l[2]), peak, target)
    l = [v * t for v in l]
    m = gamut_matrix()
    return tuple(oetf709(np.clip((m[i][0] * l[0] + m[i][1] * l[1] + m[i][2] * l[2]) / float(target), 0.0, 1.0)) for i in range(3))


def model_out(out_matrix, out_full, r, g, b):
    """R'G'B' -> unrounded 8-bit Y', Cb, Cr"""
    kr, kb = OUT_K[out_matrix]
    ys, cs, oy = (255.0, 255.0, 0.0) if out_full else (219.0, 224.0, 16.0)
    yl = kr * r + (1.0 - kr - kb) * g + kb * b
    return oy + ys * yl, 128.0 + cs * (b - yl) / (2.0 * (1.0 - kb)), 128.0 + cs * (r - yl) / (2.0 * (1.0 - kr))


# ---------------------------------------------------------------- the block, built in numpy from the model
def _r(x):
    return int(math.floor(x + 0.5))


def gain_points():
    """the values s the entries of a gain table stand for"""
    s = [(64 + m) << (o + 2) for o in range(20) for m in range(64)] + [ONE28, ONE28]
    return np.array(s, np.float64)


def build_block(transfer, full, peak, target, out_matrix, out_full):
    peak, target = resolve(peak, target)
    b = np.zeros(BLOCK_WORDS, np.int64)
    b[0:8] = [1, transfer, full, peak, target, out_matrix, out_full, BLOCK_WORDS]
    ysc, csc = (1023.0, 1023.0) if full else (876.0, 896.0)
    kg = 1.0 - KR - KB
    b[8] = 0 if full else 64
    b[9] = _r(268435456.0 / ysc)
    b[10] = _r(2.0 * (1.0 - KR) * 268435456.0 / csc)
    b[11] = -_r(2.0 * (1.0 - KB) * KB / kg * 268435456.0 / csc)
    b[12] = -_r(2.0 * (1.0 - KR) * KR / kg * 268435456.0 / csc)
    b[13] = _r(2.0 * (1.0 - KB) * 268435456.0 / csc)
    b[14], b[16] = _r(LUMA2020[0] * 65536.0), _r(LUMA2020[2] * 65536.0)
    b[15] = 65536 - b[14] - b[16]
    m = gamut_matrix()
    for i in range(3):
        for j in range(3):
            if i != j:
                b[17 + 3 * i + j] = _r(m[i][j] * 1048576.0)
        b[17 + 4 * i] = 1048576 - sum(b[17 + 3 * i + j] for j in range(3) if j != i)
    kr, kb = OUT_K[out_matrix]
    ys, cs = (255.0, 255.0) if out_full else (219.0, 224.0)
    b[26], b[28] = _r(kr * ys * 16384.0), _r(kb * ys * 16384.0)
    b[27] = _r(ys * 16384.0) - b[26] - b[28]
    b[31] = _r(0.5 * cs * 16384.0); b[29] = -_r(kr / (2.0 * (1.0 - kb)) * cs * 16384.0); b[30] = -b[31] - b[29]
    b[32] = _r(0.5 * cs * 16384.0); b[34] = -_r(kb / (2.0 * (1.0 - kr)) * cs * 16384.0); b[33] = -b[32] - b[34]
    b[35] = 0 if out_full else 16
    x = np.arange(LIN_N) / 4096.0
    lin = np.minimum(pq_eotf(x), float(peak)) / float(peak) if transfer == PQ else hlg_inv_oetf(x)
    b[LIN_AT:LIN_AT + LIN_N] = np.floor(lin * 268435456.0 + 0.5)
    s = gain_points() / 268435456.0
    b[GA_AT:GA_AT + GAIN_N] = np.floor(np.power(s, hlg_gamma(peak) - 1.0) * 1073741824.0 + 0.5) if transfer == HLG else 1 << 30
    b[GB_AT:GB_AT + GAIN_N] = np.floor(tone_gain(s * peak, peak, target) * (float(peak) / float(target)) * 16777216.0 + 0.5)
    b[OE_AT:OE_AT + OE_N] = np.floor(oetf709(np.arange(OE_N) / 1024.0) * 65536.0 + 0.5)
    return b.astype(np.int32)


# ---------------------------------------------------------------- the rule
class Shadow:
    """the largest magnitude every named intermediate of the rule took (numpy int64 shadows), against the type section 22 names for it"""
    TYPES = {"t": 31, "x": 31, "lin_prod": 63, "l": 31, "ys_sum": 63, "ys": 31, "gain_prod": 63, "gain": 31, "v_prod": 63, "v": 31, "w_prod": 63, "w": 31,
             "u_sum": 63, "u": 31, "oe_prod": 31, "e": 31, "y_sum": 63, "c_sum": 63}

    def __init__(self):
        self.peak = {}

    def see(self, name, a):
        a = np.asarray(a)
        if a.size:
            self.peak[name] = max(self.peak.get(name, 0), int(np.max(np.abs(a))))

    def fits(self):
        return {k: v < (1 << self.TYPES[k]) for k, v in self.peak.items()}


def _gain(tab, s, sh_):
    s = np.minimum(s, ONE28)
    big = np.maximum(s, 256)
    e = np.floor(np.log2(big.astype(np.float64))).astype(np.int64)
    e = np.where((1 << e) > big, e - 1, np.where((1 << (e + 1)) <= big, e + 1, e))  # (exact whatever log2 rounds to)
    sh = e - 6
    q = big >> sh
    i = 64 * (e - 8) + q - 64
    f = big - (q << sh)
    prod = (tab[i + 1] - tab[i]) * f + (1 << (sh - 1))
    g = np.where(s < 256, tab[0], tab[i] + (prod >> sh))
    if sh_ is not None:
        sh_.see("gain_prod", prod)
        sh_.see("gain", g)
    return g


def rule_rgb(block, y, cb, cr, shadow=None):
    """10-bit codes -> (R, G, B) non-linear BT.709 in 2^-16 units, int64 arrays"""
    b = np.asarray(block).astype(np.int64)
    see = shadow.see if shadow is not None else (lambda *a: None)
    y, u, v = np.asarray(y, np.int64) - b[8], np.asarray(cb, np.int64) - 512, np.asarray(cr, np.int64) - 512
    t = [b[9] * y + b[10] * v, b[9] * y + b[11] * u + b[12] * v, b[9] * y + b[13] * u]
    lin, l = b[LIN_AT:LIN_AT + LIN_N], []
    for ti in t:
        see("t", ti)
        x = np.clip((ti + 8) >> 4, 0, ONE24)
        see("x", x)
        k = np.minimum(x >> 12, 4095)
        f = x - (k << 12)
        prod = (lin[k + 1] - lin[k]) * f + 2048
        see("lin_prod", prod)
        l.append(lin[k] + (prod >> 12))
        see("l", l[-1])
    if b[1] == HLG:
        ysum = b[14] * l[0] + b[15] * l[1] + b[16] * l[2] + 32768
        see("ys_sum", ysum)
        ys = ysum >> 16
        see("ys", ys)
        g1 = _gain(b[GA_AT:GA_AT + GAIN_N], ys, shadow)
        vv = []
        for li in l:
            prod = li * g1 + (1 << 29)
            see("v_prod", prod)
            vv.append(prod >> 30)
    else:
        vv = l
    for vi in vv:
        see("v", vi)
    n = np.maximum(np.maximum(vv[0], vv[1]), vv[2])
    g2 = _gain(b[GB_AT:GB_AT + GAIN_N], n, shadow)
    w = []
    for vi in vv:
        prod = vi * g2 + (1 << 23)
        see("w_prod", prod)
        w.append(prod >> 24)
        see("w", w[-1])
    oe, out = b[OE_AT:OE_AT + OE_N], []
    for i in range(3):
        usum = b[17 + 3 * i] * w[0] + b[18 + 3 * i] * w[1] + b[19 + 3 * i] * w[2] + (1 << 19)
        see("u_sum", usum)
        uu = np.clip(usum >> 20, 0, ONE28)
        see("u", uu)
        k = np.minimum(uu >> 18, 1023)
        f = uu - (k << 18)
        prod = (oe[k + 1] - oe[k]) * f + (1 << 17)
        see("oe_prod", prod)
        out.append(oe[k] + (prod >> 18))
        see("e", out[-1])
    return tuple(out)


def rule_luma(block, r, g, b_, shadow=None):
    b = np.asarray(block).astype(np.int64)
    s = b[26] * r + b[27] * g + b[28] * b_ + (b[35] << 30) + (1 << 29)
    if shadow is not None:
        shadow.see("y_sum", s)
    return np.clip(s >> 30, 0, 255)


def rule_chroma(block, sr, sg, sb, shadow=None):
    """from the sums of R, G, B over the four samples of a pair"""
    b = np.asarray(block).astype(np.int64)
    cb = b[29] * sr + b[30] * sg + b[31] * sb + (128 << 32) + (1 << 31)
    cr = b[32] * sr + b[33] * sg + b[34] * sb + (128 << 32) + (1 << 31)
    if shadow is not None:
        shadow.see("c_sum", cb)
        shadow.see("c_sum", cr)
    return np.clip(cb >> 32, 0, 255), np.clip(cr >> 32, 0, 255)


def rule_out(block, y, cb, cr, shadow=None):
    """a flat area of one (Y, Cb, Cr): the 8-bit (Y', Cb, Cr) the rule gives"""
    r, g, b = rule_rgb(block, y, cb, cr, shadow)
    c = rule_chroma(block, 4 * r, 4 * g, 4 * b, shadow)
    return rule_luma(block, r, g, b, shadow), c[0], c[1]


def unpack10(fmt, planes, w, h):
    """-> 10-bit Y (h, w), Cb, Cr (h / 2, w / 2) as the rule reads them"""
    if fmt == FMT_P010:
        return YR.unpack_p010(planes, w, h)
    if fmt == FMT_I420_10:
        return YR.unpack_i420_10(planes, w, h)
    y, u, v = YR.unpack_v210(planes[0], w, h)
    return y, (u[0::2] + u[1::2] + 1) >> 1, (v[0::2] + v[1::2] + 1) >> 1


def tone_map_nv12(block, fmt, planes, w, h):
    """-> the coded-size (multiples of 16) NV12 surfaces (Y, UV); the margin repeats the last visible row / column / chroma pair"""
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    y, cb, cr = unpack10(fmt, planes, w, h)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    r, g, b = rule_rgb(block, y, up(cb), up(cr))
    s4 = lambda a: a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    oy = rule_luma(block, r, g, b).astype(np.uint8)
    ocb, ocr = rule_chroma(block, s4(r), s4(g), s4(b))
    return _pad(np.ascontiguousarray(oy), H, W, False), _pad(YR._interleave(ocb.astype(np.uint8), ocr.astype(np.uint8)), H // 2, W, True)
