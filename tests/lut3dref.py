"""The 3D colour LUT step's rule (include/mi355enc.h states it) restated independently in numpy and Python integers: the coefficients from
exact fractions of this file's own KR_KB, the rule on NV12 planes, the .cube parser in int / fractions, a double-precision model of the same pipeline (float
matrices, float tetrahedral interpolation over unquantised nodes, one rounding at the end), and cube generators."""
import re
from fractions import Fraction

import numpy as np

KR_KB = {1: ("0.2126", "0.0722"), 5: ("0.299", "0.114"), 6: ("0.299", "0.114"), 9: ("0.2627", "0.0593")}
N_MIN, N_MAX = 2, 65


def _scales(full):
    return (255, 255, 0) if full else (219, 224, 16)


def _matrices(matrix, full):
    """(M^-1 from code differences to R'G'B' in 0 .. 1, M from R'G'B' to code differences), as Fractions"""
    kr, kb = (Fraction(s) for s in KR_KB[matrix])
    kg = 1 - kr - kb
    ys, cs, _ = _scales(full)
    minv = [[Fraction(1, ys), Fraction(0), 2 * (1 - kr) / cs],
            [Fraction(1, ys), -2 * kb * (1 - kb) / kg / cs, -2 * kr * (1 - kr) / kg / cs],
            [Fraction(1, ys), 2 * (1 - kb) / cs, Fraction(0)]]
    m = [[ys * kr, ys * kg, ys * kb],
         [-cs * kr / (2 * (1 - kb)), -cs * kg / (2 * (1 - kb)), Fraction(cs, 2)],
         [Fraction(cs, 2), -cs * kg / (2 * (1 - kr)), -cs * kb / (2 * (1 - kr))]]
    return minv, m


def _round(x):
    return int((x + Fraction(1, 2)).__floor__())


def coefficients(matrix, full):
    """The 19 words of mi355enc_lut3d_coefficients"""
    minv, m = _matrices(matrix, full)
    return [_round(v * 4096 * 2 ** 14) for row in minv for v in row] + [_round(v / 1023 * 2 ** 20) for row in m for v in row] + [_scales(full)[2]]


def _interp(nodes, N, c):
    """steps 2 and 3: c (..., 3) int64 in Q12 -> g (..., 3) ten-bit"""
    p = c * (N - 1)
    i = np.minimum(p >> 12, N - 2)
    f = p - (i << 12)
    order = np.argsort(-f, axis=-1, kind="stable")  # descending, ties in the order R, G, B
    fs = np.take_along_axis(f, order, axis=-1)
    stride = np.array([1, N, N * N], np.int64)
    base = (i * stride).sum(-1)
    n0 = base
    n1 = n0 + stride[order[..., 0]]
    n2 = n1 + stride[order[..., 1]]
    n3 = base + 1 + N + N * N
    w = [4096 - fs[..., 0], fs[..., 0] - fs[..., 1], fs[..., 1] - fs[..., 2], fs[..., 2]]
    tab = np.asarray(nodes, np.int64)
    out = []
    for k in (0, 10, 20):
        ch = (tab >> k) & 1023
        out.append((ch[n0] * w[0] + ch[n1] * w[1] + ch[n2] * w[2] + ch[n3] * w[3] + 2048) >> 12)
    return np.stack(out, -1)


def apply(nodes, N, strength, matrix, full, y, uv, rect=None, visible=None):
    """The rule on NV12 planes y (H x W) / uv (H / 2 x W) inside rect (x0, x1, y0, y1; all of it without) -> new (y, uv).  visible (w, h): the planes are coded
    surfaces with that visible size (rule 6): the rule runs on the rectangle's visible part, and where the rectangle reaches the surfaces' right (bottom) edge
    the margin beside (below) it becomes what with_margins makes of the graded visible picture -- luma the last visible column / row, chroma the last pair / row"""
    y, uv = np.array(y, np.uint8), np.array(uv, np.uint8)
    H, W = y.shape
    x0, x1, y0, y1 = rect if rect is not None else (0, W, 0, H)
    assert N_MIN <= N <= N_MAX and len(nodes) == N ** 3 and 0 <= strength <= 256 and not (x0 | x1 | y0 | y1) & 1
    if strength == 0:
        return y, uv
    if visible is not None:
        vw, vh = visible
        assert not (vw | vh) & 1 and x0 < vw and y0 < vh and (x1 <= vw or x1 == W) and (y1 <= vh or y1 == H)
        gy, guv = apply(nodes, N, strength, matrix, full, y, uv, (x0, min(x1, vw), y0, min(y1, vh)))
        if x1 > vw:  # the margin columns of the rectangle's visible rows
            gy[y0:min(y1, vh), vw:] = gy[y0:min(y1, vh), vw - 1:vw]
            c = guv.reshape(H // 2, W // 2, 2)
            c[y0 // 2:min(y1, vh) // 2, vw // 2:] = c[y0 // 2:min(y1, vh) // 2, vw // 2 - 1:vw // 2]
        if y1 > vh:  # the margin rows, of the rectangle's columns and of the margin columns just written: the corner is both
            xe = W if x1 > vw else x1
            gy[vh:, x0:xe] = gy[vh - 1:vh, x0:xe]
            guv[vh // 2:, x0:xe] = guv[vh // 2 - 1:vh // 2, x0:xe]
        return gy, guv
    co = coefficients(matrix, full)
    minv, mf, yoff = np.array(co[:9], np.int64).reshape(3, 3), np.array(co[9:18], np.int64).reshape(3, 3), co[18]
    Y = y[y0:y1, x0:x1].astype(np.int64)
    qh, qw = (y1 - y0) // 2, (x1 - x0) // 2
    C = uv[y0 // 2:y1 // 2, x0:x1].astype(np.int64).reshape(qh, qw, 2)
    Yq = Y.reshape(qh, 2, qw, 2).transpose(0, 2, 1, 3).reshape(qh, qw, 4)  # the quad's four samples
    v = np.stack([Yq - yoff, np.broadcast_to(C[..., None, 0] - 128, Yq.shape), np.broadcast_to(C[..., None, 1] - 128, Yq.shape)], -1)  # (qh, qw, 4, 3)
    c = np.clip((v @ minv.T + (1 << 13)) >> 14, 0, 4096)
    g = _interp(nodes, N, c)
    t = g @ mf.T  # (qh, qw, 4, 3)
    Yg = np.clip((t[..., 0] + (yoff << 20) + (1 << 19)) >> 20, 0, 255)
    Cg = np.clip((t[..., 1:].sum(2) + (128 << 22) + (1 << 21)) >> 22, 0, 255)
    Yo = Yq + (((Yg - Yq) * strength + 128) >> 8)
    Co = C + (((Cg - C) * strength + 128) >> 8)
    y[y0:y1, x0:x1] = Yo.reshape(qh, qw, 2, 2).transpose(0, 2, 1, 3).reshape(y1 - y0, x1 - x0)
    uv[y0 // 2:y1 // 2, x0:x1] = Co.reshape(qh, 2 * qw)
    return y, uv


def model(cube, N, matrix, full, y, uv):
    """The double-precision model at full strength over the whole picture: cube (N^3, 3) floats, red fastest -> (y, uv) as floats before the one rounding, and rounded"""
    minv, m = _matrices(matrix, full)
    minv, m = np.array(minv, np.float64), np.array(m, np.float64)
    yoff = _scales(full)[2]
    H, W = np.shape(y)
    Y = np.asarray(y, np.float64)
    C = np.asarray(uv, np.float64).reshape(H // 2, W // 2, 2)
    Cb, Cr = (np.repeat(np.repeat(C[..., k], 2, 0), 2, 1) - 128.0 for k in (0, 1))
    rgb = np.clip(np.stack([Y - yoff, Cb, Cr], -1) @ minv.T, 0.0, 1.0)
    p = rgb * (N - 1)
    i = np.minimum(np.floor(p).astype(np.int64), N - 2)
    f = p - i
    order = np.argsort(-f, axis=-1, kind="stable")
    fs = np.take_along_axis(f, order, axis=-1)
    stride = np.array([1, N, N * N], np.int64)
    base = (i * stride).sum(-1)
    n1 = base + stride[order[..., 0]]
    n2 = n1 + stride[order[..., 1]]
    n3 = base + 1 + N + N * N
    cube = np.asarray(cube, np.float64)
    g = (cube[base] * (1 - fs[..., :1]) + cube[n1] * (fs[..., :1] - fs[..., 1:2]) + cube[n2] * (fs[..., 1:2] - fs[..., 2:3]) + cube[n3] * fs[..., 2:3])
    t = g @ m.T
    yf = t[..., 0] + yoff
    cf = t[..., 1:].reshape(H // 2, 2, W // 2, 2, 2).mean(axis=(1, 3)) + 128.0
    return np.clip(np.floor(yf + 0.5), 0, 255).astype(np.uint8), np.clip(np.floor(cf.reshape(H // 2, W) + 0.5), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ cubes: (N^3, 3) floats, red fastest
def _grid(N):
    a = np.arange(N, dtype=np.float64) / (N - 1)
    b, g, r = np.meshgrid(a, a, a, indexing="ij")
    return np.stack([r, g, b], -1).reshape(-1, 3)


def cube_identity(N):
    return _grid(N)


def cube_invert(N):
    return 1.0 - _grid(N)


def cube_gamma_sat(N, gamma=0.45, sat=1.3):
    v = _grid(N) ** gamma
    luma = v @ np.array([0.2126, 0.7152, 0.0722])
    return np.clip(luma[:, None] + sat * (v - luma[:, None]), 0.0, 1.0)


def cube_log(N, k=4.0):
    """an exponential curve, as a camera-log-to-display cube has it"""
    return (np.exp(k * _grid(N)) - 1.0) / (np.exp(k) - 1.0)


def cube_noise(N, seed):
    return np.random.default_rng(seed).random((N ** 3, 3))


NAMED = {"identity": cube_identity, "invert": cube_invert, "gamma_sat": cube_gamma_sat, "log": cube_log}


def quantise(cube):
    q = np.clip(np.floor(np.asarray(cube, np.float64) * 1023.0 + 0.5), 0, 1023).astype(np.uint32)
    return q[:, 0] | q[:, 1] << 10 | q[:, 2] << 20


def identity(N):
    """mi355enc_lut3d_identity, in integers"""
    q = np.array([(2 * i * 1023 + (N - 1)) // (2 * (N - 1)) for i in range(N)], np.uint32)
    b, g, r = np.meshgrid(q, q, q, indexing="ij")
    return (r | g << 10 | b << 20).reshape(-1)


def check(nodes, N):
    return N_MIN <= N <= N_MAX and len(nodes) == N ** 3 and not (np.asarray(nodes, np.uint32) >> 30).any()


# ------------------------------------------------------------------ the .cube parser
_NUM = re.compile(r"([+-]?)(?:(\d+)(?:\.(\d*))?|\.(\d+))(?:[eE]([+-]?\d+))?\Z")
UNIT = 10 ** 9


def _number(tok):
    """a decimal in units of 10^-9, the magnitude's further digits truncated; ValueError for anything else and for |value| >= 10^6"""
    m = _NUM.match(tok)
    if not m or not tok.isascii():
        raise ValueError("not a number: %r" % tok)
    sign, ip, fp, fp2, ex = m.groups()
    frac = fp2 if ip is None else (fp or "")
    mag = Fraction(int((ip or "") + frac or "0"), 10 ** len(frac)) * Fraction(10) ** int(ex or 0)
    if mag >= 10 ** 6:
        raise ValueError("too large: %r" % tok)
    units = int(mag * UNIT)
    return -units if sign == "-" else units


def parse_cube(text, cap=None):
    """(nodes, N) of a .cube text (bytes or str); ValueError where mi355enc_lut3d_parse_cube refuses"""
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    lo, hi, N, rows = [0, 0, 0], [UNIT] * 3, 0, []
    for line in text.split("\n"):
        if line.endswith("\r"):
            line = line[:-1]
        tok = [t for t in re.split(r"[ \t]+", line) if t]
        if not tok or tok[0].startswith("#"):
            continue
        if tok[0][0].isascii() and tok[0][0].isalpha():
            if rows:
                raise ValueError("keyword behind the rows")
            if tok[0] == "TITLE":
                continue
            vals = [_number(t) for t in tok[1:]]
            if tok[0] == "LUT_3D_SIZE":
                if N or len(vals) != 1 or vals[0] % UNIT or not N_MIN * UNIT <= vals[0] <= N_MAX * UNIT:
                    raise ValueError("size")
                N = vals[0] // UNIT
                if cap is not None and N ** 3 > cap:
                    raise ValueError("capacity")
            elif tok[0] in ("DOMAIN_MIN", "DOMAIN_MAX"):
                if len(vals) != 3:
                    raise ValueError("domain")
                (lo if tok[0] == "DOMAIN_MIN" else hi)[:] = vals
            elif tok[0] == "LUT_3D_INPUT_RANGE":
                if len(vals) != 2 or vals != [0, UNIT]:
                    raise ValueError("input range")
            else:
                raise ValueError("keyword %r" % tok[0])
            continue
        vals = [_number(t) for t in tok]
        if not N or len(rows) >= N ** 3 or len(vals) != 3:
            raise ValueError("row")
        word = 0
        for c in range(3):
            d = hi[c] - lo[c]
            if d <= 0:
                raise ValueError("domain")
            q = min(max(Fraction((vals[c] - lo[c]) * 2046 + d, 2 * d), 0).__floor__(), 1023)
            word |= q << (10 * c)
        rows.append(word)
    if not N or len(rows) != N ** 3 or any(h <= l for l, h in zip(lo, hi)):
        raise ValueError("rows")
    return np.array(rows, np.uint32), N


def cube_text(cube, N, title="generated", eol="\n"):
    lines = ['TITLE "%s"' % title, "LUT_3D_SIZE %d" % N] + ["%.6f %.6f %.6f" % tuple(r) for r in np.asarray(cube)]
    return eol.join(lines) + eol
