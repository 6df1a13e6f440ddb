"""The mesh warp's rule restated in numpy, all integers (int64 throughout; >> and // are floors): the coefficient table, the builder, the
mesh interpolation and the whole picture, with the margin up to whole macroblocks by pad_kernel's rule.  What ceracoder_amd/csrc/warp_host.c and k_warp.hip are
compared against, bit for bit."""
import numpy as np

NODE_MIN, NODE_MAX = -2048 * 256, 10240 * 256
Q_MAX = 4194304  # (why not the 262144 first written down)
SIZES = [(72, 40), (64, 48), (96, 96), (160, 96)]
STRIPS = [(1936, 32), (32, 1100)]
NEUTRAL = dict(k1=0, k2=0, zoom=65536, cos=65536, sin=0, kh=0, kv=0)
RANGES = dict(k1=(-65536, 65536), k2=(-65536, 65536), zoom=(16384, 262144), cos=(-65536, 65536), sin=(-65536, 65536), kh=(-32768, 32768), kv=(-32768, 32768))
SETS = {
    "barrel": dict(k1=-13107, k2=1966),
    "roll": dict(cos=65454, sin=3276),
    "keystone": dict(kh=8192, kv=-8192),
    "all": dict(k1=-13107, k2=1966, zoom=60000, cos=65454, sin=3276, kh=8192, kv=-4096),
    "quarter": dict(cos=0, sin=65536),
    "shrink": dict(zoom=163840),
}


def mesh_size(w, h):
    return (w + 15) // 16 + 1, (h + 15) // 16 + 1


def taps(kind, f):
    if kind == 0:
        return [0, 4 * (32 - f), 4 * f, 0]
    a = (-f ** 3 + 64 * f ** 2 - 1024 * f + 256) >> 9
    c = (-3 * f ** 3 + 128 * f ** 2 + 1024 * f + 256) >> 9
    d = (f ** 3 - 32 * f ** 2 + 256) >> 9
    return [a, 128 - a - c - d, c, d]


TABLE = np.array([[taps(k, f) for f in range(32)] for k in (0, 1)], np.int64)


def build(w, h, **kw):
    """the mesh (ny, nx, 2) int32 of a parameter set, or None where the rule refuses it"""
    return build_why(w, h, **kw)[0]


def build_why(w, h, **kw):
    """(mesh, None), or (None, why the rule refuses the set: "range" -- a parameter outside its range -- "d", "q" or "node")"""
    p = dict(NEUTRAL, **kw)
    if w < 2 or h < 2 or any(not RANGES[n][0] <= p[n] <= RANGES[n][1] for n in RANGES):
        return None, "range"
    nx, ny = mesh_size(w, h)
    i, j = np.meshgrid(np.arange(nx, dtype=np.int64), np.arange(ny, dtype=np.int64))
    u, v = 32 * i - (w - 1), 32 * j - (h - 1)
    U = (p["zoom"] * (p["cos"] * u - p["sin"] * v)) >> 16
    V = (p["zoom"] * (p["sin"] * u + p["cos"] * v)) >> 16
    d = 65536 + (p["kh"] * U) // ((w - 1) << 16) + (p["kv"] * V) // ((h - 1) << 16)
    if (d < 16384).any():
        return None, "d"
    U, V = (U << 16) // d, (V << 16) // d
    r2 = ((U >> 8) ** 2 + (V >> 8) ** 2) >> 16
    q = (r2 << 16) // ((w - 1) ** 2 + (h - 1) ** 2)
    if (q > Q_MAX).any():
        return None, "q"
    g = 65536 + ((p["k1"] * q) >> 16) + ((p["k2"] * ((q * q) >> 16)) >> 16)
    sx = ((w - 1) * 65536 + ((U * g) >> 16) + 256) >> 9
    sy = ((h - 1) * 65536 + ((V * g) >> 16) + 256) >> 9
    m = np.stack([sx, sy], axis=-1)
    if (m < NODE_MIN).any() or (m > NODE_MAX).any():
        return None, "node"
    return m.astype(np.int32), None


def identity(w, h):
    nx, ny = mesh_size(w, h)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    return np.stack([4096 * i, 4096 * j], axis=-1).astype(np.int32)


def random_mesh(w, h, seed):
    """nodes anywhere inside the valid range around the picture: cells fold and stretch"""
    nx, ny = mesh_size(w, h)
    rng = np.random.default_rng(seed)
    m = identity(w, h).astype(np.int64) + rng.integers(-24 * 256, 24 * 256 + 1, (ny, nx, 2))
    return np.clip(m, NODE_MIN, NODE_MAX).astype(np.int32)


def points(mesh, x, y):
    """P (1/65536 sample) of both coordinates at the luma points (x, y) (int64 arrays of one shape) -> (PX, PY); below 2^31 by the node range"""
    m = mesh.astype(np.int64)
    i, j, xf, yf = x >> 4, y >> 4, x & 15, y & 15
    out = []
    for c in (0, 1):
        n = m[..., c]
        P = (16 - yf) * ((16 - xf) * n[j, i] + xf * n[j, i + 1]) + yf * ((16 - xf) * n[j + 1, i] + xf * n[j + 1, i + 1])
        assert int(np.abs(P).max()) < 1 << 31
        out.append(P)
    return out


def positions(mesh, w, h):
    """((px, py) of the luma samples, (px, py) of the chroma pairs), 1/32 sample of their plane"""
    x, y = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    PX, PY = points(mesh, x, y)
    cx, cy = np.meshgrid(np.arange(w // 2, dtype=np.int64), np.arange(h // 2, dtype=np.int64))
    QX, QY = points(mesh, 2 * cx, 2 * cy)
    return ((PX + 1024) >> 11, (PY + 1024) >> 11), ((QX + 2048) >> 12, (QY + 2048) >> 12)


def outside(px, py, pw, ph):
    ix, iy = px >> 5, py >> 5
    return (ix < -1) | (ix > pw - 1) | (iy < -1) | (iy > ph - 1)


def sample(plane, px, py, kind, fill):
    """plane (ph, pw) of one component at positions (px, py) -> uint8"""
    ph, pw = plane.shape
    s = plane.astype(np.int64)
    ix, iy, cx, cy = px >> 5, py >> 5, TABLE[kind][px & 31], TABLE[kind][py & 31]
    a = np.zeros(px.shape, np.int64)
    for r in range(4):
        yy = np.clip(iy - 1 + r, 0, ph - 1)
        t = np.zeros(px.shape, np.int64)
        for k in range(4):
            t += cx[..., k] * s[yy, np.clip(ix - 1 + k, 0, pw - 1)]
        a += cy[..., r] * t
    out = np.clip((a + 8192) >> 14, 0, 255)
    return np.where(outside(px, py, pw, ph), fill, out).astype(np.uint8)


def apply(kind, fill, mesh, y, uv):
    """NV12 planes of the visible size (h, w), (h / 2, w) -> the warped planes of the same size"""
    h, w = y.shape
    (lx, ly), (cx, cy) = positions(mesh, w, h)
    oy = sample(y, lx, ly, kind, fill[0])
    ouv = np.empty_like(uv)
    for c in (0, 1):
        ouv[:, c::2] = sample(uv[:, c::2], cx, cy, kind, fill[1 + c])
    return oy, ouv


def pad(y, uv):
    """up to whole macroblocks: the last visible column / row, chroma the last pair (pad_kernel's rule)"""
    h, w = y.shape
    W, H = (w + 15) & ~15, (h + 15) & ~15
    py = np.pad(y, ((0, H - h), (0, W - w)), mode="edge")
    pc = np.pad(uv.reshape(h // 2, w // 2, 2), ((0, (H - h) // 2), (0, (W - w) // 2), (0, 0)), mode="edge").reshape(H // 2, W)
    return py, pc


def plan(mesh, w, h, room_y=64, room_c=36):
    """(staged, direct): per 32 x 32 tile of the coded size, whether the source window -- floor(smallest node) - 1 .. floor(largest node) + 2 per axis over the
    nodes of the tile's visible cells, clamped to the plane -- fits room_y x room_y luma samples and room_c x room_c chroma pairs"""
    W, H = (w + 15) & ~15, (h + 15) & ~15
    m = mesh.astype(np.int64)
    staged = direct = 0
    for ty in range((H + 31) // 32):
        for tx in range((W + 31) // 32):
            xe, ye = min(32 * tx + 31, w - 1), min(32 * ty + 31, h - 1)
            n = m[2 * ty:(ye >> 4) + 2, 2 * tx:(xe >> 4) + 2]
            fits = True
            for c, size in ((0, w), (1, h)):
                lo, hi = int(n[..., c].min()), int(n[..., c].max())
                for shift, lim, room in ((8, size, room_y), (9, size // 2, room_c)):
                    a, b = min(max((lo >> shift) - 1, 0), lim - 1), min(max((hi >> shift) + 2, 0), lim - 1)
                    fits = fits and b - a + 1 <= room
            staged, direct = staged + fits, direct + (not fits)
    return staged, direct


def outside_fraction(mesh, w, h):
    """of the luma samples"""
    (lx, ly), _ = positions(mesh, w, h)
    return float(outside(lx, ly, w, h).mean())


def noise(w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)


def checkerboard(w, h, cell=3):
    """saturated: 0 / 255 in luma and in both chroma components"""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    yy = ((((x // cell) + (y // cell)) & 1) * 255).astype(np.uint8)
    cx, cy = np.meshgrid(np.arange(w // 2), np.arange(h // 2))
    c = ((((cx // cell) + (cy // cell)) & 1) * 255).astype(np.uint8)
    return yy, np.repeat(c, 2, axis=1)
