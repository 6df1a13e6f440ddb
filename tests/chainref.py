"""The input chain as one composition of the steps' own references ("The chain"; ingest_end in ceracoder_amd/csrc/enc_input.cpp):

    fill -> orientation -> warp -> colour step -> spatial noise filter -> temporal noise filter -> 3D LUT -> automatic levels -> picture controls
         -> [frame-rate mix] -> image layers -> text

New here is only the order, the picture rectangle (yuvref.picture_mask, handed to each step in the form its reference takes) and the margin predicate; every
rule is the step's own reference.  A step's state depends on its own inputs alone, so the composition runs step by step over the whole clip with each step's
own chain function, which is how a handle's state behaves.  Nothing here calls the library unless a test swaps a rule for the library's host statement (RULES)."""
import numpy as np

from tests import adjustref, autolevelref, denoisemcref, denoiseref, dspatialref, geomref, imageref, lut3dref, orientref, overlayref, rateref, stabref, warpref, yuvref

ORDER = ("warp", "yuv", "dspatial", "denoise", "lut", "autolevel", "adjust", "layers", "text")  # ingest_end's; the mix sits between adjust and layers


def coded(w, h):
    return (w + 15) // 16 * 16, (h + 15) // 16 * 16


def with_margins(y, uv, W, H):
    return autolevelref.with_margins(np.asarray(y), np.asarray(uv), W, H)


def visible_part(y, uv, w, h):
    return np.ascontiguousarray(y[:h, :w]), np.ascontiguousarray(uv[:h // 2, :w])


def margins_are_replicas(y, uv, w, h):
    """the margin convention: a sample of the coded margin is its clamped visible position's -- luma the last visible column / row, chroma
    the last visible pair / row, the corner both"""
    H, W = y.shape
    ry, ruv = with_margins(*visible_part(y, uv, w, h), W, H)
    return np.array_equal(y, ry) and np.array_equal(uv, ruv)


def picture_rect(w, h, dst=None, method=0):
    """(mask (H, W), rect (x0, x1, y0, y1)) of the picture part of the coded surfaces: dst the geometry's destination in the pre-orientation target, method the
    orientation.  The rectangle reaches the surfaces' edge where it reaches the visible picture's: a margin sample is what its clamped visible position is."""
    mask = yuvref.picture_mask(w, h, dst, method)
    ys, xs = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
    rect = (int(xs[0]), int(xs[-1]) + 1, int(ys[0]), int(ys[-1]) + 1)
    assert mask[rect[2]:rect[3], rect[0]:rect[1]].all() and mask.sum() == (rect[1] - rect[0]) * (rect[3] - rect[2]) and not any(v & 1 for v in rect)
    return mask, rect


# ---- the fill: what a submit makes of its input, visible pictures of the coded visible size
def fill_geometry(fmt, planes, in_size, crop, dst, target, border=geomref.BLACK, offset=None, method=0):
    """crop -> dst of the pre-orientation `target`, the border around it, then the orientation; offset (ox, oy): the stabiliser's -> the visible (y, uv)"""
    (iw, ih), (tw, th) = in_size, target
    crop = crop if crop is not None else (0, 0, iw, ih)
    if offset is None:
        y, uv = geomref.to_nv12(fmt, planes, iw, ih, crop, dst, tw, th, border)
    else:
        y, uv = stabref.to_nv12(fmt, planes, iw, ih, crop, dst, tw, th, offset[0], offset[1], border)
    return orientref.orient(*visible_part(y, uv, tw, th), method)


def stabiliser(lumas, setting, crop, in_size):
    """the records (ox, oy among them) of a clip's lumas under setting (range, leak, margin x, margin y)"""
    return stabref.run(lumas, setting, crop, in_size[0], in_size[1])


# ---- the rules a test may swap for the library's host statements
def adjust_tables(a, full):
    """(luma table, (cu, su)) in integers: gamma 1000 only, and a rotation whose products are whole numbers or far from a half"""
    a = adjustref.params(**a)
    cu, su = adjustref.chroma_model(a)
    assert min(abs(cu - np.floor(cu) - 0.5), abs(su - np.floor(su) - 0.5)) > 1e-6
    return adjustref.luma_table_int(a, full), (int(np.floor(cu + 0.5)), int(np.floor(su + 0.5)))


RULES = dict(
    warp=lambda s, mesh, y, uv: warpref.apply(s.get("kind", 1), s.get("fill", (16, 128, 128)), mesh, y, uv),
    warp_mesh=lambda w, h, params: warpref.build(w, h, **params),
    dspatial=dspatialref.apply,
    lut=lut3dref.apply,
    adjust_tables=adjust_tables,
)


class Handle:
    """What is fixed for a handle: the visible size, the geometry's destination and the orientation (for the rectangle), the output range and matrix, the
    colour step's coefficients (None: no colour step), the rate conversion (mode, pts per second, fps, max_fill) or None"""

    def __init__(self, w, h, dst=None, method=0, full=0, matrix=6, yuv=None, rate=None, rules=None):
        self.w, self.h, self.full, self.matrix, self.yuv, self.rate = w, h, full, matrix, yuv, rate
        self.W, self.H = coded(w, h)
        self.mask, self.rect = picture_rect(w, h, dst, method)
        self.rules = dict(RULES, **(rules or {}))


def _per_input(hd, pics, sets, skip):
    """the steps that run once per input, each over the whole clip: pics coded surfaces, sets one dict per picture -> (surfaces, records per picture)"""
    w, h, rect, vis = hd.w, hd.h, hd.rect, (hd.w, hd.h)
    get = lambda s, k: None if k == skip else s.get(k)
    recs = [dict() for _ in pics]
    # warp: the whole visible picture through the mesh, the margin by pad_kernel's rule
    out = []
    for (y, uv), s in zip(pics, sets):
        ws = get(s, "warp")
        if ws is not None:
            mesh = hd.rules["warp_mesh"](w, h, ws["params"])
            y, uv = warpref.pad(*hd.rules["warp"](ws, mesh, *visible_part(y, uv, w, h)))
        out.append((y, uv))
    pics = out
    # the colour step: the handle's, on every picture, inside the mask
    if hd.yuv is not None and skip != "yuv":
        pics = [yuvref.convert(y, uv, hd.yuv, hd.mask) for y, uv in pics]
    # the spatial noise filter: its own chain (the state X, priming after off), the filter itself swappable
    res, x, primed = [], 0, False
    for i, ((y, uv), s) in enumerate(zip(pics, sets)):
        a = dspatialref.params(get(s, "dspatial"))
        rec = dict(dspatialref.ZERO)
        if not dspatialref.active(a):
            primed = False
        elif a["auto_gain"] == 0:
            primed = False
            rec = dict(rec, s_luma=a["luma"], s_chroma=a["chroma"])
            y, uv = hd.rules["dspatial"](y, uv, a["luma"] or None, a["chroma"] or None, rect, vis)
        else:
            rec, x = dspatialref.decide(dspatialref.measure(y, rect, vis, hd.full), a, x, not primed)
            primed = True
            y, uv = hd.rules["dspatial"](y, uv, rec["s_luma"] if a["luma"] else None, rec["s_chroma"] if a["chroma"] else None, rect, vis)
        recs[i]["dspatial"] = rec
        res.append((y, uv))
    pics = res
    # the temporal noise filter: (luma, chroma, motion) per picture
    dn = [get(s, "denoise") or (0, 0, 0) for s in sets]
    if any(d[0] or d[1] for d in dn):
        pics = denoisemcref.chain(pics, [d[:2] for d in dn], [d[2] for d in dn], visible=vis) if any(d[2] for d in dn) else denoiseref.chain(pics, [d[:2] for d in dn], visible=vis)
    # the 3D LUT: (nodes, N, strength) per picture, the margin by rule 6
    res = []
    for (y, uv), s in zip(pics, sets):
        t = get(s, "lut")
        if t is not None and t[2] > 0:
            y, uv = hd.rules["lut"](t[0], t[1], t[2], hd.matrix, hd.full, y, uv, rect, visible=vis)
        res.append((y, uv))
    pics = res
    # automatic levels: its own chain
    al = autolevelref.chain(pics, [get(s, "autolevel") for s in sets], hd.full, rect=rect, visible=vis)
    pics = [(r[0], r[1]) for r in al]
    for i, r in enumerate(al):
        recs[i]["autolevel"] = (r[2], r[3])
    # the picture controls
    res = []
    for (y, uv), s in zip(pics, sets):
        a = get(s, "adjust")
        if a is not None and adjustref.params(**a) != adjustref.NEUTRAL:
            a = adjustref.params(**a)
            luma, chroma = hd.rules["adjust_tables"](a, hd.full)
            y, uv = adjustref.apply(y, uv, a, luma, chroma, rect, vis)
        res.append((y, uv))
    return res, recs


def _drawn(hd, y, uv, s, skip):
    """layers, then text: drawn into the visible picture, the margin following as if they had been in the picture before padding"""
    vy, vuv = visible_part(y, uv, hd.w, hd.h)
    layers = None if skip == "layers" else s.get("layers")
    text = None if skip == "text" else s.get("text")
    if not layers and not text:
        return y, uv
    if layers:
        vy, vuv = imageref.blend(vy, vuv, layers, imageref.coefficients(hd.matrix, hd.full, hd.W, hd.H))
    if text:
        vy, vuv = overlayref.draw(vy, vuv, text[0], **text[1])
    if not margins_are_replicas(y, uv, hd.w, hd.h):
        raise ValueError("layers and text on a picture whose margin is no replica: the composition has no rule for it")
    return with_margins(vy, vuv, hd.W, hd.H)


def compose(hd, inputs, sets, pts=None, skip=None):
    """inputs: the visible pictures (y, uv) the fill made, one per submit; sets: the settings latched at each submit, a dict with any of ORDER's names --
    warp dict(kind=, fill=, params=dict), dspatial dict, denoise (luma, chroma, motion), lut (nodes, N, strength), autolevel dict, adjust dict, layers [imageref
    layers], text (text, style dict); pts: the inputs' time stamps under a rate conversion; skip: one of ORDER's names left out.
    -> a list with one dict per output picture: y, uv (the coded surfaces), visible (what a plain encoder is fed), records (autolevel (record, table), dspatial),
    input (the index of the submit that yielded it), pts"""
    coded_in = [with_margins(y, uv, hd.W, hd.H) for y, uv in inputs]
    if hd.rate is None:
        done, recs = _per_input(hd, coded_in, sets, skip)
        outs = [(i, i, i, 256, i) for i in range(len(inputs))]
    else:
        mode, pps, fps, max_fill = hd.rate
        steps = rateref.run(mode, pps, fps, 1, max_fill, pts)
        # hold: an input that yields nothing is dropped in front of every latch and every step; blend: it is the next pair's first picture and goes through them
        live = [i for i in range(len(inputs)) if mode == rateref.BLEND or steps[i][0]]
        d, r = _per_input(hd, [coded_in[i] for i in live], [sets[i] for i in live], skip)
        done, recs = dict(zip(live, d)), dict(zip(live, r))
        owner = [i for i, st in enumerate(steps) for _ in st[0]]  # the submit that yields each output picture: its latches hold for layers and text
        outs = [(t, a, b, wt, o) for (t, a, b, wt), o in zip(rateref.shown(mode, steps), owner)]
    result = []
    for t, a, b, wt, o in outs:
        y, uv = done[b] if wt == 256 else (rateref.mix(done[a][0], done[b][0], wt), rateref.mix(done[a][1], done[b][1], wt))
        y, uv = _drawn(hd, y, uv, sets[o], skip)
        result.append(dict(y=y, uv=uv, visible=visible_part(y, uv, hd.w, hd.h), records=recs[b], input=o, pts=t))
    return result


# ---- the cases tests/test_input_chain_cpu.py and tests/test_input_chain_gpu.py share (the smallest pictures at which the named thing can go wrong)
COLORIMETRY = (0, 2, 2, 1)     # the output: limited-range BT.709 ...
INPUT_COLORIMETRY = (1, 6)     # ... from full-range BT.601 input: the colour step is on
FULL, MATRIX = 0, 1
BORDER = (235, 60, 200)
IN = (96, 64)                  # the input size of the pictures that are scaled
STAB = (8, 16, 8, 8)           # range, leak, margins
PICTURES = {
    # name: visible size, the geometry (crop, dst of the pre-orientation target, that target) or None, the orientation
    "A": dict(size=(70, 50), geom=None, method=0),  # ten margin columns, fourteen margin rows; 70 is no multiple of 8: the 8-wide patches straddle the visible edge
    "B": dict(size=(42, 26), geom=None, method=0),  # a partly visible 8 x 8 block row (26 & 7 = 2); the padding pass behind the plain NV12 copies
    "C": dict(size=(70, 50), geom=((8, 8, 80, 48), (12, 8, 58, 42), (70, 50)), method=0),  # a letterbox that reaches the visible right and bottom edge, border on the other two sides
    "D": dict(size=(50, 70), geom=(None, (6, 4, 52, 40), (70, 50)), method=1),  # 90r: the rectangle transposed and flipped, border on all four sides
    "E": dict(size=(64, 48), geom=None, method=0),  # no margin at all: the smallest picture whose device planes can be coded where they lie (tests/test_input_steps_gpu.py)
}
_CACHE = {}


def cube9():
    if "cube" not in _CACHE:
        _CACHE["cube"] = lut3dref.quantise(lut3dref.cube_gamma_sat(9))
    return _CACHE["cube"]


def handle(name, yuv=True, rate=None, rules=None):
    p = PICTURES[name]
    coef = yuvref.coefficients(INPUT_COLORIMETRY[1], INPUT_COLORIMETRY[0], COLORIMETRY[3], COLORIMETRY[0]) if yuv else None
    return Handle(p["size"][0], p["size"][1], p["geom"][1] if p["geom"] else None, p["method"], FULL, MATRIX, coef, rate, rules)


def sources(name, n, still=True, seed=7):
    """the n pictures a test submits for picture `name` (NV12 planes of the submitted size: the visible size, or IN where a geometry scales)"""
    p = PICTURES[name]
    w, h = IN if p["geom"] else p["size"]
    if p["geom"] and p["geom"][0]:  # stabilised: a clip that shakes
        return [tuple(pic) for pic in stabref.clip(w, h, seed=2600 + seed)][:n]
    return autolevelref.clip(w, h, n, seed=seed, still=True) if still else moving_clip(w, h, n, seed)


def moving_clip(w, h, n, seed, sigma=3.0, step=(2, -2)):
    """a texture of 4 x 4 cells that moves by `step` a picture plus seeded Gaussian noise, visible NV12 pictures: what a motion search has something to find in"""
    rng = np.random.default_rng(seed)
    big = np.kron(rng.integers(40, 216, ((h + 96) // 4, (w + 96) // 4)), np.ones((4, 4), np.int64))
    bigc = np.kron(rng.integers(90, 166, ((h + 96) // 4, (w + 96) // 4, 2)), np.ones((2, 2, 1), np.int64))
    noisy = lambda p: np.clip(np.rint(p + sigma * rng.standard_normal(p.shape)), 0, 255).astype(np.uint8)
    out = []
    for i in range(n):
        ox, oy = 48 - step[0] * i, 48 - step[1] * i
        out.append((noisy(big[oy:oy + h, ox:ox + w]), noisy(bigc[oy // 2:oy // 2 + h // 2, ox // 2:ox // 2 + w // 2].reshape(h // 2, w))))
    return out


def inputs(name, src, stabilise=True):
    """-> (the visible pictures the fill makes of the sources, the stabiliser's records or None)"""
    p = PICTURES[name]
    if not p["geom"]:
        return [tuple(s) for s in src], None
    crop, dst, target = p["geom"]
    recs = stabiliser([s[0] for s in src], STAB, crop, IN) if crop and stabilise else None
    off = [(r["ox"], r["oy"]) for r in recs] if recs else [None] * len(src)
    return [fill_geometry(geomref.FMT_NV12, list(s), IN, crop, dst, target, BORDER, o, p["method"]) for s, o in zip(src, off)], recs


def all_on(name, seed=1, auto=False):
    """every step's setting at once, each one doing something on every picture (tests/test_input_chain_cpu.py checks that); auto: the spatial filter measures
    the picture and sets its own strength"""
    w, h = PICTURES[name]["size"]
    img = imageref.random_image(np.random.default_rng(40 + seed), 24, 16)
    return dict(
        warp=dict(kind=1, fill=(40, 90, 200), params=dict(k1=-6000, cos=65502, sin=2100)),
        dspatial=dict(luma=8, chroma=8, auto_gain=1000, percentile=50, speed=64) if auto else dict(luma=6, chroma=4),
        denoise=(8, 8, 0),
        lut=(cube9(), 9, 256),
        autolevel=dict(levels=900, balance=800, speed=64),
        adjust=dict(brightness=40, contrast=1200, saturation=1250, sharpen=16),
        layers=[imageref.layer(img, w - 20, h - 12, 200)],  # across the visible right and bottom edge: the margin follows the blended picture
        text=("A%d" % seed, dict(halign=overlayref.LEFT, valign=overlayref.BOTTOM, xpad=2, ypad=0, scale=1, shaded_background=1)),
    )


def changing(name="A", n=8):
    """settings that change while three pictures are in flight: every step's at another picture as far as eight steps, one of which also comes back, fit seven
    pictures -- the temporal filter goes off at picture 3 and is on again, with other strengths, at picture 6, where it primes again.  One object per setting as
    long as it lasts, so that a test sets what changed and no more (a set counts a generation)."""
    on, other = all_on(name), all_on(name, seed=2)
    warp2, ds2, dn2, lut2 = dict(on["warp"], params=dict(k1=4000, cos=65502, sin=-2100)), dict(luma=3, chroma=8), (4, 12, 0), (on["lut"][0], 9, 128)
    al2, adj2 = dict(levels=600, balance=1000, speed=128), dict(brightness=-30, contrast=900, saturation=1250, sharpen=-8)
    sets = []
    for i in range(n):
        sets.append(dict(
            warp=warp2 if i >= 1 else on["warp"], dspatial=ds2 if i >= 2 else on["dspatial"], denoise=None if i in (3, 4, 5) else dn2 if i >= 6 else on["denoise"],
            lut=lut2 if i >= 4 else on["lut"], autolevel=al2 if i >= 5 else on["autolevel"], adjust=adj2 if i >= 7 else on["adjust"],
            layers=other["layers"] if i >= 6 else on["layers"], text=other["text"] if i >= 7 else on["text"]))
    return sets
