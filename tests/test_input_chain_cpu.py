"""The input chain without a device ("The chain"): what holds the steps' references together -- the margin convention of section 23 on each
reference alone at two sizes with margin columns and rows, the motion-compensated filter's stated exception (section 25), tests/chainref.py against the
library's host statements, and that in every case tests/test_input_chain_gpu.py runs every step does something on every picture."""
import numpy as np
import pytest

from tests import adjustref as A
from tests import autolevelref as AL
from tests import chainref as C
from tests import denoisemcref as M
from tests import denoiseref as D
from tests import dspatialref as DS
from tests import imageref as I
from tests import lut3dref as L
from tests import overlayref as O
from tests import rateref
from tests import warpref as W
from tests import yuvref as Y

SIZES = {"A": (70, 50), "B": (42, 26)}  # in 80 x 64 and in 48 x 32


def clip(w, h, n=2, seed=7):
    return AL.clip(w, h, n, seed=seed, still=True)


# name -> (the step on coded surfaces (y, uv, w, h) -> (y', uv'), the step on a visible picture (y, uv) -> (y', uv'))
def _warp(kind):
    def vis(y, uv):
        h, w = y.shape
        return W.apply(kind, (40, 90, 200), W.build(w, h, k1=-6000, cos=65502, sin=2100), y, uv)
    return (lambda y, uv, w, h: W.pad(*vis(*C.visible_part(y, uv, w, h)))), vis


def _yuv():
    coef = Y.coefficients(6, 1, 1, 0)
    return (lambda y, uv, w, h: Y.convert(y, uv, coef, Y.picture_mask(w, h))), (lambda y, uv: Y.convert(y, uv, coef))


def _dspatial():
    return (lambda y, uv, w, h: DS.apply(y, uv, 6, 4, None, (w, h))), (lambda y, uv: DS.apply(y, uv, 6, 4))


def _lut():
    nodes = C.cube9()
    return (lambda y, uv, w, h: L.apply(nodes, 9, 256, 6, 0, y, uv, None, visible=(w, h))), (lambda y, uv: L.apply(nodes, 9, 256, 6, 0, y, uv))


def _autolevel():
    a = dict(levels=900, balance=800, speed=64)
    return (lambda y, uv, w, h: AL.step(y, uv, a, 0, None, True, None, (w, h))[:2]), (lambda y, uv: AL.step(y, uv, a, 0, None, True)[:2])


def _adjust(**kw):
    a = A.params(**kw)
    luma, chroma = C.adjust_tables(a, 0)
    return (lambda y, uv, w, h: A.apply(y, uv, a, luma, chroma, None, (w, h))), (lambda y, uv: A.apply(y, uv, a, luma, chroma))


def _layer():
    img = I.random_image(np.random.default_rng(41), 24, 16)
    def vis(y, uv):
        h, w = y.shape
        return I.blend(y, uv, [I.layer(img, w - 20, h - 12, 200)], I.coefficients(2, 0, w, h))
    return (lambda y, uv, w, h: I.blend_coded(*C.visible_part(y, uv, w, h), [I.layer(img, w - 20, h - 12, 200)], I.coefficients(2, 0, w, h))), vis


def _text():
    style = dict(halign=O.RIGHT, valign=O.BOTTOM, xpad=0, ypad=0, scale=1, shaded_background=1)
    return (lambda y, uv, w, h: O.draw_coded(*C.visible_part(y, uv, w, h), "A7", **style)), (lambda y, uv: O.draw(y, uv, "A7", **style))


STEPS = {
    "warp-bilinear": _warp(0), "warp-bicubic": _warp(1), "colour-step": _yuv(), "spatial-filter": _dspatial(), "lut": _lut(), "autolevel": _autolevel(),
    "controls-table": _adjust(brightness=40, contrast=1200, saturation=1250), "controls-sharpen": _adjust(brightness=40, contrast=1200, saturation=1250, sharpen=16),
    "controls-blur": _adjust(sharpen=-16), "layer": _layer(), "text": _text(),
}


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("step", list(STEPS))
def test_each_reference_alone_keeps_the_margins_replicas(step, size):
    """on an input whose margins are replicas the output's are, and the step commutes with with_margins"""
    (w, h), (coded, vis) = SIZES[size], STEPS[step]
    Wc, Hc = C.coded(w, h)
    y, uv = clip(w, h)[1]
    sy, suv = C.with_margins(y, uv, Wc, Hc)
    assert C.margins_are_replicas(sy, suv, w, h) and (Wc - w, Hc - h) in ((10, 14), (6, 6))
    oy, ouv = coded(sy, suv, w, h)
    assert not np.array_equal(oy[:h, :w], y) or not np.array_equal(ouv[:h // 2, :w], uv)  # (it did something)
    assert C.margins_are_replicas(oy, ouv, w, h)
    vy, vuv = vis(y, uv)
    ry, ruv = C.with_margins(vy, vuv, Wc, Hc)
    assert np.array_equal(oy, ry) and np.array_equal(ouv, ruv)


@pytest.mark.parametrize("size", list(SIZES))
def test_the_temporal_filter_and_the_mix_keep_the_margins_replicas(size):
    """(their references have no visible-size form: the filter works on 8 x 8 blocks of the coded surface, the mix on two surfaces)"""
    w, h = SIZES[size]
    Wc, Hc = C.coded(w, h)
    pics = _moving(w, h, (0, 0))  # (a still scene with fresh noise on both planes per picture)
    out = D.chain(pics, [(8, 8)] * 3, visible=(w, h))
    assert all(C.margins_are_replicas(y, uv, w, h) for y, uv in out) and all(not np.array_equal(o[0], p[0]) and not np.array_equal(o[1], p[1]) for o, p in zip(out[1:], pics[1:]))
    for wt in (1, 77, 128, 255):
        my, muv = rateref.mix(pics[0][0], pics[1][0], wt), rateref.mix(pics[0][1], pics[1][1], wt)
        assert C.margins_are_replicas(my, muv, w, h)
        ry, ruv = C.with_margins(rateref.mix(pics[0][0][:h, :w], pics[1][0][:h, :w], wt), rateref.mix(pics[0][1][:h // 2, :w], pics[1][1][:h // 2, :w], wt), Wc, Hc)
        assert np.array_equal(my, ry) and np.array_equal(muv, ruv)


@pytest.mark.parametrize("size", list(SIZES))
def test_a_lut_that_grades_the_visible_rectangle_alone_or_the_whole_surface_breaks_the_convention(size):
    """why rule 6 of DESIGN.md section 29 is there: cut to the visible size the margin keeps the ungraded replica, and graded pointwise over the whole surface the
    chroma of a margin quad comes from four samples of the last column alone -- neither is the replica of the graded picture"""
    w, h = SIZES[size]
    Wc, Hc = C.coded(w, h)
    y, uv = AL.with_margins(*clip(w, h)[1], Wc, Hc)
    nodes = C.cube9()
    cy, cuv = L.apply(nodes, 9, 256, 6, 0, y, uv, (0, w, 0, h))
    ry, ruv = C.with_margins(cy[:h, :w], cuv[:h // 2, :w], Wc, Hc)
    assert np.array_equal(cy[:h, :w], ry[:h, :w]) and (cy != ry).sum() > (Wc * Hc - w * h) * 9 // 10 and (cuv != ruv).sum() > 0
    py, puv = L.apply(nodes, 9, 256, 6, 0, y, uv)
    assert np.array_equal(py, ry) and (puv != ruv).sum() > 0
    gy, guv = L.apply(nodes, 9, 256, 6, 0, y, uv, None, visible=(w, h))
    assert np.array_equal(gy, ry) and np.array_equal(guv, ruv)


def _moving(w, h, move, n=3, seed=2511):
    rng = np.random.default_rng(seed + w)
    big = rng.integers(60, 200, (h + 8, w + 8), dtype=np.uint8), rng.integers(60, 200, (h // 2 + 4, w + 8), dtype=np.uint8)
    pics = []
    for k in range(n):
        ox, oy = move[0] * k, move[1] * k
        y = np.clip(big[0][oy:oy + h, ox:ox + w].astype(np.int64) + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)
        uv = np.clip(big[1][oy // 2:oy // 2 + h // 2, ox:ox + w].astype(np.int64) + rng.integers(-6, 7, (h // 2, w)), 0, 255).astype(np.uint8)
        pics.append(C.with_margins(y, uv, *C.coded(w, h)))
    return pics


# (visible size, the scene's move per picture): still at both sizes; 70 x 48 has a partly visible block column only, and the scene moves down along it
@pytest.mark.parametrize("w,h,move", [(70, 50, (0, 0)), (42, 26, (0, 0)), (70, 48, (0, 2)), (64, 50, (2, 0))])
def test_the_motion_compensated_filter_keeps_them_where_section_25_says(w, h, move):
    """on a still scene, and on one that moves along the margin; a vector across a margin reads other history columns for the margin samples of a partly visible
    block than for the last visible one, so nothing is claimed elsewhere"""
    pics = _moving(w, h, move)
    hy = huv = None
    moved = False
    for y, uv in pics:
        oy, ouv, hy, huv, vec, _ = M.step(y, uv, hy, huv, 8, 8, 4, visible=(w, h), vectors=True)
        moved |= vec is not None and bool(vec.any())
        assert C.margins_are_replicas(oy, ouv, w, h)
    assert moved == (move != (0, 0)) and not np.array_equal(oy, pics[-1][0])


# ---- chainref against the C side
def test_one_picture_through_the_chain_with_the_librarys_host_statements_in_place_of_the_python_rules(E):
    """mi355enc_warp_build / _warp_apply_host, mi355enc_denoise_spatial_apply_host, mi355enc_lut3d_apply_host (which grades a rectangle and knows no margin: the
    rectangle cut to the visible size, then the convention), mi355enc_adjust_tables; and mi355enc_denoise_tables against the filter's"""
    def lut(nodes, N, strength, matrix, full, y, uv, rect, visible):
        (w, h), (H, Wc) = visible, y.shape
        gy, guv = E.lut3d_apply_host(nodes, strength, matrix, full, y, uv, (0, w, 0, h))
        return C.with_margins(gy[:h, :w], guv[:h // 2, :w], Wc, H)

    rules = dict(
        warp=lambda s, mesh, y, uv: E.warp_apply_host(dict(kind=s["kind"], fill=s["fill"]), mesh, y, uv),
        warp_mesh=lambda w, h, params: E.warp_build(w, h, **params),
        dspatial=lambda y, uv, sl, sc, rect, vis: E.denoise_spatial_apply_host(y, uv, -1 if sl is None else sl, -1 if sc is None else sc, rect, vis),
        lut=lut,
        adjust_tables=lambda a, full: E.adjust_tables(a, full),
    )
    for name in ("A", "B"):
        ins, _ = C.inputs(name, C.sources(name, 2))
        sets = [C.all_on(name)] * 2
        want = C.compose(C.handle(name), ins, sets)
        got = C.compose(C.handle(name, rules=rules), ins, sets)
        for a, b in zip(got, want):
            assert _same_records(a, b)
    for d in ((8, 8), (3, 0), (0, 5), (32, 32)):
        for got, want in zip(E.denoise_tables(luma=d[0], chroma=d[1]), D.tables(*d)):
            assert np.array_equal(got, want), d


def _same_records(a, b):
    (ra, ta), (rb, tb) = a["records"]["autolevel"], b["records"]["autolevel"]
    return np.array_equal(a["y"], b["y"]) and np.array_equal(a["uv"], b["uv"]) and ra == rb and np.array_equal(ta, tb) and a["records"]["dspatial"] == b["records"]["dspatial"]


# ---- every case of tests/test_input_chain_gpu.py does what it is there for
def _differs(a, b):
    return not np.array_equal(a["y"], b["y"]) or not np.array_equal(a["uv"], b["uv"])


# every clip and settings list tests/test_input_chain_gpu.py runs: (picture, pictures, colour step, settings)
CASES = {
    "A": ("A", 6, True, None), "B": ("B", 6, True, None), "C": ("C", 6, True, None), "D": ("D", 6, True, None),
    "D-auto": ("D", 6, True, lambda n: [C.all_on("D", auto=True)] * n),                       # the spatial filter measures under the transposed rectangle
    "settings-changed": ("A", 8, True, lambda n: C.changing("A", n)),                          # test 4
    "mix": ("A", 10, True, None), "hold": ("A", 4, True, None),                                # test 5: the inputs, which the once-per-input steps see
    "off-after-on": ("A", 7, False, lambda n: [C.all_on("A")] * 3 + [{}] * 2 + [C.all_on("A")] * 2),  # test 7
}


@pytest.mark.parametrize("case", list(CASES))
def test_in_every_case_every_step_changes_every_picture(case):
    """the composition with any one step left out differs from the full one on every picture that step is on for -- but for the temporal filter's priming
    pictures, the first after off, which the rule itself passes through (out = c, H' = 16 c: denoiseref.step); a step whose setting is the identity would test nothing"""
    name, n, yuv, make = CASES[case]
    hd = C.handle(name, yuv=yuv)
    ins, recs = C.inputs(name, C.sources(name, n))
    sets = make(n) if make else [C.all_on(name)] * n
    full = C.compose(hd, ins, sets)
    assert len(full) == n and all(C.margins_are_replicas(o["y"], o["uv"], hd.w, hd.h) for o in full)
    for k in C.ORDER:
        if k == "yuv" and not yuv:
            continue
        part = C.compose(hd, ins, sets, skip=k)
        for i, (a, b) in enumerate(zip(full, part)):
            on = k == "yuv" or bool(sets[i].get(k))
            priming = k == "denoise" and (i == 0 or not sets[i - 1].get("denoise"))  # (the first picture after off)
            if on and not priming:
                assert _differs(a, b), (k, i)
            if not on and k in ("layers", "text", "lut", "adjust", "warp"):  # (a stateless step that is off leaves the picture as it is)
                assert not _differs(a, b), (k, i)
    if case == "D-auto":  # the strength comes from the measurement, below the setting's bound, and moves with it
        s = [o["records"]["dspatial"] for o in full]
        assert all(r["valid"] and 0 < r["s_luma"] < 8 and r["candidates"] == 24 for r in s) and len({r["x"] for r in s}) > 1
    if name == "C":  # the stabiliser moves the crop, and not only once
        assert len({(r["ox"], r["oy"]) for r in recs}) >= 3
        still, _ = C.inputs(name, C.sources(name, n), stabilise=False)
        assert all(not np.array_equal(a[0], b[0]) for a, b in zip(ins[1:], still[1:]))
    # the rectangle, worked out by hand: C reaches the visible right and bottom edge and so the surfaces'; D, turned right, shows pre-orientation (y, 49 - x):
    # rows 6 .. 57 are its columns, columns 6 .. 45 its rows 4 .. 43 mirrored
    assert hd.rect == {"A": (0, 80, 0, 64), "B": (0, 48, 0, 32), "C": (12, 80, 8, 64), "D": (6, 46, 6, 58)}[name]


def test_the_mix_alone_shows_mixes_at_both_sizes():
    for name in ("A", "B"):
        src, pts = C.sources(name, 5), [i * 10 ** 9 // 50 for i in range(5)]
        want = C.compose(C.handle(name, yuv=False, rate=(rateref.BLEND, 10 ** 9, 30, 2)), src, [{}] * 5, pts=pts)
        assert len(want) == 3 and any(not any(np.array_equal(o["visible"][0], s[0]) for s in src) for o in want)


def test_the_motion_compensated_case_moves_and_differs_from_the_uncompensated_one():
    hd = C.handle("A")
    ins, _ = C.inputs("A", C.sources("A", 4, still=False))
    on = C.all_on("A")
    full = C.compose(hd, ins, [dict(on, denoise=(8, 8, 8))] * 4)
    plain = C.compose(hd, ins, [on] * 4)
    none = C.compose(hd, ins, [dict(on, denoise=(8, 8, 8))] * 4, skip="denoise")
    assert [_differs(a, b) for a, b in zip(full, plain)][1:] == [True] * 3 and [_differs(a, b) for a, b in zip(full, none)][1:] == [True] * 3
    assert all(C.margins_are_replicas(o["y"], o["uv"], hd.w, hd.h) for o in full)  # (the LUT behind the filter writes the margin afresh)
