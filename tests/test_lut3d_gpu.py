"""GPU: the 3D colour LUT step (mi355enc_set_lut3d, k_lut3d.hip) -- the launch alone, in both of its forms, bit for bit against
tests/lut3dref.py, and streams: the access units of an encoder with the LUT on equal, byte for byte, those of a plain encoder fed lut3dref's pictures."""
import numpy as np
import pytest

from tests import adjustref as A
from tests import autolevelref as AL
from tests import denoiseref as D
from tests import lut3dref as R
from tests import rateref
from tests.inputref import device_free
from tests.test_geometry_gpu import geom_pictures, nv12_clip, plain_stream, run, same
from tests.test_yuv_convert_gpu import dev_get, dev_put

pytestmark = pytest.mark.gpu

GOP, QP, NPIC = 30, 28, 6
MATRIX = 6  # what an unspecified matrix resolves to at these sizes
# (visible size, geometry's input size and destination or None) -> coded surfaces 16 x 16, 80 x 80 (eight columns of padding), 208 x 128 (a letterbox inside), and
# 80 x 64 around 70 x 50 with a letterbox that reaches the bottom edge from a column that is no multiple of 8: to the right edge too (the corner), and to a
# column inside the visible width that is no multiple of 8 either (border columns in the margin rows on both sides)
SHAPES = {"16x16": ((16, 16), None), "72x80": ((72, 80), None), "208x128-letterbox": ((208, 128), ((176, 108), (16, 10, 176, 108))),
          "70x50-letterbox-to-the-corner": ((70, 50), ((96, 64), (12, 8, 58, 42))), "70x50-letterbox-to-the-bottom": ((70, 50), ((96, 64), (12, 8, 42, 42)))}
# the picture rectangle in the coded surfaces: it reaches their edge where it reaches the visible picture's (72 x 80: the eight margin columns belong to it)
RECTS = {"16x16": (0, 16, 0, 16), "72x80": (0, 80, 0, 80), "208x128-letterbox": (16, 192, 10, 118), "70x50-letterbox-to-the-corner": (12, 80, 8, 64),
         "70x50-letterbox-to-the-bottom": (12, 54, 8, 64)}
COLORIMETRY = [(0, 1), (1, 1), (0, 6), (1, 9)]  # (full range, matrix)
CUBES = {}


def cube(kind, N):
    """the test cubes, made once: seeded noise, and the log cube"""
    if (kind, N) not in CUBES:
        CUBES[kind, N] = R.quantise(R.cube_noise(N, 40 + N) if kind == "noise" else R.cube_log(N))
    return CUBES[kind, N]


def noise_surfaces(W, H, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)


def encoder(E, shape, full=0, matrix=2, **kw):
    (w, h), geom = SHAPES[shape]
    if geom:
        kw["geometry"] = E.geometry(geom[0], dst=geom[1], border=(235, 60, 200))
    return E.Encoder(w, h, fixed_qp=QP, colorimetry=(full, 2, 2, matrix), **kw)


@pytest.mark.parametrize("form", [0, 1], ids=["direct", "staged"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_probe_is_byte_equal_to_the_reference(E, shape, form):
    rect, (w, h) = RECTS[shape], SHAPES[shape][0]
    for k, (full, matrix) in enumerate(COLORIMETRY):
        e = encoder(E, shape, full, matrix)
        W, H = 16 * e.mbw, 16 * e.mbh
        y, uv = noise_surfaces(W, H, 10 * k + W)
        outside_y, outside_uv = np.ones((H, W), bool), np.ones((H // 2, W), bool)
        outside_y[rect[2]:rect[3], rect[0]:rect[1]] = False
        outside_uv[rect[2] // 2:rect[3] // 2, rect[0]:rect[1]] = False
        for N in (2, 3, 17, 33) + ((65,) if form == 0 else ()):
            for kind, strength in (("noise", 256), ("log", 256), ("noise", 128)):
                if k and (kind, strength) != ("noise", 256) and N not in (3, 33):
                    continue  # (every N, cube and strength with the first pair; the other pairs with two sizes of each)
                nodes = cube(kind, N)
                gy, guv = e.lut3d_probe(nodes, y, uv, strength, form)
                wy, wuv = R.apply(nodes, N, strength, matrix, full, y, uv, rect, visible=(w, h))
                assert np.array_equal(gy, wy) and np.array_equal(guv, wuv), (N, kind, strength, full, matrix)
                assert np.array_equal(gy[outside_y], y[outside_y]) and np.array_equal(guv[outside_uv], uv[outside_uv])  # the letterbox border keeps its bytes
                # the coded margin (noise on the way in) comes out as the replica of the graded visible picture, inside the rectangle's columns and rows
                ry, ruv = AL.with_margins(gy[:h, :w], guv[:h // 2, :w], W, H)
                inside_y, inside_uv = ~outside_y, ~outside_uv
                assert np.array_equal(gy[inside_y], ry[inside_y]) and np.array_equal(guv[inside_uv], ruv[inside_uv]), (N, kind, strength, full, matrix)
                assert not np.array_equal(gy, y) and not np.array_equal(guv, uv)
        assert e.debug_lut3d_bytes() == 0 and e.get_lut3d() is None  # (the probe is no part of the handle's own step)
        e.close()


def test_the_plan_names_the_form_the_probe_takes(E):
    e = encoder(E, "72x80")
    y, uv = noise_surfaces(80, 80, 3)
    for N in (2, 17, 33, 34, 35, 65):
        nodes = R.quantise(R.cube_noise(N, N))
        want = R.apply(nodes, N, 200, MATRIX, 0, y, uv, RECTS["72x80"], visible=(72, 80))
        got = e.lut3d_probe(nodes, y, uv, 200)
        assert E.lut3d_plan(N) in (E.LUT3D_DIRECT, E.LUT3D_STAGED) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    e.close()


def test_a_staged_form_asked_for_a_table_it_cannot_hold_is_refused(E, capfd):
    e = encoder(E, "16x16")
    y, uv = noise_surfaces(16, 16, 1)
    for N in (35, 65):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.lut3d_probe(E.lut3d_identity(N), y, uv, 256, E.LUT3D_STAGED)
    for bad in (dict(strength=0), dict(strength=257), dict(form=2), dict(form=-2)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.lut3d_probe(E.lut3d_identity(2), y, uv, **bad)
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        e.lut3d_probe(np.full(8, 1 << 31, np.uint32), y, uv)
    gy, guv = e.lut3d_probe(E.lut3d_identity(34), y, uv, 256, E.LUT3D_STAGED)  # the largest it can
    wy, wuv = R.apply(R.identity(34), 34, 256, MATRIX, 0, y, uv)
    assert np.array_equal(gy, wy) and np.array_equal(guv, wuv)
    e.close()
    assert "mi355enc:" not in capfd.readouterr().err  # (no HIP call failed on the way)


# ---- streams
def graded(pics, tables, strength=256, full=0, matrix=MATRIX, rect=None):
    """lut3dref's pictures: tables -- one (nodes, N) or None per picture"""
    return [p if t is None else R.apply(t[0], t[1], strength, matrix, full, p[0], p[1], rect) for p, t in zip(pics, tables)]


def stream(e, pics, depth=2, before=None):
    """-> ((access units, reconstruction), the pictures' (setting, generation))"""
    out, last = [], []

    def collect():
        out.append(e.collect())
        last.append(e.last_lut3d())

    for i in range(len(pics)):
        if before:
            before(i)  # (with the pipeline full: depth + 1 pictures in flight)
        if e.pending > depth:
            collect()
        e.submit(*pics[i], pts=i)
    while e.pending:
        collect()
    return (out, (e.fetch(0), e.fetch(1))), last


@pytest.mark.parametrize("w,h", [(64, 48), (208, 128), (72, 80), (70, 50)], ids=lambda v: str(v))
def test_stream_equals_the_plain_encoder_fed_the_references_pictures(E, w, h):
    pics = nv12_clip(w, h, NPIC, 500)
    t = (cube("noise", 17), 17)
    want = graded(pics, [t] * NPIC, 200)
    assert all(not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1]) for a, b in zip(want, pics))
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    assert e.get_lut3d() is None and e.debug_lut3d_bytes() == 0  # off by default
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.last_lut3d()
    e.set_lut3d(t[0], 200)
    assert e.get_lut3d() == dict(size=17, strength=200) and e.debug_lut3d_bytes() == 0  # nothing is allocated before the first graded picture
    got, last = stream(e, pics)
    assert e.debug_lut3d_bytes() >= 4 * 65 ** 3 and last == [(dict(size=17, strength=200), 1)] * NPIC
    same(got, ref)
    e.close()


@pytest.mark.parametrize("w,h", [(64, 48), (208, 128), (72, 80), (70, 50)], ids=lambda v: str(v))
def test_off_after_on_returns_to_plain_bytes(E, w, h):
    pics = nv12_clip(w, h, NPIC, 507)
    t = (cube("log", 33), 33)
    ref = plain_stream(E, w, h, graded(pics, [t] * 3 + [None] * 3))
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    e.set_lut3d(t[0])
    got, last = stream(e, pics, before=lambda i: e.set_lut3d(None) if i == 3 else None)
    assert e.get_lut3d() is None and last[:3] == [(dict(size=33, strength=256), 1)] * 3 and last[3:] == [(dict(size=0, strength=0), 0)] * 3
    py, puv = AL.with_margins(*pics[-1], 16 * e.mbw, 16 * e.mbh)  # (off, the coded surfaces are the input path's: the picture and its replicas)
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), py) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), puv)
    e.close()
    same(got, ref)
    # on and off again before the first picture: the plain stream, and nothing was allocated
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    e.set_lut3d(t[0])
    e.set_lut3d(None)
    got, last = stream(e, pics)
    assert e.debug_lut3d_bytes() == 0
    e.close()
    same(got, plain_stream(E, w, h, pics))


def test_strength_0_and_never_on_are_off(E):
    w, h = 64, 48
    pics = nv12_clip(w, h, NPIC, 501)
    ref = plain_stream(E, w, h, pics)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    e.set_lut3d(cube("noise", 17), 0)
    got, last = stream(e, pics)
    assert e.debug_lut3d_bytes() == 0 and all(g == 0 for _, g in last)
    same(got, ref)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.time_stage(E.STAGE_LUT3D, 2)
    for bad in (-1, 257):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.set_lut3d(cube("noise", 17), bad)
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        e.set_lut3d(np.full(8, 1 << 30, np.uint32))
    with pytest.raises(ValueError):
        e.set_lut3d(np.zeros(9, np.uint32))
    e.close()


def test_a_table_replaced_mid_stream_each_picture_carries_the_table_of_its_submit(E):
    """replaced after picture 2 with three pictures in flight, and the size changed 17 -> 33 on the way"""
    w, h = 64, 48
    pics = nv12_clip(w, h, NPIC, 502)
    a, b, c = (cube("noise", 17), 17), (cube("log", 17), 17), (cube("noise", 33), 33)
    tables = [a, a, a, b, c, c]
    ref = plain_stream(E, w, h, graded(pics, tables))
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    e.set_lut3d(a[0])

    def before(i):
        if i == 3:
            assert e.pending == 3  # pictures 0 .. 2 are in flight with the first table
            e.set_lut3d(b[0])
        if i == 4:
            e.set_lut3d(c[0])

    got, last = stream(e, pics, before=before)
    e.close()
    assert [g for _, g in last] == [1, 1, 1, 2, 3, 3] and [s["size"] for s, _ in last] == [17, 17, 17, 17, 33, 33]
    same(got, ref)


def test_a_cube_text_sets_the_table_under_a_letterbox_the_border_keeps_its_bytes(E):
    iw, ih, w, h, dst = 160, 96, 208, 128, (24, 16, 160, 96)
    rect = (dst[0], dst[0] + dst[2], dst[1], dst[1] + dst[3])
    pics = nv12_clip(iw, ih, NPIC, 503)
    boxed = geom_pictures(pics, (iw, ih), (0, 0, iw, ih), dst, w, h, border=(235, 60, 200))
    text = R.cube_text(R.cube_gamma_sat(5), 5)
    t = R.parse_cube(text)
    want = graded(boxed, [t] * NPIC, rect=rect)
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, geometry=E.geometry((iw, ih), dst=dst, border=(235, 60, 200)))
    e.set_lut3d(text)
    got, last = stream(e, pics)
    sy, suv = e.fetch(E.FETCH_SOURCE_Y), e.fetch(E.FETCH_SOURCE_UV)
    e.close()
    mask = np.zeros((h, w), bool)
    mask[rect[2]:rect[3], rect[0]:rect[1]] = True
    assert (sy[~mask] == 235).all() and (suv[~mask[0::2]].reshape(-1, 2) == (60, 200)).all() and not np.array_equal(sy[mask], boxed[-1][0][mask])
    assert last[-1] == (dict(size=5, strength=256), 1)
    same(got, ref)


@pytest.mark.parametrize("w,h", [(64, 48), (208, 128)], ids=lambda v: str(v))
def test_in_the_chain_the_stream_is_the_composition_of_the_references(E, w, h):
    """noise filter -> 3D LUT -> automatic levels -> picture controls: the filter's history stays ungraded, automatic levels measure the graded picture, and
    the controls (run by the plain encoder itself) trim on top"""
    pics = AL.clip(w, h, NPIC, still=True)
    t = (R.quantise(R.cube_gamma_sat(9)), 9)
    al, adj = dict(levels=900, balance=800, speed=64), dict(brightness=40, contrast=1200, saturation=1300)
    filtered = D.chain(pics, [(8, 8)] * NPIC)
    lut = graded(filtered, [t] * NPIC)
    res = AL.chain(lut, [al] * NPIC, 0, visible=(w, h))
    want = [(np.ascontiguousarray(r[0][:h, :w]), np.ascontiguousarray(r[1][:h // 2, :w])) for r in res]
    other = AL.chain(graded(pics, [t] * NPIC), [al] * NPIC, 0, visible=(w, h))  # (the filter behind the LUT, or no filter: other pictures)
    assert any(not np.array_equal(a[0], b[0][:h, :w]) for a, b in zip(want, other)) and any(r[2]["off_u"] or r[2]["off_v"] for r in res)
    ref = plain_stream(E, w, h, want, adjust=adj)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, denoise=dict(luma=8, chroma=8), autolevel=al, adjust=adj)
    e.set_lut3d(t[0])
    got, last = stream(e, pics)
    assert e.last_autolevel()[1] == res[-1][2]
    e.close()
    same(got, ref)


def test_a_repeated_picture_is_graded_once(E):
    w, h, ns = 64, 48, 10 ** 9
    pics = nv12_clip(w, h, 2, 504)
    t = (cube("noise", 17), 17)
    want = graded(pics, [t] * 2)
    e = E.Encoder(w, h, fps=60, gop=GOP, fixed_qp=QP, pipeline_depth=2, rate=(rateref.HOLD, ns, 2))
    e.set_lut3d(t[0])
    assert e.submit(*pics[0], pts=0) == 1
    e.collect()
    first = (e.fetch(E.FETCH_SOURCE_Y), e.fetch(E.FETCH_SOURCE_UV))
    assert np.array_equal(first[0], want[0][0]) and np.array_equal(first[1], want[0][1])
    assert e.submit(*pics[1], pts=ns // 30) == 2  # the tick in between repeats the first picture: graded once, not twice
    e.collect()
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), first[0]) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), first[1])
    e.collect()
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), want[1][0]) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), want[1][1])
    e.close()


def test_submit_device_never_grades_the_callers_planes(E):
    """64 x 48 on aligned planes would take the in-place exit: with the step on it must not, and the planes stay what they were"""
    w, h = 64, 48
    pics = nv12_clip(w, h, 3, 505)
    t = (cube("noise", 17), 17)
    ref = plain_stream(E, w, h, graded(pics, [t] * 3))
    dev = [(dev_put(y), dev_put(uv)) for y, uv in pics]
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    e.set_lut3d(t[0])
    got = run(e, lambda i: e.submit_device(dev[i][0], w, dev[i][1], w, pts=i), 3)
    e.close()
    for (dy, duv), (y, uv) in zip(dev, pics):
        assert np.array_equal(dev_get(dy, y.shape), y) and np.array_equal(dev_get(duv, uv.shape), uv)
        device_free(dy); device_free(duv)
    same(got, ref)


def test_the_timed_stage_is_refused_when_off_and_the_handle_encodes_correctly_after_it(E):
    w, h = 64, 48
    pics = nv12_clip(w, h, NPIC, 506)
    t = (cube("noise", 33), 33)
    ref = plain_stream(E, w, h, graded(pics, [t] * NPIC))
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.time_stage(E.STAGE_LUT3D, 2)
    assert e.debug_lut3d_bytes() == 0
    e.set_lut3d(t[0])
    assert e.time_stage(E.STAGE_LUT3D, 3) > 0 and e.debug_lut3d_bytes() >= 4 * 65 ** 3
    got, last = stream(e, pics)
    same(got, ref)
    assert e.time_stage(E.STAGE_LUT3D, 3) > 0
    e.submit(*pics[0], pts=NPIC)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):  # the probe refuses pictures in flight
        e.lut3d_probe(t[0], *noise_surfaces(64, 48, 1))
    e.collect()
    e.close()
