"""The mesh warp's rule without a device: the C statement (ceracoder_amd/csrc/warp_host.c) against tests/warpref.py -- the coefficient
table, the builder node for node with its range edges and its three refusals, the whole picture on noise with both filters, the identity, the clip on saturated
checkerboards, the plan of the kernel's two forms -- and the entry points' argument checks."""
import ctypes as C

import numpy as np
import pytest

from tests import warpref as R

ALL_SIZES = R.SIZES + R.STRIPS
FILL = (40, 90, 200)


def test_exports_are_present(E):
    L = E.load()
    names = [n for n in E.EXPORTS if "warp" in n]
    assert len(names) == 14
    for n in names:
        getattr(L, n)
    assert L.mi355enc_abi_version() == 4 and E.STAGE_WARP == 31


def test_coefficient_table_entry_for_entry(E):
    for kind in (0, 1):
        for f in range(32):
            c = E.warp_coeff(kind, f)
            assert c == R.taps(kind, f) and sum(c) == 128, (kind, f)
    assert E.warp_coeff(1, 0) == [0, 128, 0, 0] and E.warp_coeff(1, 16) == [-8, 72, 72, -8] and E.warp_coeff(1, 1) == [-2, 128, 2, 0]
    assert E.warp_coeff(0, 0) == [0, 128, 0, 0] and E.warp_coeff(0, 31) == [0, 4, 124, 0]
    c = np.zeros(4, np.int16)
    for kind, f in ((2, 0), (-1, 0), (0, 32), (1, -1)):
        assert E.load().mi355enc_warp_coeff(kind, f, c.ctypes.data) == E.ERR_ARG
    assert E.load().mi355enc_warp_coeff(0, 0, None) == E.ERR_ARG


@pytest.mark.parametrize("size", ALL_SIZES + [(2, 2), (16, 16), (8192, 16)], ids=lambda s: "%dx%d" % s)
def test_mesh_size_and_the_neutral_mesh_is_the_identity(E, size):
    w, h = size
    assert E.warp_mesh_size(w, h) == R.mesh_size(w, h) == ((w + 15) // 16 + 1, (h + 15) // 16 + 1)
    d = E.WarpParams()
    E.load().mi355enc_warp_params_default(C.byref(d))
    assert d.as_dict() == R.NEUTRAL
    ref, why = R.build_why(w, h)
    if why:  # (2 x 2: the nodes at 16 lie 31 half samples from the centre, past the bound on q)
        assert (w, h) == (2, 2) and why == "q"
        with pytest.raises(E.EncoderError):
            E.warp_build(w, h)
    else:
        assert np.array_equal(ref, R.identity(w, h)) and np.array_equal(E.warp_build(w, h), ref)


@pytest.mark.parametrize("size", ALL_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(R.SETS))
def test_builder_node_for_node(E, name, size):
    w, h = size
    ref = R.build(w, h, **R.SETS[name])
    assert ref is not None and ref.dtype == np.int32 and ref.min() >= R.NODE_MIN and ref.max() <= R.NODE_MAX
    got = E.warp_build(w, h, **R.SETS[name])
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:4]
    assert E.load().mi355enc_warp_mesh_check(got.ctypes.data, got.shape[1], got.shape[0]) == 0


def _built(E, w, h, **p):
    try:
        return E.warp_build(w, h, **p)
    except E.EncoderError:
        return None


@pytest.mark.parametrize("field", list(R.RANGES))
def test_every_range_edge_of_every_parameter(E, field):
    lo, hi = R.RANGES[field]
    w, h = 64, 48
    for edge in (lo, hi):
        for v in range(edge - 2, edge + 3):
            ref, why = R.build_why(w, h, **{field: v})
            got = _built(E, w, h, **{field: v})
            assert (ref is None) == (got is None), (field, v, why)
            assert (why == "range") == (not lo <= v <= hi), (field, v, why)
            if ref is not None:
                assert np.array_equal(ref, got), (field, v)


REFUSALS = [
    ("d", (160, 96), dict(zoom=262144, kh=-32768)),      # 1 + kh U / (w - 1) falls to 1 - 2
    ("q", (160, 96), dict(zoom=262144, kh=-12000)),      # d stays above 1/4, the radius passes eight half diagonals
    ("node", (1936, 32), dict(zoom=262144)),             # 968 - 4 * 968 lies left of -2048
]


@pytest.mark.parametrize("why, size, p", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_three_refusals(E, why, size, p):
    assert R.build_why(*size, **p) == (None, why)
    assert _built(E, *size, **p) is None


def test_builder_argument_checks(E):
    L = E.load()
    p = E.warp_params()
    m = np.zeros(2 * 5 * 4, np.int32)
    assert L.mi355enc_warp_build(C.byref(p), 64, 48, m.ctypes.data, m.size) == 0
    assert L.mi355enc_warp_build(C.byref(p), 64, 48, m.ctypes.data, m.size - 1) == E.ERR_ARG  # no room
    assert L.mi355enc_warp_build(None, 64, 48, m.ctypes.data, m.size) == E.ERR_ARG and L.mi355enc_warp_build(C.byref(p), 64, 48, None, m.size) == E.ERR_ARG
    for w, h in ((1, 48), (64, 1), (8193, 16), (16, 8193)):
        assert L.mi355enc_warp_build(C.byref(p), w, h, m.ctypes.data, 1 << 30) == E.ERR_ARG
    bad = R.identity(64, 48)
    assert L.mi355enc_warp_mesh_check(bad.ctypes.data, 5, 4) == 0
    for v in (R.NODE_MIN - 1, R.NODE_MAX + 1):
        bad[2, 3, 1] = v
        assert L.mi355enc_warp_mesh_check(bad.ctypes.data, 5, 4) == E.ERR_ARG
    for v in (R.NODE_MIN, R.NODE_MAX):
        bad[2, 3, 1] = v
        assert L.mi355enc_warp_mesh_check(bad.ctypes.data, 5, 4) == 0


@pytest.mark.parametrize("kind", [0, 1], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_whole_picture_against_warpref(E, size, kind):
    w, h = size
    y, uv = R.noise(w, h, w + h + kind)
    iy, iuv = E.warp_apply_host(dict(kind=kind, fill=FILL), R.identity(w, h), y, uv)
    assert np.array_equal(iy, y) and np.array_equal(iuv, uv)  # the identity is a copy
    ry, ruv = R.apply(kind, FILL, R.identity(w, h), y, uv)
    assert np.array_equal(ry, y) and np.array_equal(ruv, uv)
    meshes = [R.build(w, h, **p) for p in R.SETS.values()] + [R.random_mesh(w, h, 7)]
    for n, m in enumerate(meshes):
        gy, guv = E.warp_apply_host(dict(kind=kind, fill=FILL), m, y, uv)
        ry, ruv = R.apply(kind, FILL, m, y, uv)
        assert np.array_equal(gy, ry), (n, np.argwhere(gy != ry)[:4])
        assert np.array_equal(guv, ruv), (n, np.argwhere(guv != ruv)[:4])


def test_the_sets_do_what_they_are_named_for():
    """on the reference, at 160 x 96: so that no comparison above passes vacuously"""
    w, h = 160, 96
    out = {n: R.outside_fraction(R.build(w, h, **p), w, h) for n, p in R.SETS.items()}
    assert out["barrel"] == 0 and out["all"] == 0 and 0.05 < out["keystone"] < 0.15 and 0.35 < out["quarter"] < 0.45 and 0.80 < out["shrink"] < 0.90
    y, uv = R.noise(w, h, 3)
    m = R.build(w, h, **R.SETS["barrel"])
    assert (R.apply(0, FILL, m, y, uv)[0] != R.apply(1, FILL, m, y, uv)[0]).mean() >= 0.8
    q = R.build(w, h, **R.SETS["quarter"])  # whole luma positions: f = 0, and the two filters agree there
    assert np.array_equal(R.apply(0, FILL, q, y, uv)[0], R.apply(1, FILL, q, y, uv)[0])


def test_the_clip_acts_on_saturated_checkerboards(E):
    w, h = 160, 96
    y, uv = R.checkerboard(w, h)
    m = R.build(w, h, **R.SETS["barrel"])
    by, buv = R.apply(1, FILL, m, y, uv)
    ly, luv = R.apply(0, FILL, m, y, uv)
    for b, l in ((by, ly), (buv, luv)):
        sat = ((b == 0) | (b == 255)) & ~((l == 0) | (l == 255))
        assert int(sat.sum()) > 0  # overshoot of the bicubic filter, clipped where the bilinear one stays inside
    gy, guv = E.warp_apply_host(dict(kind=1, fill=FILL), m, y, uv)
    assert np.array_equal(gy, by) and np.array_equal(guv, buv)


@pytest.mark.parametrize("size", ALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_plan_against_the_references_window_test(E, size):
    w, h = size
    tiles = ((w + 15) // 16 * 16 + 31) // 32 * (((h + 15) // 16 * 16 + 31) // 32)
    for m in [R.build(w, h, **p) for p in R.SETS.values()] + [R.identity(w, h), R.random_mesh(w, h, 7), R.random_mesh(w, h, 8)]:
        got = E.warp_plan(m, w, h)
        assert got == R.plan(m, w, h) and sum(got) == tiles
    assert E.warp_plan(R.identity(w, h), w, h) == (tiles, 0)


def test_plan_of_the_named_sets_and_its_argument_checks(E):
    w, h = 160, 96
    plans = {n: R.plan(R.build(w, h, **p), w, h) for n, p in R.SETS.items()}
    assert plans["barrel"] == plans["all"] == (15, 0) and plans["shrink"] == (8, 7)  # (a zoom of 2.5 reads 80 source samples per 32: only the tiles that clamp at an edge fit)
    L, m, a, b = E.load(), R.identity(w, h), C.c_int(0), C.c_int(0)
    assert L.mi355enc_warp_plan(m.ctypes.data, 11, 7, w, h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (15, 0)
    for nx, ny, ww, hh in ((10, 7, w, h), (11, 8, w, h), (11, 7, w - 1, h), (11, 7, 1, h)):
        assert L.mi355enc_warp_plan(m.ctypes.data, nx, ny, ww, hh, C.byref(a), C.byref(b)) == E.ERR_ARG
    assert L.mi355enc_warp_plan(None, 11, 7, w, h, C.byref(a), C.byref(b)) == L.mi355enc_warp_plan(m.ctypes.data, 11, 7, w, h, None, C.byref(b)) == E.ERR_ARG
    bad = m.copy()
    bad[3, 3, 0] = R.NODE_MIN - 1
    assert L.mi355enc_warp_plan(bad.ctypes.data, 11, 7, w, h, C.byref(a), C.byref(b)) == E.ERR_ARG


def test_apply_host_argument_checks(E):
    L = E.load()
    w, h = 64, 48
    y, uv = R.noise(w, h, 1)
    oy, ouv = np.empty_like(y), np.empty_like(uv)
    m = R.identity(w, h)
    s = E.warp(kind=1)

    def call(s=s, m=m, w=w, h=h, ys=w, os=w):
        return L.mi355enc_warp_apply_host(C.byref(s) if s else None, m.ctypes.data if m is not None else None, w, h, y.ctypes.data, ys, uv.ctypes.data, w, oy.ctypes.data, os, ouv.ctypes.data, w)

    assert call() == 0
    bad = m.copy()
    bad[0, 0, 0] = R.NODE_MAX + 1
    assert call(s=None) == call(m=None) == call(m=bad) == call(s=E.warp(kind=2)) == call(w=63) == call(ys=w - 1) == call(os=w - 1) == E.ERR_ARG


def test_every_handle_entry_point_refuses_a_null_handle(E, capfd):
    L = E.load()
    s, p, m, g, on = E.warp(), E.warp_params(), R.identity(64, 48), C.c_uint(0), C.c_int(0)
    y, uv = np.zeros((48, 64), np.uint8), np.zeros((24, 64), np.uint8)
    assert L.mi355enc_set_warp(None, C.byref(s), C.byref(p)) == E.ERR_ARG
    assert L.mi355enc_set_warp_mesh(None, C.byref(s), m.ctypes.data, 5, 4) == E.ERR_ARG
    assert L.mi355enc_get_warp(None, C.byref(on), C.byref(s)) == E.ERR_ARG
    assert L.mi355enc_last_warp(None, C.byref(g)) == E.ERR_ARG
    assert L.mi355enc_debug_warp_bytes(None) == 0 and L.mi355enc_debug_warp_staging(None, 0) == E.ERR_ARG
    assert L.mi355enc_warp_probe(None, C.byref(s), m.ctypes.data, y.ctypes.data, uv.ctypes.data) == E.ERR_ARG
    ms = C.c_double(0)
    assert L.mi355enc_time_stage(None, 31, 1, C.byref(ms)) == E.ERR_ARG
    assert "mi355enc:" not in capfd.readouterr().err
