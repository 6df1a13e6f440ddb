"""The electronic image stabiliser's rule without a device: the C statement (ceracoder_amd/csrc/stab_host.c) against tests/stabref.py --
projections, votes (ties, flat bands, minima on the window's edge, n = 4 range, the 33-bit cost), medians, the trajectory step -- the setting's ranges, the
table property that decides what "the offset" means, and the entry points' argument checks."""
import ctypes as C

import numpy as np
import pytest

from tests import geomref as G
from tests import stabref as S


def test_exports_are_present(E):
    L = E.load()
    names = [n for n in E.EXPORTS if "stabilize" in n]
    assert len(names) == 12
    for n in names:
        getattr(L, n)
    assert L.mi355enc_abi_version() == 4
    assert (E.STAGE_STABILIZE_PROJECT, E.STAGE_STABILIZE_MATCH) == (29, 30)


def test_default_is_off_and_check_at_every_edge(E):
    d = E.Stabilize()
    E.load().mi355enc_stabilize_default(C.byref(d))
    assert d.as_dict() == dict(range=0, leak=16, margin_x=0, margin_y=0) == E.stabilize().as_dict()
    assert E.stabilize(range=16, margin=32).as_dict() == dict(range=16, leak=16, margin_x=32, margin_y=32)
    assert E.stabilize_check() == 0
    for field, lo, hi, even in (("range", 0, 32, False), ("leak", 0, 255, False), ("margin_x", 0, 1024, True), ("margin_y", 0, 1024, True)):
        for edge in (lo, hi):
            for v in range(edge - 2, edge + 3):
                ok = lo <= v <= hi and not (even and v % 2)
                assert (E.stabilize_check(**{field: v}) == 0) == ok, (field, v)
    assert E.load().mi355enc_stabilize_check(None) == E.ERR_ARG


@pytest.mark.parametrize("shape", [(64, 48), (70, 50), (3, 5), (1, 1), (257, 33)])
def test_projection_against_stabref(E, shape):
    w, h = shape
    rng = np.random.default_rng(w * 100 + h)
    for step, first, pad, offset in ((1, 0, 0, 0), (1, 0, 3, 1), (2, 0, 1, 0), (2, 1, 2, 3)):
        row = first + (w - 1) * step + 1 + pad
        buf = rng.integers(0, 256, offset + row * h, dtype=np.uint8)
        luma = np.lib.stride_tricks.as_strided(buf[offset + first:], (h, w), (row, step))
        c, r = E.stabilize_project(luma)
        rc, rr = S.project(luma)
        assert np.array_equal(c, rc) and np.array_equal(r, rr), (step, first, pad)
    sat = np.full((h, w), 255, np.uint8)
    c, r = E.stabilize_project(sat)
    assert np.array_equal(c, S.project(sat)[0]) and int(c.sum()) == 255 * w * h == int(r.sum())


CASES = S.match_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_vote_motion_and_step_against_stabref(E, case):
    name, prev, cur, rng, leak, bnd, state = case
    rec = S.match(prev, cur, rng, leak, bnd, state)
    assert (rec["mx"], rec["my"], rec["votes_x"], rec["votes_y"]) == S.EXPECT[name]  # (the reference finds what the case was built to hold)
    got = []
    for axis in (0, 1):
        votes = []
        for k in range(4):
            ok, d = E.stabilize_vote(cur[axis][k], prev[axis][k], rng)
            assert (ok, d) == S.vote(cur[axis][k], prev[axis][k], rng), (axis, k)
            if ok:
                votes.append(d)
        m = E.stabilize_motion(votes)
        assert m == S.motion(votes)
        got += [m, len(votes)] + list(E.stabilize_step(state[axis], m, leak, bnd[2 * axis], bnd[2 * axis + 1]))
    assert got == [rec["mx"], rec["votes_x"], rec["sx"], rec["ox"], rec["my"], rec["votes_y"], rec["sy"], rec["oy"]]


def test_the_cost_at_the_ceiling_needs_33_bits(E):
    """(as a signed number: it passes 2^31, so an int accumulator would go negative)"""
    a = np.tile(np.array([0, S.CEIL], np.uint32), 4096)
    c = S.costs(a, S.CEIL - a, 32)
    assert max(c) == (8192 - 64) * S.CEIL > 1 << 31 and min(c) == 0 and c.count(0) == 32
    assert E.stabilize_vote(a, S.CEIL - a, 32) == (False, -31)  # a tie: no vote
    b = a.copy()
    b[4001] = 5  # one odd shift is now the only best one; every even one still costs more than a signed 32-bit word holds
    p = np.roll(b, 3)
    assert E.stabilize_vote(p, b, 32) == S.vote(p, b, 32) == (True, 3)


def test_vote_refuses_what_is_no_projection(E):
    L, d = E.load(), C.c_int(0)
    p = np.zeros(64, np.uint32)
    a = p.ctypes.data
    assert L.mi355enc_stabilize_vote(a, a, 64, 16, C.byref(d)) == 0  # n = 4 range: flat, no vote
    for n, rng in ((63, 16), (64, 0), (64, 33), (8193, 4)):
        assert L.mi355enc_stabilize_vote(a, a, n, rng, C.byref(d)) == E.ERR_ARG
    assert L.mi355enc_stabilize_vote(None, a, 64, 4, C.byref(d)) == E.ERR_ARG and L.mi355enc_stabilize_vote(a, a, 64, 4, None) == E.ERR_ARG


def test_motion_is_the_lower_median(E):
    for votes, want in (([], 0), ([5], 5), ([5, -3], -3), ([5, -3, 7], 5), ([5, -3, 7, 0], 0), ([2, 2, 2, -8], 2)):
        assert E.stabilize_motion(votes) == S.motion(votes) == want


@pytest.mark.parametrize("leak", [0, 1, 16, 128, 254, 255])
def test_trajectory_floors_negative_states(E, leak):
    rng = np.random.default_rng(leak)
    for lo, hi in ((0, 0), (-16, 0), (0, 16), (-1024, 1024), (-2, 6)):
        states = list(rng.integers(-262144, 262145, 300)) + [-262144, -257, -256, -255, -1, 0, 1, 255, 256, 262144]
        for s in states:
            m = int(rng.integers(-32, 33))
            assert E.stabilize_step(int(s), m, leak, lo, hi) == S.step(int(s), m, leak, lo, hi), (s, m, lo, hi)
    assert S.step(-1, 0, 1, -16, 16) == (-1, 0) and S.step(-300, 0, 128, -16, 16) == (-150, 0) and S.step(-255, 0, 255, -16, 16)[0] == -1  # floor, not truncation
    assert E.stabilize_step(100000, 32, leak, 0, 0) == (0, 0)  # no room: the crop does not move
    with pytest.raises(E.EncoderError):
        E.stabilize_step(0, 0, leak, 2, 4)  # lo above 0
    with pytest.raises(E.EncoderError):
        E.stabilize_step(0, 0, leak, -3, 4)  # odd


def test_bounds_follow_the_crop(E):
    assert S.bounds(16, 16, 128, 160) == (-16, 16)
    assert S.bounds(16, 6, 128, 160) == (-6, 16) and S.bounds(16, 7, 128, 160) == (-6, 16)  # even, towards zero
    assert S.bounds(16, 0, 160, 160) == (0, 0) and S.bounds(16, 32, 128, 160) == (-16, 0)


def _same_tables(off, o, crop, dst, kind, disp):
    moved, base = G.table(off + o, crop, dst, kind), G.table(off, crop, dst, kind)
    return [(f, list(q)) for f, q in moved] == [(f + disp, list(q)) for f, q in base]


def test_displaced_base_tables_are_not_the_moved_crops_tables():
    """why the offset displaces the base tables: at 1:1 and 2:1 the tables of the crop moved by o are the base tables with every index displaced, entry for
    entry; at other ratios a few weights differ in the last place, because off + x rounds differently in double"""
    for crop, dst in ((128, 128), (128, 64)):
        for o in range(-32, 33, 2):
            assert _same_tables(32, o, crop, dst, G.LUMA, o) and _same_tables(32, o, crop, dst, G.CHROMA_V422, o), (crop, dst, o)
            assert _same_tables(32, o, crop, dst, G.CHROMA_H, o // 2) and _same_tables(32, o, crop, dst, G.CHROMA_V, o // 2), (crop, dst, o)
    kinds = ((G.LUMA, 1), (G.CHROMA_H, 2), (G.CHROMA_V, 2), (G.CHROMA_V422, 1))
    for crop, dst, where in ((1600, 1920, {G.CHROMA_V422}), (3200, 1920, {G.LUMA, G.CHROMA_V})):  # (which of the tables it hits depends on the ratio)
        differ = [(kind, o) for kind, div in kinds for o in range(-32, 33, 8) if not _same_tables(32, o, crop, dst, kind, o // div)]
        assert differ and {k for k, _ in differ} == where and all(o for _, o in differ), (crop, dst)
        kind, o = differ[0]  # ... in a few entries only (a weight's last place, or a tap at the very edge of the support that comes or goes)
        moved, base = G.table(32 + o, crop, dst, kind), G.table(32, crop, dst, kind)
        assert 0 < sum((f, list(a)) != (g + o // dict(kinds)[kind], list(b)) for (f, a), (g, b) in zip(moved, base)) < len(base) // 8


def test_every_handle_entry_point_refuses_a_null_handle(E, capfd):
    L = E.load()
    st, info = E.stabilize(range=8, margin=16), E.StabilizeInfo()
    buf = np.zeros(4 * (64 + 48), np.uint32)
    luma = np.zeros((48, 64), np.uint8)
    assert L.mi355enc_set_stabilize(None, C.byref(st)) == E.ERR_ARG
    assert L.mi355enc_get_stabilize(None, C.byref(st)) == E.ERR_ARG
    assert L.mi355enc_last_stabilize(None, C.byref(st), C.byref(info)) == E.ERR_ARG
    assert L.mi355enc_debug_stabilize_bytes(None) == 0
    assert L.mi355enc_stabilize_probe_project(None, luma.ctypes.data, 64, 1, 64, 48, buf.ctypes.data) == E.ERR_ARG
    assert L.mi355enc_stabilize_probe_match(None, buf.ctypes.data, buf.ctypes.data, 64, 48, C.byref(st), C.byref((C.c_int * 4)(0, 0, 0, 0)), C.byref((C.c_int * 2)(0, 0)), 0,
                                            C.byref(info)) == E.ERR_ARG
    ms = C.c_double(0)
    for stage in (29, 30, 31):
        assert L.mi355enc_time_stage(None, stage, 1, C.byref(ms)) == E.ERR_ARG
    assert "mi355enc:" not in capfd.readouterr().err
