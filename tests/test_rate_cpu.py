"""The rule of the frame-rate conversion on the host: the C plan (rate_host.c through mi355enc_rate_plan_init / _step) against
tests/rateref.py step for step, on the cases the design states with their expected sequences written out, on seeded random sequences, and at large values.
No GPU."""
import ctypes as C
import random

import pytest

from tests import rateref as R
from ceracoder_amd import enc as E

NS = 10 ** 9


def inputs(num, den=1, n=13, pps=NS):
    return [i * pps * den // num for i in range(n)]


def both(mode, pps, fps_num, fps_den, max_fill, pts_list, t0=None, k_next=-1):
    """the sequence through the C plan and through rateref; asserts they agree step for step and returns the steps"""
    c = E.RatePlan(mode, pps, fps_num, fps_den, max_fill, t0=t0 or 0, k_next=k_next)
    r = R.Plan(mode, pps, fps_num, fps_den, max_fill, t0=t0 if k_next >= 0 else None, k_next=max(k_next, 0))
    steps = []
    for i, p in enumerate(pts_list):
        got, want = c.step(p), r.step(p)
        assert got == (want[0], want[1], want[2]), (i, p, got, want)
        steps.append(want)
    return steps


def kept(steps):
    return [i for i, (pts, _, _) in enumerate(steps) if pts]


def test_hold_60_to_30():
    st = both(R.HOLD, NS, 30, 1, 2, inputs(60))
    assert kept(st) == [0, 2, 3, 6, 8, 9, 12]
    assert sum(1 for s in st if not s[0]) == 6 and all(len(s[0]) <= 1 for s in st) and not any(s[2] for s in st)
    assert [s[0][0] for s in st if s[0]] == [k * NS // 30 for k in range(7)]


def test_blend_60_to_30_and_same_rate():
    st = both(R.BLEND, NS, 30, 1, 2, inputs(60))
    assert all(w == 256 for s in st for w in s[1]) and sum(len(s[0]) for s in st) == 7
    for mode in (R.HOLD, R.BLEND):
        st = both(mode, NS, 30, 1, 2, inputs(30))
        assert [(len(s[0]), s[1], s[2]) for s in st] == [(1, [256], False)] * 13
        assert [s[0][0] for s in st] == [k * NS // 30 for k in range(13)]


def test_hold_30_to_ntsc():
    st = both(R.HOLD, NS, 30000, 1001, 2, inputs(30))
    assert [len(s[0]) for s in st] == [1] * 13 and not any(s[2] for s in st)
    assert [s[0][0] for s in st] == [k * NS * 1001 // 30000 for k in range(13)]
    both(R.HOLD, NS, 7013, 234, 2, inputs(30))


def test_hold_25_to_30_repeats():
    st = both(R.HOLD, NS, 30, 1, 2, inputs(25))
    sh = R.shown(R.HOLD, st)
    srcs = [a for _, a, _, _ in sh]
    assert srcs == [0, 1, 2, 2, 3, 4, 5, 6, 7, 7, 8, 9, 10, 11, 12, 12][: len(srcs)] and len(srcs) >= 15
    assert [i for i, s in enumerate(st) if len(s[0]) == 2] == [3, 8]  # the inputs AFTER 2 and 7 make two ticks due: the first repeats 2 / 7
    assert [t for t, _, _, _ in sh] == [k * NS // 30 for k in range(len(sh))]


def test_blend_25_to_30():
    st = both(R.BLEND, NS, 30, 1, 2, inputs(25))
    sh = R.shown(R.BLEND, st)
    assert [w for _, _, _, w in sh][:8] == [256, 213, 171, 128, 85, 43, 256, 213]
    assert [(a, b) for _, a, b, _ in sh][:8] == [(0, 0), (0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (4, 5), (5, 6)]


@pytest.mark.parametrize("pps", [NS, 90000])
def test_blend_50_to_30(pps):
    st = both(R.BLEND, pps, 30, 1, 2, inputs(50, pps=pps))
    sh = R.shown(R.BLEND, st)
    assert [w for _, _, _, w in sh][:6] == [256, 171, 85, 256, 171, 85]
    assert [(a, b) for _, a, b, _ in sh][:6] == [(0, 0), (1, 2), (3, 4), (4, 5), (6, 7), (8, 9)]
    if pps == 90000:
        assert [t for t, _, _, _ in sh] == [3000 * k for k in range(len(sh))]


def test_hold_jitter_and_hole():
    rng = random.Random(7)
    pts = [i * NS // 30 + rng.randint(-8_000_000, 8_000_000) for i in range(200)]
    st = both(R.HOLD, NS, 30, 1, 2, pts)
    assert [len(s[0]) for s in st] == [1] * 200 and not any(s[2] for s in st)
    st = both(R.HOLD, NS, 30, 1, 2, [0, NS // 30, 2 * NS // 30, NS])
    assert [len(s[0]) for s in st] == [1, 1, 1, 1] and [s[2] for s in st] == [False, False, False, True] and st[3][0] == [NS]


def random_sequence(rng):
    pps = rng.choice([1000, 90000, 10 ** 6, NS])
    fi, fo = (rng.choice([(24000, 1001), (25, 1), (30000, 1001), (30, 1), (50, 1), (60, 1), (7013, 234), (15, 1), (120, 1)]) for _ in range(2))
    step = pps * fi[1] // fi[0]
    base, pts = rng.randrange(0, 10 ** 12), []
    for i in range(rng.randint(5, 60)):
        ev = rng.random()
        if ev < 0.05:
            base += step * rng.randint(1, 40)  # a hole
        elif ev < 0.08:
            base -= step * rng.randint(1, 5)   # a backward step
        j = rng.randint(-step // 3, step // 3) if rng.random() < 0.5 else 0
        pts.append(base + i * step + j)
    return rng.choice([R.HOLD, R.BLEND]), pps, fo[0], fo[1], rng.randint(0, 4), pts


def test_random_sequences_equal_the_reference():
    rng = random.Random(20241)
    seen = {"drop": 0, "multi": 0, "resync": 0, "blend": 0}
    for _ in range(2000):
        mode, pps, num, den, mf, pts = random_sequence(rng)
        for o, w, rs in both(mode, pps, num, den, mf, pts):
            seen["drop"] += not o; seen["multi"] += len(o) > 1; seen["resync"] += rs; seen["blend"] += any(0 < x < 256 for x in w)
            assert len(o) <= mf + 1
    assert all(v > 100 for v in seen.values()), seen


def test_large_anchor_gives_the_same_counts_and_weights():
    rng = random.Random(5)
    for mode, fi in ((R.HOLD, 25), (R.BLEND, 50), (R.BLEND, 25), (R.HOLD, 60)):
        pts = [i * NS // fi + rng.randint(-3_000_000, 3_000_000) for i in range(60)]
        a = both(mode, NS, 30000, 1001, 2, pts)
        b = both(mode, NS, 30000, 1001, 2, [p + 2 ** 61 for p in pts])
        assert [(len(o), w, rs) for o, w, rs in a] == [(len(o), w, rs) for o, w, rs in b]
        assert [[t + 2 ** 61 for t in o] for o, _, _ in a] == [o for o, _, _ in b]


def test_tick_pts_exact_beyond_2_32():
    # ten days of nanoseconds at N = 60000 pass 2^63 in 2 N (p - T0); ticks beyond 2^32 pass it in k D long before
    for num, den in ((60000, 1001), (240000, 1001), (30, 1)):
        k0 = 2 ** 32 + 12345
        D = NS * den
        pts = [(k0 + i) * D // num for i in range(40)]
        st = both(R.HOLD, NS, num, den, 2, pts, t0=0, k_next=k0)
        assert [o for o, _, _ in st] == [[p] for p in pts]
        half = [(2 * (k0 + i) + 1) * D // (2 * num) for i in range(0, 40, 2)]  # every other tick's midpoint to the next: 50 -> 30-like cadence
        both(R.BLEND, NS, num, den, 2, half, t0=0, k_next=k0)


def test_argument_checks():
    L = E.load()
    assert E.rate_check(1, NS, 2) and E.rate_check(0, 1, 0) and E.rate_check(2, 90000, 0)
    for bad in ((-1, NS, 2), (3, NS, 2), (1, 0, 2), (1, -5, 2), (2, NS, -1)):
        assert not E.rate_check(*bad), bad
    assert L.mi355enc_rate_check(None) == E.ERR_ARG
    assert L.mi355enc_set_rate_conversion(None, C.byref(E.Rate(1, NS, 2))) == E.ERR_ARG
    assert L.mi355enc_rate_peek(None, 0) == E.ERR_ARG and L.mi355enc_last_submit_count(None) == 0 and L.mi355enc_debug_rate_bytes(None) == 0
    assert L.mi355enc_rate_stats(None, None) == E.ERR_ARG
    assert L.mi355enc_stage_rate(None, 0, None, None, None, None, None, None) == E.ERR_ARG
    p = E.RatePlan(1, NS, 30, 1, 99)
    assert p.st.max_fill == E.RATE_MAX_OUT - 1
    n, rs = C.c_int(), C.c_int()
    assert L.mi355enc_rate_plan_step(None, 0, C.byref(n), None, None, C.byref(rs)) == E.ERR_ARG
    assert L.mi355enc_rate_plan_step(C.byref(p.st), 0, C.byref(n), None, None, C.byref(rs)) == E.ERR_ARG
