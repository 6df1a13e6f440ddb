"""GPU: automatic levels and white balance (mi355enc_set_autolevel, k_autolevel.hip) -- the measure and the decide launch alone and the
three launches on one picture bit for bit against tests/autolevelref.py, and streams: the autolevelling encoder's access units equal, byte for byte, those of a
plain encoder fed autolevelref's pictures, and every picture's record and table equal the reference's."""
import numpy as np
import pytest

from tests import autolevelref as R
from tests import denoiseref as D
from tests import rateref
from tests.test_adjust_gpu import coded
from tests.test_geometry_gpu import geom_pictures, plain_stream, same
from tests.test_yuv_convert_gpu import dev_get, dev_put
from tests.inputref import device_free

pytestmark = pytest.mark.gpu

GOP, QP = 30, 28
ON = dict(levels=900, balance=800, speed=64)


@pytest.fixture(scope="module")
def probe(E):
    e = E.Encoder(64, 48, fixed_qp=QP)
    yield e
    e.close()


# ---- the measure launch alone
# (surface W x H, rect or None, visible or None): every sample an edge; whole; margins that do not count; a border that does not count, patches straddling both
# of its edges; more patches than a workgroup's 256 along either axis; the width limit; more patches than the grid's first pass (256 workgroups x 256)
SHAPES = [(16, 16, None, None), (64, 48, None, None), (80, 64, None, (70, 50)), (80, 64, (18, 62, 10, 38), None), (1104, 48, None, None), (48, 1104, None, None),
          (8192, 16, None, None), (2048, 528, None, (2040, 522))]


def contents(W, H, full, reach, seed):
    """(name, y, uv) for one surface"""
    rng = np.random.default_rng(seed)
    B, S = R.black_scale(full)
    lb, ub = B + (S >> 3), B + S - (S >> 3)
    xx, yy = np.meshgrid(np.arange(W), np.arange(H))
    grey = np.full((H // 2, W), 128, np.uint8)
    out = [("noise", rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8))]
    out.append(("flat", np.full((H, W), 97, np.uint8), np.full((H // 2, W), 131, np.uint8)))
    out.append(("checkerboard", (((xx + yy) & 1) * 255).astype(np.uint8), ((xx[: H // 2] & 1) * 255).astype(np.uint8)))
    out.append(("ramp", ((xx + 3 * yy) & 255).astype(np.uint8), ((2 * xx[: H // 2] + yy[: H // 2]) & 255).astype(np.uint8)))
    edge = np.array([128 - reach - 1, 128 - reach, 128 + reach, 128 + reach + 1], np.int64).clip(0, 255).astype(np.uint8)
    out.append(("chroma-at-the-reach", np.full((H, W), (lb + ub) // 2, np.uint8), edge[rng.integers(0, 4, (H // 2, W))]))
    bound = np.array([lb - 1, lb, ub, ub + 1], np.uint8)
    out.append(("luma-at-the-vote-bounds", bound[rng.integers(0, 4, (H, W))], grey + rng.integers(0, 3, (H // 2, W), dtype=np.uint8)))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d%s%s" % (s[0], s[1], "-rect" if s[2] else "", "-vis%dx%d" % s[3] if s[3] else ""))
def test_probe_measure_is_bit_exact(probe, shape):
    W, H, rect, vis = shape
    rect, vis = rect or (0, W, 0, H), vis or (W, H)
    for full, reach in ((0, 48), (1, 5)):
        for name, y, uv in contents(W, H, full, reach, W + H + full):
            if W * H > 500000 and (full or name not in ("noise", "flat", "checkerboard")):
                continue  # (the large surface is there for the grid's second pass: three contents, one range)
            got = probe.autolevel_probe_measure(y, uv, rect, vis, full, reach)
            want = R.measure(y, uv, rect, vis, full, reach)
            assert np.array_equal(got.pop("hist"), want.pop("hist")), (name, full)
            assert got == want, (name, full, got, want)
            if name == "flat":
                assert want["voters"] == want["chroma"]
            if name in ("chroma-at-the-reach", "luma-at-the-vote-bounds") and W * H >= 64 * 48:
                assert 0 < want["voters"] < want["chroma"], name


def test_probe_measure_refusals(E, probe):
    y, uv = np.zeros((48, 64), np.uint8), np.zeros((24, 64), np.uint8)
    for rect, vis in (((1, 64, 0, 48), (64, 48)), ((0, 66, 0, 48), (64, 48)), ((32, 64, 0, 48), (30, 48)), ((0, 64, 0, 48), (65, 48)), ((0, 0, 0, 48), (64, 48))):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            probe.autolevel_probe_measure(y, uv, rect, vis)
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        probe.autolevel_probe_measure(y, uv, (0, 64, 0, 48), (64, 48), reach=128)


# ---- the decide launch alone
CASES = R.decide_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_probe_decide_equals_the_host_function(E, probe, case):
    _, m, a, full, state = case
    want = E.autolevel_decide(m, a, full, state, prime=state is None)
    got = probe.autolevel_probe_decide(m, a, full, state, prime=state is None)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert want[0] == R.decide(m, a, full, state, prime=state is None)[0]


def test_probe_decide_on_seeded_measurements(E, probe):
    rng = np.random.default_rng(99)
    for _ in range(150):
        m, a, full, state = R.random_case(rng)
        want = R.decide(m, a, full, state, prime=state is None)
        got = probe.autolevel_probe_decide(m, a, full, state, prime=state is None)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2]


# ---- the three launches on one picture
def saturating(w, h, seed):
    """most chroma far off grey one way, some far off the other way: with every sample voting the offsets push the few past 0 and 255"""
    rng = np.random.default_rng(seed)
    y = rng.integers(60, 200, (h, w), dtype=np.uint8)
    uv = np.empty((h // 2, w), np.uint8)
    few = rng.integers(0, 8, (h // 2, w // 2)) == 0
    uv[:, 0::2] = np.where(few, 30, 240) + rng.integers(0, 4, few.shape)
    uv[:, 1::2] = np.where(few, 235, 12) + rng.integers(0, 4, few.shape)
    return y, uv


STAGE = {"luma": dict(levels=1000, clip=100), "chroma": dict(balance=1000), "both": dict(levels=700, balance=600, max_gain=4000),
         "saturating": dict(levels=1000, balance=1000, reach=127)}


@pytest.mark.parametrize("w,h", [(70, 50), (64, 48)], ids=lambda v: str(v))
@pytest.mark.parametrize("form", list(STAGE))
def test_stage_autolevel_matches_numpy(E, form, w, h):
    W, H = coded(w, h)
    e = E.Encoder(w, h, fixed_qp=QP)
    pic = saturating(w, h, 3) if form == "saturating" else R.clip(w, h, 8, 21)[7]
    y, uv = R.with_margins(pic[0], pic[1], W, H)
    gy, guv, rec, table = e.stage_autolevel(STAGE[form], y, uv)
    wy, wuv, wrec, wtable, _ = R.step(y, uv, STAGE[form], 0, None, True, visible=(w, h))
    assert rec == wrec and np.array_equal(table, wtable)
    assert np.array_equal(gy, wy) and np.array_equal(guv, wuv)
    assert np.array_equal(gy, y) == (form == "chroma") and np.array_equal(guv, uv) == (form == "luma")
    if form == "saturating":
        assert rec["off_u"] > 60 and rec["off_v"] < -60 and (guv[:, 0::2] == 0).any() and (guv[:, 1::2] == 255).any()
    ry, ruv = R.with_margins(gy[:h, :w], guv[:h // 2, :w], W, H)
    assert np.array_equal(ry, gy) and np.array_equal(ruv, guv)  # the margins stay replicas
    assert e.debug_autolevel_bytes() > 256 * 260 * 4
    e.close()


def test_stage_autolevel_full_range_and_refused_values(E):
    w, h = 64, 48
    pic = R.clip(w, h, 3, 22)[2]
    e = E.Encoder(w, h, fixed_qp=QP, colorimetry=(1, 1, 1, 1))
    gy, guv, rec, table = e.stage_autolevel(STAGE["both"], *pic)
    wy, wuv, wrec, wtable, _ = R.step(pic[0], pic[1], STAGE["both"], 1, None, True)
    assert rec == wrec and np.array_equal(table, wtable) and np.array_equal(gy, wy) and np.array_equal(guv, wuv)
    assert not np.array_equal(wtable, R.step(pic[0], pic[1], STAGE["both"], 0, None, True)[3])
    for bad in ({}, dict(levels=1001), dict(levels=500, speed=0), dict(balance=500, reach=128), dict(levels=500, max_gain=999)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.stage_autolevel(bad, *pic)
    for bad in (dict(levels=-1), dict(clip_low=2001), dict(max_gain=8001)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.set_autolevel(bad)
    assert e.get_autolevel() == R.DEFAULT
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.last_autolevel()
    e.close()


# ---- streams
def run(e, feed, n, depth=2, before=None):
    """-> ((access units, reconstruction), the pictures' (record, table))"""
    out, recs = [], []

    def collect():
        out.append(e.collect())
        _, rec, table = e.last_autolevel()
        recs.append((rec, table))

    for i in range(n):
        if before:
            before(i)
        feed(i)
        if e.pending > depth:
            collect()
    while e.pending:
        collect()
    return (out, (e.fetch(0), e.fetch(1))), recs


def reference(pics, settings, w, h, full=0):
    """autolevelref's chain on the coded surfaces -> (its records and tables, its visible pictures)"""
    W, H = coded(w, h)
    res = R.chain([R.with_margins(y, uv, W, H) for y, uv in pics], settings, full, visible=(w, h))
    return [(r[2], r[3]) for r in res], [(np.ascontiguousarray(r[0][:h, :w]), np.ascontiguousarray(r[1][:h // 2, :w])) for r in res]


def equal_records(got, want):
    assert len(got) == len(want)
    for i, ((gr, gt), (wr, wt)) in enumerate(zip(got, want)):
        assert gr == wr and np.array_equal(gt, wt), (i, gr, wr)


def conditions(recs, pics, want):
    """on the reference, so that no stream test passes vacuously: the points move with the exposure, the cast is seen and followed, the pictures change"""
    los = [r["lo"] for r, _ in recs if r != R.ZERO]
    assert len(set(los)) >= 4 and len({r["hi"] for r, _ in recs}) >= 4
    assert any(r["off_u"] > 0 for r, _ in recs[5:]) and any(r["off_v"] < 0 for r, _ in recs[5:]) and all(r["off_u"] == 0 for r, _ in recs[:5])
    assert sum(not np.array_equal(p[0], q[0]) for p, q in zip(pics, want)) >= len(pics) - 3


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("w,h", [(64, 48), (160, 96)], ids=lambda v: str(v))
def test_stream_equals_the_plain_encoder_fed_the_references_pictures(E, w, h, depth):
    pics = R.clip(w, h)
    recs, want = reference(pics, [ON] * len(pics), w, h)
    conditions(recs, pics, want)
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, autolevel=ON)
    assert e.debug_autolevel_bytes() == 0 and e.get_autolevel() == R.params(ON)
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), len(pics), depth)
    assert e.debug_autolevel_bytes() > 256 * 260 * 4 and e.last_autolevel()[0] == R.params(ON)
    e.close()
    equal_records(infos, recs)
    same(got, ref)


@pytest.mark.parametrize("w,h", [(64, 48), (160, 96)], ids=lambda v: str(v))
def test_the_setting_is_latched_per_picture_and_off_then_on_primes(E, w, h):
    pics = R.clip(w, h)
    late = dict(levels=1000, balance=300, speed=256, clip=400, max_gain=8000, reach=20)
    settings = [ON] * 4 + [late] * 2 + [None] * 2 + [ON] * (len(pics) - 8)
    recs, want = reference(pics, settings, w, h)
    assert recs[6][0] == R.ZERO and recs[8][0]["s_lo"] == 256 * recs[8][0]["lo"] and recs[4][0]["s_hi"] == 256 * recs[4][0]["hi"]
    assert np.array_equal(want[6][0], pics[6][0]) and not np.array_equal(want[8][0], pics[8][0])
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, autolevel=ON)
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), len(pics), before=lambda i: e.set_autolevel(settings[i]))
    e.close()
    equal_records(infos, recs)
    same(got, ref)


@pytest.mark.parametrize("w,h", [(64, 48), (160, 96)], ids=lambda v: str(v))
def test_the_picture_controls_trim_on_top(E, w, h):
    """autolevel, then the controls: the plain encoder runs the same controls on the reference's pictures (the other order gives other bytes)"""
    pics = R.clip(w, h)
    adj = dict(brightness=60, contrast=1300, saturation=1400, sharpen=16)
    recs, want = reference(pics, [ON] * len(pics), w, h)
    ref = plain_stream(E, w, h, want, adjust=adj)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, autolevel=ON, adjust=adj)
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), len(pics))
    e.close()
    equal_records(infos, recs)
    same(got, ref)


@pytest.mark.parametrize("w,h", [(64, 48), (160, 96)], ids=lambda v: str(v))
def test_the_measurement_sees_the_filtered_picture(E, w, h):
    pics = R.clip(w, h, still=True)
    filtered = D.chain(pics, [(8, 8)] * len(pics))
    assert sum(not np.array_equal(f[0], p[0]) for f, p in zip(filtered, pics)) >= len(pics) - 1
    recs, want = reference(filtered, [ON] * len(pics), w, h)
    raw = reference(pics, [ON] * len(pics), w, h)[0]
    assert any(a[0] != b[0] for a, b in zip(recs, raw))
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, autolevel=ON, denoise=dict(luma=8, chroma=8))
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), len(pics))
    e.close()
    equal_records(infos, recs)
    same(got, ref)


def test_under_a_letterbox_the_border_keeps_its_bytes_and_does_not_count(E):
    iw, ih, w, h, dst = 160, 96, 128, 96, (20, 12, 80, 48)  # (2 : 1 both ways: no sample aspect ratio in the SPS, so the plain encoder writes the same one)
    rect = (dst[0], dst[0] + dst[2], dst[1], dst[1] + dst[3])
    pics = R.clip(iw, ih)
    boxed = geom_pictures(pics, (iw, ih), (0, 0, iw, ih), dst, w, h, border=(235, 60, 200))  # (a border that would move both points and the vote if it counted)
    res = R.chain(boxed, [ON] * len(pics), rect=rect)
    recs, want = [(r[2], r[3]) for r in res], [(r[0], r[1]) for r in res]
    assert all(r["hi"] < 235 for r, _ in recs) and any(r["off_u"] for r, _ in recs)
    mask = np.zeros((h, w), bool)
    mask[rect[2]:rect[3], rect[0]:rect[1]] = True
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, autolevel=ON, geometry=E.geometry((iw, ih), dst=dst, border=(235, 60, 200)))
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), len(pics))
    sy, suv = e.fetch(E.FETCH_SOURCE_Y), e.fetch(E.FETCH_SOURCE_UV)
    e.close()
    assert np.array_equal(sy, want[-1][0]) and np.array_equal(suv, want[-1][1])
    assert (sy[~mask] == 235).all() and (suv[~mask[0::2]].reshape(-1, 2) == (60, 200)).all() and not np.array_equal(sy[mask], boxed[-1][0][mask])
    equal_records(infos, recs)
    same(got, ref)


@pytest.mark.parametrize("w,h", [(64, 48), (160, 96)], ids=lambda v: str(v))
def test_dropped_inputs_leave_no_trace_in_the_state(E, w, h):
    """hold at half rate: every other input is dropped before it is transferred, and the state steps from kept picture to kept picture"""
    pics = R.clip(w, h)
    rate = (rateref.HOLD, 120, 0)  # inputs at 120 pts units a second into a 60 fps stream
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, autolevel=ON, rate=rate)
    counts = []
    got, infos = run(e, lambda i: counts.append(e.submit(*pics[i], pts=i)), len(pics))
    e.close()
    kept = [i for i, c in enumerate(counts) if c]
    assert set(counts) == {0, 1} and len(infos) == len(kept) and 4 <= len(kept) < len(pics)
    recs, want = reference([pics[i] for i in kept], [ON] * len(kept), w, h)
    every = reference(pics, [ON] * len(pics), w, h)[0]
    assert any(a[0] != every[i][0] for a, i in zip(recs, kept))  # (had the dropped ones been measured, the state would be another)
    fed = list(pics)
    for i, p in zip(kept, want):
        fed[i] = p
    ref = plain_stream(E, w, h, fed, rate=rate)
    equal_records(infos, recs)
    same(got, ref)


def test_a_repeated_picture_is_corrected_once(E):
    w, h, ns = 64, 48, 10 ** 9
    pics = R.clip(w, h)
    recs, want = reference(pics[:2], [ON] * 2, w, h)
    e = E.Encoder(w, h, fps=60, gop=GOP, fixed_qp=QP, pipeline_depth=2, rate=(rateref.HOLD, ns, 2), autolevel=ON)
    assert e.submit(*pics[0], pts=0) == 1
    e.collect()
    first = (e.fetch(E.FETCH_SOURCE_Y), e.fetch(E.FETCH_SOURCE_UV))
    assert np.array_equal(first[0], want[0][0]) and np.array_equal(first[1], want[0][1]) and e.last_autolevel()[1] == recs[0][0]
    assert e.submit(*pics[1], pts=ns // 30) == 2  # the tick in between repeats the first picture
    e.collect()
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), first[0]) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), first[1]) and e.last_autolevel()[1] == R.ZERO
    e.collect()
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), want[1][0]) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), want[1][1]) and e.last_autolevel()[1] == recs[1][0]
    e.close()


def test_submit_device_never_corrects_the_callers_planes(E):
    """64 x 48 on aligned planes would take the in-place exit: with the step on it must not, and the planes stay what they were"""
    w, h = 64, 48
    pics = R.clip(w, h, 3)
    recs, want = reference(pics, [ON] * 3, w, h)
    ref = plain_stream(E, w, h, want)
    dev = [(dev_put(y), dev_put(uv)) for y, uv in pics]
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, autolevel=ON)
    got, infos = run(e, lambda i: e.submit_device(dev[i][0], w, dev[i][1], w, pts=i), 3)
    e.close()
    for (dy, duv), (y, uv) in zip(dev, pics):
        assert np.array_equal(dev_get(dy, y.shape), y) and np.array_equal(dev_get(duv, uv.shape), uv)
        device_free(dy); device_free(duv)
    equal_records(infos, recs)
    same(got, ref)


# ---- off
def test_off_is_off(E):
    w, h = 64, 48
    pics = R.clip(w, h, 5)
    ref = plain_stream(E, w, h, pics)
    never = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    got, infos = run(never, lambda i: never.submit(*pics[i], pts=i), 5)
    assert never.debug_autolevel_bytes() == 0 and all(r == R.ZERO and not t.any() for r, t in infos)
    same(got, ref)
    zero = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, autolevel=dict(levels=0, balance=0, speed=256, clip=0, max_gain=8000, reach=127))
    assert zero.get_autolevel() == R.DEFAULT  # both strengths 0: off, and the defaults are reported
    got, infos = run(zero, lambda i: zero.submit(*pics[i], pts=i), 5)
    assert zero.debug_autolevel_bytes() == 0 and all(r == R.ZERO for r, _ in infos)
    same(got, ref)
    for stage in (E.STAGE_AUTOLEVEL_MEASURE, E.STAGE_AUTOLEVEL_DECIDE, E.STAGE_AUTOLEVEL_APPLY):
        with pytest.raises(E.EncoderError, match=r"\(-6\)"):
            zero.time_stage(stage, 2)
    assert zero.debug_autolevel_bytes() == 0
    never.close(); zero.close()


def test_timed_stages_run_when_on_and_leave_the_state_unprimed(E):
    w, h = 64, 48
    pics = R.clip(w, h)
    recs, _ = reference(pics[:2], [ON] * 2, w, h)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, autolevel=ON)
    e.submit(*pics[0], pts=0)
    e.submit(*pics[1], pts=1)
    e.collect(); e.collect()
    assert e.last_autolevel()[1] == recs[1][0] and recs[1][0]["s_lo"] != 256 * recs[1][0]["lo"]
    for stage in (E.STAGE_AUTOLEVEL_MEASURE, E.STAGE_AUTOLEVEL_DECIDE, E.STAGE_AUTOLEVEL_APPLY):
        assert e.time_stage(stage, 3) > 0
    e.submit(*pics[2], pts=2)  # primes: the state the probes left is no picture's
    e.collect()
    assert e.last_autolevel()[1] == reference(pics[2:3], [ON], w, h)[0][0][0]
    # both probes and the stage call refuse pictures in flight
    e.submit(*pics[3], pts=3)
    y, uv = pics[0]
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.autolevel_probe_measure(y, uv, (0, w, 0, h), (w, h))
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.autolevel_probe_decide(R.measure(y, uv), ON, prime=True)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.stage_autolevel(ON, y, uv)
    e.collect()
    e.close()
