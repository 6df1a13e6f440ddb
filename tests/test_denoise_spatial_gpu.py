"""GPU: the spatial noise filter and its noise estimate (mi355enc_set_denoise_spatial, k_dspatial.hip) -- the filter launches, the measure
and the decide launch alone bit for bit against tests/dspatialref.py, and streams: the filtering encoder's access units equal, byte for byte, those of a plain
encoder fed dspatialref's pictures, and every picture's record equals the reference's."""
import numpy as np
import pytest

from tests import denoiseref as D
from tests import dspatialref as R
from tests import rateref
from tests.test_geometry_gpu import GOP, QP, geom_pictures, plain_stream, same
from tests.test_yuv_convert_gpu import dev_get, dev_put
from tests.inputref import device_free

pytestmark = pytest.mark.gpu

MANUAL = dict(luma=6, chroma=4)
AUTO = dict(luma=32, chroma=32, auto_gain=2000, speed=128)
SIGMAS = [1, 1, 4, 4, 2, 6]


def coded(w, h):
    return (w + 15) // 16 * 16, (h + 15) // 16 * 16


# ---- the filter launches alone
# (visible size, geometry's destination or None): every neighbour clamped; whole; margins; a border with tiles straddling both edges; more tiles than one along
# either axis; the width limit
FILTER_SHAPES = [((16, 16), None), ((64, 48), None), ((70, 50), None), ((80, 64), (18, 10, 44, 28)), ((144, 32), None), ((1104, 48), None), ((48, 1104), None),
                 ((8192, 16), None)]


def thresholds(shape, s, rng):
    """samples c, c +- s, c +- (s + 1), c +- (3 s - 1), c +- 3 s at random: every boundary of the table"""
    off = np.array([0, s, -s, s + 1, -s - 1, 3 * s - 1, 1 - 3 * s, 3 * s, -3 * s], np.int64)
    return (128 + off[rng.integers(0, 9, shape)]).astype(np.uint8)


def filter_contents(W, H, s, seed):
    rng = np.random.default_rng(seed)
    xx, yy = np.meshgrid(np.arange(W), np.arange(H))
    return [("noise", rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)),
            ("flat", np.full((H, W), 97, np.uint8), np.full((H // 2, W), 131, np.uint8)),
            ("checkerboard", (((xx + yy) & 1) * 255).astype(np.uint8), ((((xx >> 1) + yy)[: H // 2] & 1) * 255).astype(np.uint8)),
            ("ramp", ((xx + yy) & 255).astype(np.uint8), (((xx >> 1) + yy)[: H // 2] & 255).astype(np.uint8)),
            ("thresholds", thresholds((H, W), s, rng), thresholds((H // 2, W), s, rng))]


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=lambda s: "%dx%d%s" % (s[0][0], s[0][1], "-border" if s[1] else ""))
def test_the_filter_launches_are_bit_exact(E, shape):
    (w, h), dst = shape
    W, H = coded(w, h)
    e = E.Encoder(w, h, fixed_qp=QP, geometry=E.geometry((160, 96), dst=dst) if dst else None)
    rect = (dst[0], dst[0] + dst[2], dst[1], dst[1] + dst[3]) if dst else (0, W, 0, H)
    changed = 0
    for s in (1, 8, 32):
        for name, y, uv in filter_contents(W, H, s, W + H + s):
            for luma, chroma in ((s, s), (s, 0), (0, s)) if name in ("noise", "thresholds") else ((s, s),):
                gy, guv, rec = e.stage_denoise_spatial(dict(luma=luma, chroma=chroma), y, uv)
                wy, wuv = R.apply(y, uv, luma or None, chroma or None, rect, (w, h))
                assert np.array_equal(gy, wy), (name, s, luma, chroma, np.argwhere(gy != wy)[:4])
                assert np.array_equal(guv, wuv), (name, s, luma, chroma, np.argwhere(guv != wuv)[:4])
                assert rec == dict(R.ZERO, s_luma=luma, s_chroma=chroma)
                inside = (slice(rect[2], min(rect[3], h)), slice(rect[0], min(rect[1], w)))
                if name in ("flat", "checkerboard"):  # nothing to average / every difference beyond 3 s: the identity
                    assert np.array_equal(gy[inside], y[inside])
                changed += name == "noise" and s == 32 and luma > 0 and not np.array_equal(gy[inside], y[inside])
                if dst:
                    mask = np.zeros((H, W), bool)
                    mask[rect[2]:rect[3], rect[0]:rect[1]] = True
                    assert np.array_equal(gy[~mask], y[~mask]) and np.array_equal(guv[~mask[0::2]], uv[~mask[0::2]])
    assert changed == 2 and e.debug_denoise_spatial_bytes() == W * H * 3 // 2  # (manual: the two scratch planes and nothing else)
    e.close()


def test_stage_automatic_and_refused_values(E):
    w, h = 70, 50
    W, H = coded(w, h)
    e = E.Encoder(w, h, fixed_qp=QP)
    y, uv = R.with_margins(*R.noisy_clip(w, h, 1, [1])[0], W, H)
    for a in (AUTO, dict(AUTO, chroma=0), dict(AUTO, luma=2), dict(auto_gain=1000), dict(luma=9, chroma=9, auto_gain=250)):
        gy, guv, rec = e.stage_denoise_spatial(a, y, uv)
        (wy, wuv, wrec), = R.chain([(y, uv)], [a], visible=(w, h))
        assert rec == wrec and rec["valid"] and rec["v"] > 3 and np.array_equal(gy, wy) and np.array_equal(guv, wuv), (a, rec, wrec)
        if a.get("luma"):
            ry, ruv = R.with_margins(gy[:h, :w], guv[:h // 2, :w], W, H)
            assert np.array_equal(ry, gy) and (not a.get("chroma") or np.array_equal(ruv, guv))  # the margins stay replicas
    assert wrec["s_luma"] == 0 and np.array_equal(gy[:h, :w], y[:h, :w])  # (a quarter of sigma 1 rounds to 0: copied through)
    assert e.debug_denoise_spatial_bytes() > 256 * 256 * 4 + W * H * 3 // 2
    for bad in ({}, dict(luma=33), dict(luma=4, speed=0), dict(chroma=4, percentile=51), dict(luma=4, auto_gain=249), dict(luma=4, auto_gain=8001)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.stage_denoise_spatial(bad, y, uv)
    for bad in (dict(luma=-1), dict(chroma=33), dict(luma=1, percentile=0), dict(luma=1, speed=257), dict(auto_gain=100)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.set_denoise_spatial(bad)
    assert e.get_denoise_spatial() == R.DEFAULT
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.last_denoise_spatial()
    e.close()


# ---- the measure launch alone
@pytest.fixture(scope="module")
def probe(E):
    e = E.Encoder(64, 48, fixed_qp=QP)
    yield e
    e.close()


# the filter's shapes as surfaces, and two for the capped grid: 2048 x 528 (the issue's), and 8192 x 528 -- 66 495 candidates, more than 256 workgroups of 256
# blocks take in one pass
MEASURE_SHAPES = [(16, 16, None, None), (64, 48, None, None), (80, 64, None, (70, 50)), (80, 64, (18, 62, 10, 38), None), (144, 32, None, None),
                  (1104, 48, None, None), (48, 1104, None, None), (8192, 16, None, None), (2048, 528, None, (2040, 522)), (8192, 528, None, (8190, 522))]


def measure_contents(W, H, full, seed):
    rng = np.random.default_rng(seed)
    B, S = R.black_scale(full)
    lo, hi = B + (S >> 4), B + S - (S >> 4)
    xx = np.arange(W)[None, :]
    noise = np.clip(np.rint(120 + (xx % 97) / 8.0 * rng.standard_normal((H, W))), 0, 255).astype(np.uint8)  # sigma 0 .. 12 across: many bins
    # per 8 x 8 block: flat at the lower bound (votes), one sample below it (does not), flat at the upper bound (votes), one sample above it (does not)
    kind = np.kron(rng.integers(0, 4, ((H + 7) // 8, (W + 7) // 8)), np.ones((8, 8), np.int64))[:H, :W]
    bounds = np.where(kind < 2, lo, hi).astype(np.int64)
    yy = np.arange(H)[:, None]
    bounds += np.where((kind & 1) & (yy % 8 == 3) & (xx % 8 == 4), np.where(kind < 2, -1, 1), 0)
    return [("flat", np.full((H, W), 97, np.uint8)), ("noise", noise), ("vote-bounds", bounds.astype(np.uint8))]


@pytest.mark.parametrize("shape", MEASURE_SHAPES, ids=lambda s: "%dx%d%s%s" % (s[0], s[1], "-rect" if s[2] else "", "-vis%dx%d" % s[3] if s[3] else ""))
def test_probe_measure_is_bit_exact(E, probe, shape):
    W, H, rect, vis = shape
    for full in (0, 1):
        for name, y in measure_contents(W, H, full, W + H + full):
            if W * H > 500000 and full:
                continue  # (the large surfaces are there for the grid's second pass: one range)
            got = probe.denoise_spatial_probe_measure(y, rect, vis, full)
            want = R.measure(y, rect, vis, full)
            host = E.denoise_spatial_measure_host(y, rect, vis, full)
            assert np.array_equal(got.pop("hist"), want["hist"]) and np.array_equal(host.pop("hist"), want.pop("hist")), (name, full)
            assert got == want and host == want, (name, full, got, want)
            if name == "flat":
                assert want["voters"] == want["candidates"]
            if name == "vote-bounds" and W * H >= 64 * 48:
                assert 0 < want["voters"] < want["candidates"], name
    assert (W, H) != (8192, 528) or want["candidates"] > 256 * 256


def test_probe_measure_refusals(E, probe):
    y = np.zeros((48, 64), np.uint8)
    for rect, vis in (((1, 64, 0, 48), (64, 48)), ((0, 66, 0, 48), (64, 48)), ((32, 64, 0, 48), (30, 48)), ((0, 64, 0, 48), (65, 48)), ((0, 0, 0, 48), (64, 48))):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            probe.denoise_spatial_probe_measure(y, rect, vis)


# ---- the decide launch alone
CASES = R.decide_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_probe_decide_equals_the_host_function(E, probe, case):
    _, m, a, x = case
    want = E.denoise_spatial_decide(m, a, x, prime=x is None)
    assert probe.denoise_spatial_probe_decide(m, a, x, prime=x is None) == want
    assert want == R.decide(m, a, x, prime=x is None)


def test_probe_decide_on_seeded_measurements(E, probe):
    rng = np.random.default_rng(99)
    for _ in range(100):
        bins = rng.integers(0, 256, int(rng.integers(0, 400)))
        m = dict(hist=np.bincount(bins, minlength=256), voters=len(bins), candidates=len(bins) + int(rng.integers(0, 20)) * len(bins) + int(rng.integers(0, 9)))
        a = dict(luma=int(rng.integers(0, 33)), chroma=int(rng.integers(0, 33)), auto_gain=int(rng.integers(250, 8001)), percentile=int(rng.integers(1, 51)),
                 speed=int(rng.integers(1, 257)))
        x = None if rng.integers(0, 4) == 0 else int(rng.integers(0, 65281))
        assert probe.denoise_spatial_probe_decide(m, a, x, prime=x is None) == R.decide(m, a, x, prime=x is None)


# ---- streams
def run(e, feed, n, depth=2, before=None):
    """-> ((access units, reconstruction), the pictures' records)"""
    out, recs = [], []

    def collect():
        out.append(e.collect())
        recs.append(e.last_denoise_spatial()[1])

    for i in range(n):
        if before:
            before(i)
        feed(i)
        if e.pending > depth:
            collect()
    while e.pending:
        collect()
    return (out, (e.fetch(0), e.fetch(1))), recs


def reference(pics, settings, w, h):
    """dspatialref's chain on the coded surfaces -> (its records, its visible pictures)"""
    W, H = coded(w, h)
    res = R.chain([R.with_margins(y, uv, W, H) for y, uv in pics], settings, visible=(w, h))
    return [r[2] for r in res], [(np.ascontiguousarray(r[0][:h, :w]), np.ascontiguousarray(r[1][:h // 2, :w])) for r in res]


SIZES = [(64, 48), (80, 64)]


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_manual_stream_equals_the_plain_encoder_fed_the_references_pictures(E, w, h):
    pics = R.noisy_clip(w, h, 6, SIGMAS)
    recs, want = reference(pics, [MANUAL] * 6, w, h)
    assert all(not np.array_equal(p[0], q[0]) and not np.array_equal(p[1], q[1]) for p, q in zip(pics, want))
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, denoise_spatial=MANUAL)
    assert e.debug_denoise_spatial_bytes() == 0 and e.get_denoise_spatial() == R.params(MANUAL)
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), 6)
    assert e.debug_denoise_spatial_bytes() == w * h * 3 // 2 and e.last_denoise_spatial()[0] == R.params(MANUAL)
    e.close()
    assert infos == recs
    same(got, ref)


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_automatic_stream_follows_the_noise_level(E, w, h, depth):
    pics = R.noisy_clip(w, h, 6, SIGMAS)
    recs, want = reference(pics, [AUTO] * 6, w, h)
    # on the reference, so that the test does not pass vacuously: the estimate and the strength move with the noise, smoothed
    assert all(r["valid"] and r["voters"] == r["candidates"] == (w // 8) * (h // 8) for r in recs)
    assert recs[0]["x"] == 256 * recs[0]["v"] and recs[2]["v"] > 2 * recs[1]["v"] and recs[1]["x"] < recs[2]["x"] < 256 * recs[2]["v"]
    assert len({r["s_luma"] for r in recs}) >= 3 and all(r["s_luma"] == r["s_chroma"] > 0 for r in recs)
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise_spatial=AUTO)
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), 6, depth)
    assert e.debug_denoise_spatial_bytes() > 256 * 256 * 4 + w * h * 3 // 2
    e.close()
    assert infos == recs
    same(got, ref)


def test_measure_only_leaves_the_pictures_alone_and_still_reports(E):
    w, h = 64, 48
    pics = R.noisy_clip(w, h, 6, SIGMAS)
    only = dict(auto_gain=1000, speed=256)
    recs, want = reference(pics, [only] * 6, w, h)
    assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(pics, want))
    assert len({r["x"] for r in recs}) >= 4 and all(r["s_luma"] == r["s_chroma"] == 0 and r["valid"] for r in recs)
    ref = plain_stream(E, w, h, pics)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, denoise_spatial=only)
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), 6)
    assert 0 < e.debug_denoise_spatial_bytes() < 256 * 256 * 4 + 40000  # (the block, and no scratch plane)
    e.close()
    assert infos == recs
    same(got, ref)


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_the_setting_is_latched_per_picture_and_primes_again(E, w, h):
    """a strength written between two submits takes effect on the next picture; manual -> automatic and off -> on prime"""
    sig = SIGMAS + [3, 3, 5, 5]
    pics = R.noisy_clip(w, h, 10, sig)
    settings = [MANUAL, dict(luma=12), AUTO, AUTO, dict(chroma=9), AUTO, None, AUTO, AUTO, dict(AUTO, luma=2, speed=256)]
    recs, want = reference(pics, settings, w, h)
    assert recs[1] == dict(R.ZERO, s_luma=12) and np.array_equal(want[1][1], pics[1][1]) and recs[6] == R.ZERO and np.array_equal(want[6][0], pics[6][0])
    assert all(recs[i]["x"] == 256 * recs[i]["v"] for i in (2, 5, 7)) and recs[3]["x"] != 256 * recs[3]["v"] and recs[8]["x"] != 256 * recs[8]["v"]
    assert recs[9]["s_luma"] == 2 < recs[9]["s_chroma"]
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), 10, before=lambda i: e.set_denoise_spatial(settings[i]))
    e.close()
    assert infos == recs
    same(got, ref)


@pytest.mark.parametrize("setting", [MANUAL, AUTO], ids=["manual", "automatic"])
def test_the_temporal_filter_follows_the_spatial_one(E, setting):
    """both on: dspatialref's pictures through denoiseref's chain (the other order gives other bytes)"""
    w, h = 64, 48
    pics = R.noisy_clip(w, h, 6, [3] * 6)
    recs, spatial = reference(pics, [setting] * 6, w, h)
    want = D.chain(spatial, [(8, 8)] * 6)
    other = reference(D.chain(pics, [(8, 8)] * 6), [setting] * 6, w, h)[1]
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(want, other))
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, denoise_spatial=setting, denoise=dict(luma=8, chroma=8))
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), 6)
    e.close()
    assert infos == recs
    same(got, ref)


@pytest.mark.parametrize("setting", [MANUAL, AUTO], ids=["manual", "automatic"])
def test_under_a_letterbox_the_border_keeps_its_bytes_and_does_not_count(E, setting):
    iw, ih, w, h, dst = 88, 56, 80, 64, (18, 10, 44, 28)  # (2 : 1 both ways: no sample aspect ratio in the SPS, so the plain encoder writes the same one)
    rect = (dst[0], dst[0] + dst[2], dst[1], dst[1] + dst[3])
    pics = R.noisy_clip(iw, ih, 6, [2 * s for s in SIGMAS])
    boxed = geom_pictures(pics, (iw, ih), (0, 0, iw, ih), dst, w, h, border=(235, 60, 200))
    res = R.chain(boxed, [setting] * 6, rect=rect)
    recs, want = [r[2] for r in res], [(r[0], r[1]) for r in res]
    if setting is AUTO:
        assert all(r["candidates"] == 4 * 2 and r["valid"] for r in recs) and len({r["s_luma"] for r in recs}) >= 2  # the blocks wholly inside (18 .. 62, 10 .. 38)
    mask = np.zeros((h, w), bool)
    mask[rect[2]:rect[3], rect[0]:rect[1]] = True
    ref = plain_stream(E, w, h, want)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, denoise_spatial=setting, geometry=E.geometry((iw, ih), dst=dst, border=(235, 60, 200)))
    got, infos = run(e, lambda i: e.submit(*pics[i], pts=i), 6)
    sy, suv = e.fetch(E.FETCH_SOURCE_Y), e.fetch(E.FETCH_SOURCE_UV)
    e.close()
    assert np.array_equal(sy, want[-1][0]) and np.array_equal(suv, want[-1][1])
    assert (sy[~mask] == 235).all() and (suv[~mask[0::2]].reshape(-1, 2) == (60, 200)).all() and not np.array_equal(sy[mask], boxed[-1][0][mask])
    assert infos == recs
    same(got, ref)


def test_a_repeated_picture_was_filtered_once(E):
    w, h, ns = 64, 48, 10 ** 9
    pics = R.noisy_clip(w, h, 2, [3, 3])
    recs, want = reference(pics, [AUTO] * 2, w, h)
    e = E.Encoder(w, h, fps=60, gop=GOP, fixed_qp=QP, pipeline_depth=2, rate=(rateref.HOLD, ns, 2), denoise_spatial=AUTO)
    assert e.submit(*pics[0], pts=0) == 1
    e.collect()
    first = (e.fetch(E.FETCH_SOURCE_Y), e.fetch(E.FETCH_SOURCE_UV))
    assert np.array_equal(first[0], want[0][0]) and np.array_equal(first[1], want[0][1]) and e.last_denoise_spatial()[1] == recs[0]
    assert e.submit(*pics[1], pts=ns // 30) == 2  # the tick in between repeats the first picture
    e.collect()
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), first[0]) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), first[1])
    assert e.last_denoise_spatial() == (R.params(AUTO), R.ZERO)  # (the tick's slot latched the setting only)
    e.collect()
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), want[1][0]) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), want[1][1]) and e.last_denoise_spatial()[1] == recs[1]
    e.close()


def test_dropped_inputs_are_never_measured(E):
    w, h = 64, 48
    pics = R.noisy_clip(w, h, 10, SIGMAS + [3, 3, 5, 5])
    rate = (rateref.HOLD, 120, 0)  # inputs at 120 pts units a second into a 60 fps stream
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, denoise_spatial=AUTO, rate=rate)
    counts = []
    got, infos = run(e, lambda i: counts.append(e.submit(*pics[i], pts=i)), 10)
    e.close()
    kept = [i for i, c in enumerate(counts) if c]
    assert set(counts) == {0, 1} and len(infos) == len(kept) and 4 <= len(kept) < 10
    recs, want = reference([pics[i] for i in kept], [AUTO] * len(kept), w, h)
    every = reference(pics, [AUTO] * 10, w, h)[0]
    assert any(a != every[i] for a, i in zip(recs, kept))  # (had the dropped ones been measured, the state would be another)
    fed = list(pics)
    for i, p in zip(kept, want):
        fed[i] = p
    ref = plain_stream(E, w, h, fed, rate=rate)
    assert infos == recs
    same(got, ref)


def test_submit_device_never_filters_the_callers_planes(E):
    """64 x 48 on aligned planes would take the in-place exit: with the step on it must not, and the planes stay what they were"""
    w, h = 64, 48
    pics = R.noisy_clip(w, h, 3, [3] * 3)
    for setting in (MANUAL, dict(auto_gain=1000)):
        recs, want = reference(pics, [setting] * 3, w, h)
        ref = plain_stream(E, w, h, want)
        dev = [(dev_put(y), dev_put(uv)) for y, uv in pics]
        e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, denoise_spatial=setting)
        got, infos = run(e, lambda i: e.submit_device(dev[i][0], w, dev[i][1], w, pts=i), 3)
        e.close()
        for (dy, duv), (y, uv) in zip(dev, pics):
            assert np.array_equal(dev_get(dy, y.shape), y) and np.array_equal(dev_get(duv, uv.shape), uv)
            device_free(dy); device_free(duv)
        assert infos == recs
        same(got, ref)


# ---- off
def test_off_is_off(E):
    w, h = 64, 48
    pics = R.noisy_clip(w, h, 5, SIGMAS)
    ref = plain_stream(E, w, h, pics)
    never = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    got, infos = run(never, lambda i: never.submit(*pics[i], pts=i), 5)
    assert never.debug_denoise_spatial_bytes() == 0 and all(r == R.ZERO for r in infos)
    same(got, ref)
    zero = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, denoise_spatial=dict(luma=0, chroma=0, auto_gain=0, percentile=50, speed=256))
    assert zero.get_denoise_spatial() == R.DEFAULT  # nothing filters or measures: off, and the defaults are reported
    got, infos = run(zero, lambda i: zero.submit(*pics[i], pts=i), 5)
    assert zero.debug_denoise_spatial_bytes() == 0 and all(r == R.ZERO for r in infos)
    same(got, ref)
    for stage in (E.STAGE_DENOISE_SPATIAL, E.STAGE_DENOISE_SPATIAL_AUTO):
        with pytest.raises(E.EncoderError, match=r"\(-6\)"):
            zero.time_stage(stage, 2)
    assert zero.debug_denoise_spatial_bytes() == 0
    never.close(); zero.close()


def test_timed_stages_run_when_on_and_leave_the_state_unprimed(E):
    w, h = 64, 48
    pics = R.noisy_clip(w, h, 4, [1, 4, 2, 2])
    recs, _ = reference(pics[:2], [AUTO] * 2, w, h)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, denoise_spatial=AUTO)
    e.submit(*pics[0], pts=0)
    e.submit(*pics[1], pts=1)
    e.collect(); e.collect()
    assert e.last_denoise_spatial()[1] == recs[1] and recs[1]["x"] != 256 * recs[1]["v"]
    assert e.time_stage(E.STAGE_DENOISE_SPATIAL_AUTO, 3) > 0
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.time_stage(E.STAGE_DENOISE_SPATIAL, 3)  # (the manual stage with an automatic setting)
    e.submit(*pics[2], pts=2)  # primes: the state the timed launches left is no picture's
    e.collect()
    assert e.last_denoise_spatial()[1] == reference(pics[2:3], [AUTO], w, h)[0][0]
    e.set_denoise_spatial(MANUAL)
    assert e.time_stage(E.STAGE_DENOISE_SPATIAL, 3) > 0
    # both probes and the stage call refuse pictures in flight
    e.submit(*pics[3], pts=3)
    y, uv = pics[0]
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.denoise_spatial_probe_measure(y)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.denoise_spatial_probe_decide(R.measure(y), AUTO, prime=True)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.stage_denoise_spatial(MANUAL, y, uv)
    e.collect()
    e.close()
