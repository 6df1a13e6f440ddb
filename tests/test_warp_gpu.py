"""GPU: lens, roll and keystone correction (mi355enc_set_warp / mi355enc_set_warp_mesh, k_warp.hip) -- the launch alone bit-exact against
tests/warpref.py for every named set, both filters and every size, margin included, and streams: the warping encoder's access units and reconstruction equal,
byte for byte, those of a plain encoder fed warpref's pictures."""
import numpy as np
import pytest

from tests import rateref
from tests import warpref as R
from tests.test_geometry_gpu import nv12_clip, plain_stream, same
from tests.test_yuv_convert_gpu import dev_get, dev_put

pytestmark = pytest.mark.gpu

GOP, QP, N = 30, 28, 8
W, H = 160, 96
FILL = (40, 90, 200)
_ENC = {}


@pytest.fixture(scope="module")
def stage(E):
    """one handle per size, shared by the launch tests"""
    def get(w, h):
        if (w, h) not in _ENC:
            _ENC[(w, h)] = E.Encoder(w, h, fixed_qp=QP)
        return _ENC[(w, h)]
    yield get
    for e in _ENC.values():
        e.close()
    _ENC.clear()


def coded_noise(w, h, seed):
    """coded-size planes, noise in the margin too: the launch must not read it"""
    Wc, Hc = (w + 15) & ~15, (h + 15) & ~15
    return R.noise(Wc, Hc, seed)


def expect(kind, mesh, y, uv, w, h, fill=FILL):
    return R.pad(*R.apply(kind, fill, mesh, np.ascontiguousarray(y[:h, :w]), np.ascontiguousarray(uv[:h // 2, :w])))


def check_launch(e, mesh, w, h, seed):
    """both filters, as the launch chooses its form per tile and with every tile in the direct form"""
    y, uv = coded_noise(w, h, seed)
    for kind in (0, 1):
        ry, ruv = expect(kind, mesh, y, uv, w, h)
        for staging in (True, False):
            e.debug_warp_staging(staging)
            gy, guv = e.stage_warp(dict(kind=kind, fill=FILL), mesh, y, uv)
            assert np.array_equal(gy, ry), (kind, staging, np.argwhere(gy != ry)[:4])
            assert np.array_equal(guv, ruv), (kind, staging, np.argwhere(guv != ruv)[:4])
    e.debug_warp_staging(True)


# ---- the launch alone
@pytest.mark.parametrize("size", R.SIZES + R.STRIPS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(R.SETS))
def test_stage_warp_is_bit_exact(stage, name, size):
    w, h = size
    check_launch(stage(w, h), R.build(w, h, **R.SETS[name]), w, h, 10 * w + h)


def test_stage_warp_identity_is_a_copy_with_the_margin_repeated(stage):
    w, h = 72, 40
    y, uv = coded_noise(w, h, 5)
    for kind in (0, 1):
        gy, guv = stage(w, h).stage_warp(dict(kind=kind), R.identity(w, h), y, uv)
        ry, ruv = R.pad(y[:h, :w], uv[:h // 2, :w])
        assert np.array_equal(gy, ry) and np.array_equal(guv, ruv)


@pytest.mark.parametrize("seed", [7, 8])
def test_stage_warp_through_a_folded_mesh(stage, seed):
    w, h = 72, 40
    m = R.random_mesh(w, h, seed)
    assert 0.1 < R.outside_fraction(m, w, h) < 0.9 and R.plan(m, w, h)[0] > 0
    check_launch(stage(w, h), m, w, h, seed)


def test_stage_warp_refuses_an_invalid_mesh(E, stage):
    w, h = 64, 48
    y, uv = coded_noise(w, h, 1)
    m = R.identity(w, h)
    m[1, 1, 0] = R.NODE_MAX + 1
    with pytest.raises(E.EncoderError):
        stage(w, h).stage_warp(dict(kind=1), m, y, uv)
    with pytest.raises(E.EncoderError):
        stage(w, h).stage_warp(dict(kind=2), R.identity(w, h), y, uv)


def test_conditions_on_the_reference():
    """so that no case above passes vacuously"""
    out = {n: R.outside_fraction(R.build(W, H, **p), W, H) for n, p in R.SETS.items()}
    assert out["barrel"] == 0 and out["all"] == 0
    assert 0.05 < out["keystone"] < 0.15
    assert 1 - out["shrink"] >= 0.10 and out["shrink"] > 0.5
    staged, direct = R.plan(R.build(W, H, **R.SETS["shrink"]), W, H)
    assert staged > 0 and direct > 0  # neither form goes untested
    for w, h in R.SIZES + R.STRIPS:  # ... at any size: every set has tiles of the staged form, and from 96 x 96 on one set at least sends some to the direct form
        plans = [R.plan(R.build(w, h, **p), w, h) for p in R.SETS.values()]
        assert all(s > 0 for s, _ in plans) and (max(w, h) < 96 or any(d > 0 for _, d in plans)), (w, h, plans)
    y, uv = R.noise(W, H, 3)
    m = R.build(W, H, **R.SETS["barrel"])
    assert (R.apply(0, FILL, m, y, uv)[0] != R.apply(1, FILL, m, y, uv)[0]).mean() >= 0.8


# ---- streams
def run(e, feed, n, depth=2, before=None):
    """-> ((access units, reconstruction), the generation every collected picture reports)"""
    out, gens = [], []
    for i in range(n):
        if before:
            before(i)
        feed(i)
        if e.pending > depth:
            out.append(e.collect())
            gens.append(e.last_warp())
    while e.pending:
        out.append(e.collect())
        gens.append(e.last_warp())
    return (out, (e.fetch(0), e.fetch(1))), gens


@pytest.fixture(scope="module")
def clip():
    return nv12_clip(W, H, N, 2700)


def warped(pics, sets, kind=1, fill=FILL):
    """the reference's pictures: sets[i] the parameter set of picture i"""
    return [R.apply(kind, fill, R.build(W, H, **p), y, uv) for (y, uv), p in zip(pics, sets)]


def test_off_is_byte_identical_and_allocates_nothing(E, clip):
    ref = plain_stream(E, W, H, clip)
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    assert e.get_warp() is None
    e.set_warp(dict(kind=1, fill=FILL), **R.SETS["all"])
    assert e.get_warp() == dict(kind=1, fill=FILL)
    e.set_warp(None)
    assert e.get_warp() is None
    with pytest.raises(E.EncoderError):
        e.last_warp()  # before the first collect
    got, gens = run(e, lambda i: e.submit(*clip[i], pts=i), N)
    assert e.debug_warp_bytes() == 0 and gens == [0] * N
    e.close()
    same(got, ref)


@pytest.mark.parametrize("depth", [0, 2])
def test_stream_equals_the_plain_encoder_fed_the_references_pictures(E, clip, depth):
    ref = plain_stream(E, W, H, warped(clip, [R.SETS["all"]] * N))
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    e.set_warp(dict(kind=1, fill=FILL), **R.SETS["all"])
    assert e.debug_warp_bytes() == 0
    got, gens = run(e, lambda i: e.submit(*clip[i], pts=i), N, depth=depth)
    assert e.debug_warp_bytes() >= W * H * 3 // 2 and gens == [1] * N
    e.close()
    same(got, ref)


@pytest.mark.parametrize("depth", [0, 2])
def test_a_set_in_mid_stream_takes_the_next_picture(E, clip, depth):
    sets = [R.SETS["barrel"]] * 4 + [R.SETS["keystone"]] * 4
    ref = plain_stream(E, W, H, warped(clip, sets))
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    e.set_warp(dict(kind=1, fill=FILL), **sets[0])

    def before(i):
        if i == 4:  # (with depth 2, pictures 2 and 3 are still in flight and keep the mesh they latched)
            e.set_warp(dict(kind=1, fill=FILL), **sets[4])
    got, gens = run(e, lambda i: e.submit(*clip[i], pts=i), N, depth=depth, before=before)
    e.close()
    assert gens == [1, 1, 1, 1, 2, 2, 2, 2]
    same(got, ref)


def test_the_callers_own_mesh_bilinear_then_off(E, clip):
    m = R.random_mesh(W, H, 11)
    want = [R.apply(0, FILL, m, y, uv) for y, uv in clip[:4]] + list(clip[4:])
    ref = plain_stream(E, W, H, want)
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    bad = m.copy()
    bad[0, 0, 1] = R.NODE_MIN - 1
    with pytest.raises(E.EncoderError):
        e.set_warp_mesh(dict(kind=0, fill=FILL), bad)
    with pytest.raises(E.EncoderError):
        e.set_warp(dict(kind=1), zoom=262144, kh=-32768)  # refused by the builder: nothing is set
    assert e.get_warp() is None
    e.set_warp_mesh(dict(kind=0, fill=FILL), m)
    got, gens = run(e, lambda i: e.submit(*clip[i], pts=i), N, before=lambda i: e.set_warp_mesh(None, None) if i == 4 else None)
    e.close()
    assert gens == [1] * 4 + [0] * 4
    same(got, ref)


def test_order_of_steps_with_sharpening_and_the_noise_filter(E, clip):
    """geometry first: the warped picture is what the noise filter and the picture controls see (and both planes are exchanged beside the controls' luma)"""
    kw = dict(adjust=dict(sharpen=24, brightness=40, saturation=1200), denoise=dict(luma=8, chroma=8))
    ref = plain_stream(E, W, H, warped(clip, [R.SETS["all"]] * N), **kw)
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=2, **kw)
    e.set_warp(dict(kind=1, fill=FILL), **R.SETS["all"])
    got, _ = run(e, lambda i: e.submit(*clip[i], pts=i), N)
    e.close()
    same(got, ref)


def test_hold_mode_warps_a_repeated_picture_once(E, clip):
    ns = 10 ** 9
    want = warped(clip[:2], [R.SETS["all"]] * 2)
    assert not np.array_equal(R.apply(1, FILL, R.build(W, H, **R.SETS["all"]), *want[0])[0], want[0][0])  # (warped twice it would be another picture)
    e = E.Encoder(W, H, fps=60, gop=GOP, fixed_qp=QP, pipeline_depth=2, rate=(rateref.HOLD, ns, 2))
    e.set_warp(dict(kind=1, fill=FILL), **R.SETS["all"])

    def source():
        return e.fetch(E.FETCH_SOURCE_Y)[:H, :W], e.fetch(E.FETCH_SOURCE_UV)[:H // 2, :W]
    assert e.submit(*clip[0], pts=0) == 1
    e.collect()
    assert all(np.array_equal(a, b) for a, b in zip(source(), want[0]))
    assert e.submit(*clip[1], pts=ns // 30) == 2  # the tick in between repeats the first picture
    e.collect()
    assert all(np.array_equal(a, b) for a, b in zip(source(), want[0]))
    e.collect()
    assert all(np.array_equal(a, b) for a, b in zip(source(), want[1]))
    e.close()


def test_submit_device_leaves_the_in_place_exit(E, clip):
    """160 x 96 on aligned planes would be coded where it lies: warped, it goes through the encoder's own surfaces and the caller's planes stay what they were"""
    ref = plain_stream(E, W, H, warped(clip, [R.SETS["roll"]] * N))
    dev = [(dev_put(y), dev_put(uv)) for y, uv in clip]
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    e.set_warp(dict(kind=1, fill=FILL), **R.SETS["roll"])
    got, gens = run(e, lambda i: e.submit_device(dev[i][0], W, dev[i][1], W, pts=i), N)
    e.close()
    assert gens == [1] * N
    for (dy, duv), (y, uv) in zip(dev, clip):
        assert np.array_equal(dev_get(dy, y.shape), y) and np.array_equal(dev_get(duv, uv.shape), uv)
    same(got, ref)


def test_timed_stage_needs_a_warp(E):
    e = E.Encoder(W, H, fixed_qp=QP)
    with pytest.raises(E.EncoderError):
        e.time_stage(E.STAGE_WARP, 2)
    e.set_warp(dict(kind=1), **R.SETS["barrel"])
    assert e.time_stage(E.STAGE_WARP, 2) > 0
    e.close()


def test_the_launch_alone_is_refused_with_pictures_in_flight(E, clip):
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    y, uv = coded_noise(W, H, 2)
    e.submit(*clip[0], pts=0)
    with pytest.raises(E.EncoderError) as err:
        e.stage_warp(dict(kind=1), R.identity(W, H), y, uv)
    assert "(%d)" % E.ERR_STATE in str(err.value)
    e.collect()
    gy, guv = e.stage_warp(dict(kind=1), R.identity(W, H), y, uv)
    assert np.array_equal(gy, y) and np.array_equal(guv, uv)  # (160 x 96 has no margin)
    e.close()
