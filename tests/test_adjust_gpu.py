"""GPU: picture controls on the way in -- colour balance, gamma and sharpening of the coded surfaces -- bit for bit against
tests/adjustref.py applied with the tables mi355enc_adjust_tables returned: the step alone in both forms at the smallest sizes at which each thing can go wrong,
under a letterbox geometry and an orientation, inside streams (latched per input picture, reported at collect, equal to the stream of the pre-adjusted
pictures), off, under frame-rate conversion, and from device planes."""
import numpy as np
import pytest

from tests import adjustref as A
from tests import rateref
from tests import yuvref as R
from tests.inputref import device_free
from tests.test_csc_formats_gpu import drain, same
from tests.test_yuv_convert_gpu import dev_get, dev_put

pytestmark = pytest.mark.gpu

# 16 x 16: every sample is an edge; 64 x 48: no margins; 72 x 40: margins right and bottom (coded 80 x 48); 200 x 72: several tiles both ways, edges off any tile multiple
SIZES = [(16, 16), (64, 48), (72, 40), (200, 72)]
POINTWISE = {"luma": dict(brightness=120, contrast=1400, gamma=1800), "chroma": dict(saturation=1600, hue=-230),
             "both": dict(brightness=-150, contrast=1900, saturation=1900, hue=410)}
STENCIL = {"%d-thr%d" % (s, t): dict(sharpen=s, sharpen_threshold=t, **extra)
           for s, extra in ((-16, {}), (16, dict(contrast=1250, brightness=-40)), (64, dict(saturation=700, hue=90))) for t in (0, 8)}
FORMS = dict(POINTWISE, **STENCIL)
QP, GOP = 28, 4


def coded(w, h):
    return (w + 15) // 16 * 16, (h + 15) // 16 * 16


def pictures(w, h, seed):
    """two pictures as the step finds them -- coded surfaces, margins replicas of the last visible row and column: noise, and one of samples 0 and 255 only"""
    rng = np.random.default_rng(seed)
    W, H = coded(w, h)
    noise = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8))
    sat = (rng.choice(np.array([0, 255], np.uint8), (h, w)), rng.choice(np.array([0, 255], np.uint8), (h // 2, w)))
    return [A.with_margins(y, uv, W, H) for y, uv in (noise, sat)]


def want(E, y, uv, a, full=0, rect=None, visible=None):
    a = A.params(**a)
    luma, chroma = E.adjust_tables(a, full)
    return A.apply(y, uv, a, luma, chroma, rect, visible)


def margins_are_replicas(y, uv, w, h):
    H, W = y.shape
    ry, ruv = A.with_margins(y[:h, :w], uv[:h // 2, :w], W, H)
    return np.array_equal(y, ry) and np.array_equal(uv, ruv)


# ---- the step alone
@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("form", list(FORMS))
def test_stage_adjust_matches_numpy(E, form, w, h):
    e = E.Encoder(w, h, fixed_qp=30)
    for k, (y, uv) in enumerate(pictures(w, h, 100 * w + len(form))):
        got = e.stage_adjust(FORMS[form], y, uv)
        ref = want(E, y, uv, FORMS[form], visible=(w, h))
        same(got, ref)
        assert margins_are_replicas(got[0], got[1], w, h)
        if k == 0:  # on noise every plane the form names moves, and only those (the saturated picture is there for the clips: sharpening leaves 0 and 255 where they are)
            assert np.array_equal(got[0], y) == (form == "chroma") and np.array_equal(got[1], uv) == (form == "luma" or form.startswith(("-16", "16")))
    assert e.debug_adjust_bytes() == (coded(w, h)[0] * coded(w, h)[1] if form in STENCIL else 0)
    e.close()


def test_full_range_uses_its_own_black_and_scale(E):
    w, h = 72, 40
    e = E.Encoder(w, h, fixed_qp=30, colorimetry=(1, 1, 1, 1))
    a = dict(contrast=1500, brightness=50, sharpen=16)
    y, uv = pictures(w, h, 5)[0]
    got = e.stage_adjust(a, y, uv)
    same(got, want(E, y, uv, a, full=1, visible=(w, h)))
    assert not np.array_equal(got[0], want(E, y, uv, a, full=0, visible=(w, h))[0])
    e.close()


def test_stage_adjust_neutral_and_refused_values(E):
    e = E.Encoder(64, 48, fixed_qp=30)
    y, uv = pictures(64, 48, 6)[0]
    same(e.stage_adjust({}, y, uv), (y, uv))
    assert e.debug_adjust_bytes() == 0
    for bad in (dict(gamma=99), dict(sharpen=65), dict(sharpen_threshold=33), dict(hue=-1001)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.stage_adjust(bad, y, uv)
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.set_adjust(bad)
    assert e.get_adjust() == A.NEUTRAL
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.last_adjust()
    e.close()


# ---- letterbox
@pytest.mark.parametrize("method,dst", [(0, (20, 12, 88, 72)), (1, (10, 22, 72, 88))], ids=["none", "90r"])
@pytest.mark.parametrize("form", ["both", "16-thr0", "-16-thr8"])
def test_under_a_letterbox_the_border_keeps_its_bytes(E, form, method, dst):
    w, h = 128, 96
    e = E.Encoder(w, h, fixed_qp=30, orientation=method or None, geometry=E.geometry((160, 96), dst=dst))
    mask = R.picture_mask(w, h, dst, method)
    ys, xs = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
    rect = (int(xs[0]), int(xs[-1]) + 1, int(ys[0]), int(ys[-1]) + 1)
    assert mask[rect[2]:rect[3], rect[0]:rect[1]].all() and mask.sum() == dst[2] * dst[3] and 0 < rect[0] and rect[1] < w and 0 < rect[2] and rect[3] < h
    y, uv = pictures(w, h, 7 + method)[0]
    got = e.stage_adjust(FORMS[form], y, uv)
    same(got, want(E, y, uv, FORMS[form], rect=rect, visible=(w, h)))  # (the reference clamps the 3 x 3 at the rectangle's edge: the border's noise is never read)
    assert np.array_equal(got[0][~mask], y[~mask]) and not np.array_equal(got[0][mask], y[mask])
    cmask = mask[0::2]
    assert np.array_equal(got[1][~cmask], uv[~cmask])
    e.close()


@pytest.mark.parametrize("form", ["both", "16-thr0"])
def test_a_letterbox_that_reaches_the_visible_edge_takes_the_margin_with_it(E, form):
    """72 x 40 in coded 80 x 48, the destination rectangle up to the right and bottom edge of the visible picture: the margin there is picture (replicas of the
    adjusted last row and column), the border left and above keeps its bytes"""
    w, h, dst = 72, 40, (10, 6, 62, 34)
    e = E.Encoder(w, h, fixed_qp=30, geometry=E.geometry((160, 96), dst=dst))
    mask = R.picture_mask(w, h, dst, 0)
    assert mask[6:, 10:].all() and not mask[:6].any() and not mask[:, :10].any()
    y, uv = pictures(w, h, 9)[0]
    got = e.stage_adjust(FORMS[form], y, uv)
    same(got, want(E, y, uv, FORMS[form], rect=(10, 80, 6, 48), visible=(w, h)))
    assert margins_are_replicas(got[0], got[1], w, h) and np.array_equal(got[0][~mask], y[~mask]) and not np.array_equal(got[0][mask], y[mask])
    e.close()


# ---- streams
def clip(w, h, n, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h + 2 * n, w + 2 * n), dtype=np.uint8)
    cbase = rng.integers(64, 192, (h // 2 + n, w + 2 * n), dtype=np.uint8)
    return [(np.ascontiguousarray(base[2 * i:2 * i + h, 2 * i:2 * i + w]), np.ascontiguousarray(cbase[i:i + h // 2, 2 * i:2 * i + w])) for i in range(n)]


def adjusted(E, pic, a, w, h):
    """what the source surfaces hold of a submitted visible picture under a"""
    W, H = coded(w, h)
    return want(E, *A.with_margins(pic[0], pic[1], W, H), a, visible=(w, h))


def test_a_stream_latches_per_picture_and_equals_the_stream_of_the_adjusted_pictures(E):
    w, h, depth = 64, 48, 2
    pics = clip(w, h, 3, 11)
    values = [dict(brightness=100, sharpen=16), dict(saturation=800, hue=100), dict(contrast=1200, gamma=1500, sharpen=-16, saturation=1300)]
    a = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, adjust=values[0])
    assert a.get_adjust() == A.params(**values[0])
    for i in range(3):
        a.set_adjust(values[i])
        a.submit(*pics[i], pts=i)
    a.set_adjust()  # (after the last submit: no picture carries it)
    got = []
    for i in range(3):
        got.append(a.collect()[:2])
        same((a.fetch(E.FETCH_SOURCE_Y), a.fetch(E.FETCH_SOURCE_UV)), adjusted(E, pics[i], values[i], w, h))
        assert a.last_adjust() == A.params(**values[i])
    assert a.debug_adjust_bytes() == 64 * 48 and a.get_adjust() == A.NEUTRAL
    b = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    pre = [adjusted(E, pics[i], values[i], w, h) for i in range(3)]
    ref = drain(b, depth, lambda i: b.submit(pre[i][0][:h, :w], pre[i][1][:h // 2, :w], pts=i), 3)
    assert got == ref and b.debug_adjust_bytes() == 0 and b.last_adjust() == A.NEUTRAL
    a.close(); b.close()


def test_off_is_off(E):
    w, h, depth = 64, 48, 2
    pics = clip(w, h, 3, 12)
    never = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    neutral = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, adjust=dict(A.NEUTRAL, sharpen_threshold=8))  # (the threshold alone does nothing)
    neutral.set_adjust(**A.NEUTRAL)
    ref = drain(never, depth, lambda i: never.submit(*pics[i], pts=i), 3)
    assert drain(neutral, depth, lambda i: neutral.submit(*pics[i], pts=i), 3) == ref
    assert never.debug_adjust_bytes() == 0 and neutral.debug_adjust_bytes() == 0
    point = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, adjust=POINTWISE["both"])
    assert drain(point, depth, lambda i: point.submit(*pics[i], pts=i), 3) != ref
    assert point.debug_adjust_bytes() == 0
    point.set_adjust(sharpen=16)
    point.submit(*pics[0], pts=3)
    point.collect()
    assert point.debug_adjust_bytes() == 64 * 48
    never.close(); neutral.close(); point.close()


def test_hold_mode_adjusts_a_repeated_picture_once(E):
    w, h, ns = 64, 48, 10 ** 9
    pics = clip(w, h, 2, 13)
    a = dict(brightness=80, contrast=1300, sharpen=32, saturation=1500)  # (applied twice it would give another picture)
    e = E.Encoder(w, h, fps=60, gop=GOP, fixed_qp=QP, pipeline_depth=2, rate=(rateref.HOLD, ns, 2), adjust=a)
    assert e.submit(*pics[0], pts=0) == 1
    e.collect()
    first = (e.fetch(E.FETCH_SOURCE_Y), e.fetch(E.FETCH_SOURCE_UV))
    same(first, adjusted(E, pics[0], a, w, h))
    assert not np.array_equal(want(E, *first, a, visible=(w, h))[0], first[0])
    assert e.submit(*pics[1], pts=ns // 30) == 2  # the tick in between repeats the first picture
    e.collect()
    same((e.fetch(E.FETCH_SOURCE_Y), e.fetch(E.FETCH_SOURCE_UV)), first)
    e.collect()
    same((e.fetch(E.FETCH_SOURCE_Y), e.fetch(E.FETCH_SOURCE_UV)), adjusted(E, pics[1], a, w, h))
    assert e.rate_stats()["repeated"] == 1
    e.close()


@pytest.mark.parametrize("form", ["both", "16-thr0"])
def test_submit_device_never_adjusts_the_callers_planes(E, form):
    """64 x 48 on aligned planes would take the in-place exit: with an adjustment it must not, and the planes stay what they were"""
    w, h, depth = 64, 48, 2
    pics = clip(w, h, 3, 14)
    dev = [(dev_put(y), dev_put(uv)) for y, uv in pics]
    a = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, adjust=FORMS[form])
    b = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    got = drain(a, depth, lambda i: a.submit_device(dev[i][0], w, dev[i][1], w, pts=i), 3)
    pre = [adjusted(E, p, FORMS[form], w, h) for p in pics]
    assert got == drain(b, depth, lambda i: b.submit(pre[i][0][:h, :w], pre[i][1][:h // 2, :w], pts=i), 3)
    for (dy, duv), (y, uv) in zip(dev, pics):
        assert np.array_equal(dev_get(dy, y.shape), y) and np.array_equal(dev_get(duv, uv.shape), uv)
    a.close(); b.close()
    for dy, duv in dev:
        device_free(dy); device_free(duv)
