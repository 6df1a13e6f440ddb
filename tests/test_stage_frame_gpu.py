"""GPU: the frame every single-stage entry point runs in, and the table mi355enc_time_stage runs from ("The stage entry points") --
behaviour as it is.  One handle of 72 x 80 (5 x 5 macroblocks: the visible width is not the surface width, two deblocking bands with a remainder row, partly
visible 8 x 8 blocks in x) at pipeline depth 2, beside it handles that carry the settings some stages need.  With a picture in flight every device stage is
refused with its own code and leaves no trace in the stream; the in-place stages give the same planes twice, those of the features' own numpy references; a
call's temporaries are its own and are gone after it; every timed stage runs, or answers ERR_STATE where the handle lacks what it needs."""
import ctypes as C

import numpy as np
import pytest

from tests import adjustref as A
from tests import denoisemcref as M
from tests import denoiseref as D
from tests import imageref as IM
from tests import overlayref as OV
from tests import rateref
from tests import stageframe as SF
from tests import yuvref as YR
from tests.inputref import device_free
from tests.test_adjust_gpu import FORMS, want
from tests.test_denoise_gpu import equal_or_none, noise16
from tests.test_scale_gpu import clip
from tests.test_yuv_convert_gpu import PAIRS, coef_of, dev_put, noise
from tests.util import pad_planes

pytestmark = pytest.mark.gpu

W, H, CW, CH = SF.W, SF.H, 80, 80
DEPTH, QP, GOP, NS = 2, 28, 8, 10 ** 9
PAIR = PAIRS["full601-lim709"]
IN_SIZE = (2 * W, 2 * H)
POINT, STENCIL = FORMS["both"], FORMS["16-thr8"]
NOT_READY = {14, 15, 17, 18, 19, 20, 21, 23, 24, 25, 26, 27, 28}  # the stages with a readiness condition, which a plain handle does not meet
# what the three still stages answer with a picture in flight: they never had a guard of their own -- they work in a block and temporaries of their own, on the
# main stream behind the picture -- and keep answering what their run answers
SNAPSHOT_IN_FLIGHT = 0


@pytest.fixture(scope="module", autouse=True)
def _torch_sees_the_device_first():
    """torch (whose mem_get_info the leak test reads) brings a HIP runtime of its own, which has to count the devices before the library's opens one -- what the
    suite's collection does anyway (tests/test_abi_cpu.py); this keeps the module runnable by itself"""
    import torch
    assert torch.cuda.is_available()


def plain(E):
    return E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=DEPTH)


def configured(E):
    """an input size, an input colorimetry, rate conversion in blend mode, an image on layer 0, picture controls, the noise filter with a range"""
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=DEPTH, colorimetry=PAIR[1], input_colorimetry=PAIR[0], input_size=IN_SIZE,
                  rate=(rateref.BLEND, NS, 2), adjust=POINT, denoise=dict(luma=8, chroma=8, motion=4))
    e.set_image(0, IM.to_fmt(IM.random_image(np.random.default_rng(4), 21, 13), E.FMT_RGBX), 6, 10, 200)
    return e


def hdr(E):
    """HDR input (it excludes an input colorimetry): the handle takes 10-bit pictures only"""
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=DEPTH, colorimetry=(0, 1, 1, 1), hdr_input=(E.HDR_PQ, 0, 1000, 100))
    e.p010 = True
    return e


def feed(E, e, i):
    """picture i (0, 1) of the handle's kind of input, submitted at the next tick"""
    e.fed = getattr(e, "fed", 0) + 1
    if getattr(e, "p010", False):
        return e.submit_fmt(E.FMT_P010, YR.random_planes(E.FMT_P010, W, H, np.random.default_rng(50 + i)), pts=e.fed * NS // 60)
    return e.submit(*clip(*e.input_size, 2)[i], pts=e.fed * NS // 60)


def two_pictures(E, e, idr_first=True):
    """two pictures through the pipeline, as the probes do: the contexts the timed stages run on are a real picture's.  idr_first: the handle is new, or a stage
    call has touched what the next picture would predict from -- an IDR and a P picture"""
    out = []
    for i in range(2):
        feed(E, e, i)
    while e.pending:
        out.append(e.collect())
    assert len(out) == 2 and (not idr_first or [k for _, k, _, _ in out] == [True, False])
    return out


@pytest.fixture(scope="module")
def handles(E):
    hs = {"plain": plain(E), "configured": configured(E), "hdr": hdr(E)}
    yield hs
    for e in hs.values():
        e.close()


@pytest.fixture(scope="module")
def table(E):
    buf = np.zeros(SF.BUF_BYTES, np.uint8)
    dev = dev_put(np.zeros(SF.DEV_BYTES, np.uint8))
    yield [(name, args) for name, args, device in SF.entries(E, buf, dev) if device], buf
    device_free(dev)


def _planes(seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (CH, CW), dtype=np.uint8), rng.integers(0, 256, (CH // 2, CW), dtype=np.uint8)


def _same(got, ref, what):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        equal_or_none(g, r, (what, k))


# ---- in flight
@pytest.mark.parametrize("make", [plain, configured], ids=["plain", "configured"])
def test_in_flight_every_device_stage_is_refused_and_leaves_no_trace(E, table, make):
    e, twin = make(E), make(E)
    streams = []
    for x in (e, twin):
        feed(E, x, 0)
        assert x.pending >= 1
        if x is e:
            codes = {name: getattr(e.L, name)(e.h, *args) for name, args in table[0]}
        out = [x.collect() for _ in range(x.pending)]
        feed(E, x, 1)  # ... and the stream goes on as if nothing had been asked
        while x.pending:
            out.append(x.collect())
        streams.append(out)
        x.close()
    expected = {name: E.ERR_STATE for name, _ in table[0]}
    expected["mi355enc_stage_csc"] = E.ERR_ARG
    expected.update({n: SNAPSHOT_IN_FLIGHT for n in expected if n.startswith("mi355enc_stage_snapshot")})
    print("in flight:", {n: c for n, c in codes.items() if c != E.ERR_STATE})
    assert codes == expected
    assert len(streams[0]) >= 2 and streams[0] == streams[1]


# ---- round trip: twice in a row on an idle handle, against the feature's own reference
def test_yuv_convert_twice(E, handles):
    e = handles["configured"]
    y, uv = noise(W, H, 5)
    ref = YR.convert(y, uv, coef_of(PAIR))
    for k in range(2):
        _same(e.stage_yuv_convert(y, uv), ref, ("yuv_convert", k))


@pytest.mark.parametrize("form", ["both", "16-thr8"])
def test_adjust_twice(E, handles, form):
    rng = np.random.default_rng(6)
    y, uv = A.with_margins(rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8), CW, CH)
    ref = want(E, y, uv, FORMS[form], visible=(W, H))
    for k in range(2):
        _same(handles["plain"].stage_adjust(FORMS[form], y, uv), ref, ("adjust", form, k))


def test_overlay_twice(E, handles):
    rng = np.random.default_rng(7)
    y, uv = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
    py, puv = pad_planes(y, uv)
    st = dict(halign=2, valign=2, xpad=0, ypad=0, scale=1, shaded_background=1)
    ref = OV.draw_coded(y, uv, "b: 2048 rtt: 40", **st)
    assert not np.array_equal(ref[0], py)
    for k in range(2):
        _same(handles["plain"].stage_overlay("b: 2048 rtt: 40", py, puv, **st), ref, ("overlay", k))


def test_image_twice(E, handles):
    rng = np.random.default_rng(8)
    y, uv = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
    py, puv = pad_planes(y, uv)
    pix = IM.random_image(rng, 37, 21)
    ref = IM.blend_coded(y, uv, [IM.layer(pix, W - 30, 5, 200)], IM.coefficients(2, 0, W, H))
    assert not np.array_equal(ref[0], py)
    for k in range(2):
        _same(handles["plain"].stage_image([E.image_layer(IM.to_fmt(pix, E.FMT_RGBX), W - 30, 5, 200, E.FMT_RGBX)], py, puv), ref, ("image", k))


def _histories(seed):
    rng = np.random.default_rng(seed)
    return noise16(rng, (CH, CW)), noise16(rng, (CH // 2, CW))


def test_denoise_twice(E, handles):
    (y, uv), (hy, huv) = _planes(9), _histories(10)
    ref = D.step(y, uv, hy, huv, 8, 8, visible=(W, H))
    for k in range(2):
        _same(handles["plain"].stage_denoise(dict(luma=8, chroma=8), y, uv, hy, huv), ref, ("denoise", k))


def test_denoise_mc_twice_with_temporaries_of_its_own(E, handles):
    (y, uv), (hy, huv) = _planes(11), _histories(12)
    ref = M.step(y, uv, hy, huv, 8, 8, 4, visible=(W, H), vectors=True)
    for name in ("plain", "configured"):
        e = handles[name]
        if name == "configured":
            two_pictures(E, e)  # the handle's own histories exist
            assert e.debug_denoise_bytes() > 0
        held = e.debug_denoise_bytes()
        for k in range(2):
            _same(e.stage_denoise_mc(dict(luma=8, chroma=8), 4, y, uv, hy, huv), ref, ("denoise_mc", name, k))
        assert e.debug_denoise_bytes() == held


def test_rate_twice(E, handles):
    (ay, auv), (by, buv) = _planes(13), _planes(14)
    ref = (rateref.mix(ay, by, 85), rateref.mix(auv, buv, 85))
    for k in range(2):
        _same(handles["plain"].stage_rate(85, ay, auv, by, buv), ref, ("rate", k))


def test_the_temporaries_of_a_call_are_gone_after_it(E, handles):
    """20 calls each of the two stages that allocate for themselves: the device's free memory stays where the first call left it, within one allocation granule.
    The granule: 2 MiB, the unit the driver hands device memory to the runtime in.  The parent commit's run of this test could not show a smaller one: its free
    figure did not move at all over the 20 call pairs (every difference 0, as on this commit).  What the calls allocate at this size is about 60 KiB per pair
    (five buffers for stage_denoise_mc, one for stage_orient), which the runtime serves out of granules it already holds -- so the figure moves only when a
    granule is taken or given back, and the bound allows one such step either way."""
    import torch
    granule = 2 << 20
    e = handles["plain"]
    (y, uv), (hy, huv) = _planes(15), _histories(16)
    rng = np.random.default_rng(17)
    oy, ouv = rng.integers(0, 256, (W, 96), dtype=np.uint8)[:, :H], rng.integers(0, 256, (W // 2, 96), dtype=np.uint8)[:, :H]  # 90r: the source is 80 x 72
    torch.cuda.mem_get_info()
    free = []
    for k in range(20):
        e.stage_denoise_mc(dict(luma=8, chroma=8), 4, y, uv, hy, huv)
        e.stage_orient(E.ORIENT_90R, oy, ouv)
        free.append(torch.cuda.mem_get_info()[0])
    print("free after each call pair, relative to the first:", [f - free[0] for f in free])
    assert all(abs(f - free[0]) <= granule for f in free)


# ---- timed stages
def _timed(E, e, stage):
    ms = C.c_double(-1)
    return e.L.mi355enc_time_stage(e.h, stage, 2, C.byref(ms)), ms.value


def test_timed_stages_on_a_plain_handle(E, handles):
    e = handles["plain"]
    two_pictures(E, e)
    got = {s: _timed(E, e, s) for s in range(29)}
    print("plain:", got)
    assert {s for s, (r, _) in got.items() if r == E.ERR_STATE} == NOT_READY
    assert all(r == 0 and ms > 0 for s, (r, ms) in got.items() if s not in NOT_READY)
    two_pictures(E, e)  # the handle is a working encoder behind them


def test_timed_stages_on_configured_handles(E, handles):
    e, eh = handles["configured"], handles["hdr"]
    two_pictures(E, e, idr_first=False)  # (the round trips above may have run on it)
    two_pictures(E, eh)
    got = {}
    for s in range(29):
        if s == E.STAGE_ADJUST_SHARPEN:
            e.set_adjust(STENCIL)
        got[s] = _timed(E, eh if E.STAGE_HDR_P010 <= s <= E.STAGE_HDR_V210 else e, s)
        if s == E.STAGE_ADJUST_SHARPEN:
            e.set_adjust(POINT)
    print("configured:", got)
    assert all(r == 0 and ms > 0 for r, ms in got.values()), got
    assert _timed(E, eh, E.STAGE_DEEP_P010)[1] > 0
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):  # (no HDR input on this one)
        e.time_stage(E.STAGE_HDR_P010, 1)
    two_pictures(E, e)
    two_pictures(E, eh)
