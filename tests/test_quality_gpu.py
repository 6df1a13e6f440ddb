"""GPU: per-picture quality metrics computed on the device (k_quality.hip) against the numpy restatement of the rule
(tests/qualityref.py).  Every comparison is == on the five integers: the squared errors of Y, Cb, Cr, the fixed-point SSIM sum and the window
count.  The kernel alone on host and on device planes (margins filled with noise, unaligned addresses and strides), then inside the picture
pipeline in every schedule, where the reference reconstruction comes from a second encoder of the same configuration at pipeline_depth 0
through fetch(RECON_*) -- the streams are deterministic and equal, which is asserted on the access units."""
import functools

import numpy as np
import pytest

from ceracoder_amd import enc as E
from ceracoder_amd import synth
from tests import inputref as IR
from tests import qualityref as Q

pytestmark = pytest.mark.gpu

W0, H0, QP = 128, 96, 28


@pytest.fixture(scope="module", autouse=True)
def _torch_sees_the_device_first():
    """torch (the allocator of the device-plane tests) brings a HIP runtime of its own, which has to count the devices before the library's opens one
    -- what the suite's collection does anyway (tests/test_abi_cpu.py); this keeps the module runnable by itself"""
    import torch
    assert torch.cuda.is_available()


def _coded(n):
    return (n + 15) // 16 * 16


def _with_margin(y, uv, w, h, seed):
    """the visible w x h picture inside coded-size surfaces whose margin is seeded noise"""
    W, H = _coded(w), _coded(h)
    rng = np.random.default_rng(seed)
    oy, ouv = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
    oy[:h, :w] = y[:h, :w]
    ouv[:h // 2, :w] = uv[:h // 2, :w]
    return oy, ouv


def _pairs(w, h):
    """(name, source planes, reconstruction planes), visible size"""
    rng = np.random.default_rng(w * 1000 + h)
    rnd = lambda: (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8))
    a, b = rnd(), rnd()
    z, f = (np.zeros((h, w), np.uint8), np.zeros((h // 2, w), np.uint8)), (np.full((h, w), 255, np.uint8), np.full((h // 2, w), 255, np.uint8))
    y, uv = next(iter(synth.s2_frames(w, h, 1)))
    e = E.Encoder(w, h, fixed_qp=30)
    e.encode(y, uv)
    rec = (e.fetch(E.FETCH_RECON_Y), e.fetch(E.FETCH_RECON_UV))
    e.close()
    return [("identical", a, a), ("random", a, b), ("0 against 255", z, f), ("encode at QP 30", (y, uv), rec)]


@pytest.mark.parametrize("w,h", [(16, 16), (50, 38), (176, 144), (322, 242)])
def test_stage_on_host_planes_equals_the_restatement(w, h):
    """one macroblock (3 x 3 windows); neither a multiple of 4 nor of 16 (the left-out remainder, the margin); more than one tile in both directions"""
    pairs = _pairs(w, h)
    e = E.Encoder(w, h, fixed_qp=30)
    for k, (name, s, r) in enumerate(pairs):
        sy, suv = _with_margin(s[0], s[1], w, h, 10 + k)
        ry, ruv = _with_margin(r[0], r[1], w, h, 20 + k)
        want = Q.quality(sy, suv, ry, ruv, w, h)
        q = e.stage_quality(sy, suv, ry, ruv)
        assert q.ints() == want, name
        assert want[4] == (w // 4 - 1) * (h // 4 - 1)
        assert list(q.samples) == [w * h, (w // 2) * (h // 2), (w // 2) * (h // 2)]
        d = Q.derived(want, w, h)
        assert np.allclose(list(q.psnr) + [q.ssim], d, rtol=1e-12, atol=0), name
        if name == "identical":
            assert want[:4] == (0, 0, 0, want[4] << 30) and q.ssim == 1.0 and list(q.psnr) == [100.0] * 3
    e.close()


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h", [(50, 38), (176, 144)])
def test_stage_on_device_planes_at_any_address_and_stride(w, h, offset):
    """the source 0 .. 3 bytes into an aligned allocation, at strides that are and are not multiples of four: the dword path and the byte-wise
    path give the same integers.  The source buffers end with the last visible sample."""
    import torch
    rng = np.random.default_rng(w + offset)
    sy, suv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    ry = np.clip(sy.astype(np.int64) + rng.integers(-9, 10, (h, w)), 0, 255).astype(np.uint8)
    ruv = np.clip(suv.astype(np.int64) + rng.integers(-5, 6, (h // 2, w)), 0, 255).astype(np.uint8)
    ry, ruv = _with_margin(ry, ruv, w, h, 3)
    want = Q.quality(sy, suv, ry, ruv, w, h)
    e = E.Encoder(w, h, fixed_qp=30)
    dry, druv = torch.from_numpy(ry).cuda(), torch.from_numpy(ruv).cuda()
    w4 = (w + 3) // 4 * 4
    for stride in (w4, w4 + 8, w, w4 + 1, w4 + 3):
        keep = []
        for p in (sy, suv):
            host = rng.integers(0, 256, offset + stride * (p.shape[0] - 1) + w, dtype=np.uint8)
            IR.visible(host, offset, p.shape[0], w, stride)[:] = p
            keep.append(torch.from_numpy(host).cuda())
        torch.cuda.synchronize()
        q = e.stage_quality_device(keep[0].data_ptr() + offset, keep[1].data_ptr() + offset, stride, dry.data_ptr(), druv.data_ptr())
        assert q.ints() == want, stride
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        e.stage_quality_device(keep[0].data_ptr(), keep[1].data_ptr(), w - 2, dry.data_ptr(), druv.data_ptr())
    e.close()


# ---- the picture pipeline
def _take(e, metrics, fetch):
    au, key, pts, qp = e.collect()
    q = e.last_quality() if metrics else None
    if q is not None:
        assert q.pts == pts
    rec = (e.fetch(E.FETCH_RECON_Y), e.fetch(E.FETCH_RECON_UV)) if fetch else None
    return au, key, pts, q, rec


def _drive(e, n, depth, submit, metrics, before=None):
    got = []
    for i in range(n):
        if before:
            before(e, i)
        submit(e, i)
        if e.pending > depth:
            got.append(_take(e, metrics, depth == 0 and not metrics))
    while e.pending:
        got.append(_take(e, metrics, depth == 0 and not metrics))
    return got


def _check(got, ref, sources, w, h):
    """access units equal; every picture's metrics equal the restatement on (its source, the reference encoder's reconstruction of it)"""
    assert [g[2] for g in got] == [r[2] for r in ref] == list(range(len(ref)))
    assert [g[0] for g in got] == [r[0] for r in ref]
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[3].ints() == Q.quality(sources[i][0], sources[i][1], r[4][0], r[4][1], w, h), i


@functools.lru_cache(maxsize=None)
def _clip(w=W0, h=H0, n=12):
    return list(synth.s2_frames(w, h, n))


@functools.lru_cache(maxsize=None)
def _plain_reference():
    """metrics off, depth 0: the access units and reconstructions every schedule of the plain stream has to reproduce"""
    clip = _clip()
    e = E.Encoder(W0, H0, gop=60, fixed_qp=QP)
    ref = _drive(e, len(clip), 0, lambda e, i: e.submit(clip[i][0], clip[i][1], pts=i), False)
    e.close()
    return ref


@pytest.mark.parametrize("depth,kw", [(0, {}), (1, {}), (2, {}), (2, {"exclusive": True}), (2, {"single_stream": True})],
                         ids=["depth0", "depth1", "depth2", "depth2-exclusive", "depth2-single-stream"])
def test_stream_metrics_equal_the_restatement_in_every_schedule(depth, kw):
    """keep_prefilter 0.  At depth 2 the fused P stage of picture n + 2 writes the buffer picture n's metrics read: a launch in the wrong place
    reads an overwritten reconstruction and fails here on the integers."""
    clip = _clip()
    e = E.Encoder(W0, H0, gop=60, fixed_qp=QP, pipeline_depth=depth, keep_prefilter=False, **kw)
    e.set_quality_metrics(True)
    got = _drive(e, len(clip), depth, lambda e, i: e.submit(clip[i][0], clip[i][1], pts=i), True)
    e.close()
    _check(got, _plain_reference(), clip, W0, H0)
    assert any(g[3].sse[0] for g in got) and all(0 < g[3].ssim < 1 for g in got)


def _both(mk, n, submit, sources, w, h, depth=2, before=None):
    """the same stream from a depth-0 encoder without metrics and from one with them at `depth`"""
    r = mk(0)
    ref = _drive(r, n, 0, submit, False, before)
    r.close()
    e = mk(depth)
    e.set_quality_metrics(True)
    got = _drive(e, n, depth, submit, True, before)
    e.close()
    _check(got, ref, sources, w, h)
    return got, ref


def test_adaptive_quantisation_with_the_8x8_transform():
    clip = _clip(n=8)
    _both(lambda d: E.Encoder(W0, H0, gop=60, fixed_qp=QP, pipeline_depth=d, aq=True, transform8x8=1), 8,
          lambda e, i: e.submit(clip[i][0], clip[i][1], pts=i), clip, W0, H0)


def test_intra_refresh():
    clip = _clip(n=8)
    _both(lambda d: E.Encoder(W0, H0, gop=8, fixed_qp=QP, pipeline_depth=d, intra_refresh=True), 8,
          lambda e, i: e.submit(clip[i][0], clip[i][1], pts=i), clip, W0, H0)


def test_all_skip_pictures_are_measured_against_the_reference_they_repeat():
    clip = _clip(n=8)
    got, ref = _both(lambda d: E.Encoder(W0, H0, gop=60, fixed_qp=QP, pipeline_depth=d), 8,
                     lambda e, i: e.submit(clip[i][0], clip[i][1], pts=i), clip, W0, H0,
                     before=lambda e, i: e.set_fixed_drop(E.DROP_SKIP) if i == 5 else None)
    assert all(len(g[0]) < 40 for g in got[5:])  # one run of P_Skip macroblocks each
    assert all(np.array_equal(r[4][0], ref[4][4][0]) for r in ref[5:])
    assert got[5][3].sse[0] != got[6][3].sse[0]  # ... against sources that move on


def test_visible_size_that_is_no_multiple_of_16_goes_through_the_padding():
    w, h = 130, 98
    clip = _clip(w, h, 6)
    _both(lambda d: E.Encoder(w, h, gop=60, fixed_qp=QP, pipeline_depth=d), 6, lambda e, i: e.submit(clip[i][0], clip[i][1], pts=i), clip, w, h)


def test_submit_device_in_place_from_a_strided_container():
    """the kernels (this one too) read the caller's planes where they lie, at the caller's stride; everything around the visible samples is poison"""
    w, h, stride = 128, 90, 192
    clip = _clip(w, h, 6)
    cont = [IR.container(y, uv, stride, seed=40 + i) for i, (y, uv) in enumerate(clip)]
    dev = [IR.device_container(c[0]) for c in cont]
    try:
        assert all((d + c[1]) % 16 == 0 and (d + c[2]) % 16 == 0 for d, c in zip(dev, cont))  # the in-place branch of submit_device
        _both(lambda d: E.Encoder(w, h, gop=60, fixed_qp=QP, pipeline_depth=d), 6,
              lambda e, i: e.submit_device(dev[i] + cont[i][1], stride, dev[i] + cont[i][2], stride, pts=i), clip, w, h)
    finally:
        for d in dev:
            IR.device_free(d)


def test_converted_input_is_measured_as_converted():
    rng = np.random.default_rng(9)
    clip = _clip(n=6)
    planes = [[y, np.ascontiguousarray(uv[:, 0::2]), np.ascontiguousarray(uv[:, 1::2])] for y, uv in clip]
    planes[3][1] = rng.integers(0, 256, planes[3][1].shape, dtype=np.uint8)
    s = E.Encoder(W0, H0, fixed_qp=QP)
    sources = [s.stage_csc(E.FMT_I420, p) for p in planes]
    s.close()
    _both(lambda d: E.Encoder(W0, H0, gop=60, fixed_qp=QP, pipeline_depth=d), 6, lambda e, i: e.submit_fmt(E.FMT_I420, planes[i], pts=i), sources, W0, H0)


def test_scaled_input_is_measured_as_scaled():
    big = _clip(256, 192, 6)
    s = E.Encoder(W0, H0, fixed_qp=QP, input_size=(256, 192))
    sources = [s.stage_scale(E.FMT_NV12, [y, uv]) for y, uv in big]
    s.close()
    _both(lambda d: E.Encoder(W0, H0, gop=60, fixed_qp=QP, pipeline_depth=d, input_size=(256, 192)), 6,
          lambda e, i: e.submit(big[i][0], big[i][1], pts=i), sources, W0, H0)


def test_pictures_that_come_back_through_a_recovery_report_the_re_encode():
    """mi355enc_debug_trip_wait as tests/test_recovery_gpu.py uses it, once: the pictures in flight are coded again from an IDR picture, in stream
    order; a depth-0 encoder forced to an IDR picture there reproduces them, and the metrics are those of that reconstruction."""
    clip = _clip()
    r = E.Encoder(W0, H0, gop=60, fixed_qp=QP)
    ref = _drive(r, len(clip), 0, lambda e, i: e.submit(clip[i][0], clip[i][1], pts=i, force_idr=i == 5), False)
    r.close()
    e = E.Encoder(W0, H0, gop=60, fixed_qp=QP, pipeline_depth=2, exclusive=True)
    e.set_quality_metrics(True)
    got = _drive(e, len(clip), 2, lambda e, i: e.submit(clip[i][0], clip[i][1], pts=i), True, before=lambda e, i: e.debug_trip_wait(12) if i == 5 else None)
    st = e.stats()
    e.close()
    assert st.recoveries == 1 and st.safe_level == 1 and [i for i, g in enumerate(got) if g[1]] == [0, 5]
    _check(got, ref, clip, W0, H0)


def test_totals_and_call_order():
    clip = _clip(n=6)
    e = E.Encoder(W0, H0, gop=60, fixed_qp=QP, pipeline_depth=1)
    for call in (e.last_quality, e.quality_totals):  # metrics off
        with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_STATE):
            call()
    e.set_quality_metrics(True)
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_STATE):  # nothing collected
        e.last_quality()
    assert e.quality_totals().pictures == 0
    got = _drive(e, 4, 1, lambda e, i: e.submit(clip[i][0], clip[i][1], pts=i), True)
    with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_STATE):  # after the first submit
        e.set_quality_metrics(False)
    t = e.quality_totals()
    sums = tuple(sum(g[3].ints()[k] for g in got) for k in range(5))
    assert t.ints() == sums and t.pictures == 4 and t.pts == 3
    assert list(t.samples) == [4 * W0 * H0, W0 * H0, W0 * H0]
    assert np.allclose(list(t.psnr) + [t.ssim], Q.derived(sums, W0, H0, pictures=4), rtol=1e-12, atol=0)
    e.reset_stats()
    t = e.quality_totals()
    assert t.ints() == (0, 0, 0, 0, 0) and t.pictures == 0
    more = _drive(e, 2, 1, lambda e, i: e.submit(clip[4 + i][0], clip[4 + i][1], pts=4 + i), True)
    assert e.quality_totals().ints() == tuple(sum(g[3].ints()[k] for g in more) for k in range(5))
    assert e.last_quality().ints() == more[-1][3].ints()
    e.close()
