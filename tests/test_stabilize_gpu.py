"""GPU: electronic image stabilisation (mi355enc_set_stabilize, k_stab.hip, the displaced geometry launch of k_scale.hip) -- the two
launches alone bit-exact against tests/stabref.py, and streams: the stabilising encoder's access units equal, byte for byte, those of a plain encoder fed
stabref's pictures (geomref's tables with displaced indices), and every picture's record equals the reference's."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import geomref as G
from tests import orientref
from tests import stabref as S
from tests.test_geometry_gpu import _device_container, plain_stream, same

pytestmark = pytest.mark.gpu

GOP, QP = 30, 28
IN = (160, 96)
SET = (8, 16, 16, 16)  # range, leak, margins
CROP = (16, 16, 128, 64)
JPEG = os.path.join(os.path.dirname(__file__), "golden", "jpeg", "q50_420_72x40.jpg")


@pytest.fixture(scope="module")
def probe(E):
    e = E.Encoder(64, 48, fixed_qp=QP)
    yield e
    e.close()


# ---- the launches alone
def _noise_view(h, w, step, first, pad, offset, seed):
    row = first + (w - 1) * step + 1 + pad
    buf = np.random.default_rng(seed).integers(0, 256, offset + row * h + 8, dtype=np.uint8)
    return np.lib.stride_tricks.as_strided(buf[offset + first:], (h, w), (row, step))


@pytest.mark.parametrize("shape", [(64, 48), (70, 50), (1100, 36), (36, 1100)], ids=lambda s: "%dx%d" % s)
def test_probe_project_is_bit_exact(probe, shape):
    w, h = shape
    # plain; an odd base offset and a stride of width + 3; every second byte from byte 0 / 1 (YUY2 / UYVY), at base offsets 0 .. 3
    for k, (step, first, pad, offset) in enumerate([(1, 0, 0, 0), (1, 0, 3, 1), (1, 0, 1, 2), (1, 0, 2, 3), (2, 0, 1, 0), (2, 1, 0, 0), (2, 0, 3, 1), (2, 1, 2, 2), (2, 1, 1, 3)]):
        luma = _noise_view(h, w, step, first, pad, offset, 100 * w + k)
        c, r = probe.stabilize_probe_project(luma)
        rc, rr = S.project(luma)
        assert np.array_equal(c, rc), (k, np.argwhere(c != rc)[:4])
        assert np.array_equal(r, rr), (k, np.argwhere(r != rr)[:4])


def test_probe_project_saturated_checkerboard_at_the_width_limit(probe):
    luma = (((np.arange(16)[:, None] + np.arange(8192)[None, :]) & 1) * 255).astype(np.uint8)
    c, r = probe.stabilize_probe_project(luma)
    rc, rr = S.project(luma)
    assert np.array_equal(c, rc) and np.array_equal(r, rr) and int(r.max()) == 1024 * 255


CASES = S.match_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_probe_match_is_bit_exact(E, probe, case):
    name, prev, cur, rng, leak, bnd, state = case
    want = S.match(prev, cur, rng, leak, bnd, state)
    assert (want["mx"], want["my"], want["votes_x"], want["votes_y"]) == S.EXPECT[name]
    st = E.stabilize(range=rng, leak=leak, margin=16)
    assert probe.stabilize_probe_match(prev, cur, st, bnd, state) == want
    assert probe.stabilize_probe_match(prev, cur, st, bnd, state, prime=True) == dict.fromkeys(S.KEYS, 0)


# ---- streams
def run(e, feed, n, depth=2, before=None):
    """-> ((access units, reconstruction), the pictures' records)"""
    out, recs = [], []
    for i in range(n):
        if before:
            before(i)
        feed(i)
        if e.pending > depth:
            out.append(e.collect())
            recs.append(e.last_stabilize()[1])
    while e.pending:
        out.append(e.collect())
        recs.append(e.last_stabilize()[1])
    return (out, (e.fetch(0), e.fetch(1))), recs


@pytest.fixture(scope="module")
def clip():
    return S.clip(*IN)


def planes_in(fmt, pic):
    y, uv = pic
    u, v = uv[:, 0::2], uv[:, 1::2]
    if fmt == G.FMT_NV12:
        return [y, uv]
    if fmt == G.FMT_I420:
        return [y, np.ascontiguousarray(u), np.ascontiguousarray(v)]
    p = np.empty((y.shape[0], 2 * y.shape[1]), np.uint8)  # 4:2:2: every chroma row twice
    yo, uo, vo = (0, 1, 3) if fmt == G.FMT_YUY2 else (1, 0, 2)
    p[:, yo::2], p[:, uo::4], p[:, vo::4] = y, np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0)
    return [p]


def conditions(recs, script=S.SCRIPT, on_bound=True):
    """on the reference, so that no stream test passes vacuously"""
    assert recs[0] == dict.fromkeys(S.KEYS, 0)
    for r, m in zip(recs[1:], script[1:]):
        assert r["votes_x"] >= 3 and r["votes_y"] >= 3 and (r["mx"], r["my"]) == m, (r, m)
    if on_bound:
        for k in ("ox", "oy"):
            vals = {r[k] for r in recs}
            assert len(vals) >= 5 and min(vals) < 0 < max(vals), vals
        assert any(abs(r["ox"]) == 16 or abs(r["oy"]) == 16 for r in recs)


def reference(fmt, planes, crops, dst, target, moved_too=False, setting=SET):
    """(the reference's records, its visible target pictures)"""
    (iw, ih), (tw, th) = IN, target
    recs = S.run([G.components(fmt, pl, iw, ih)[0] for pl in planes], setting, crops, iw, ih)
    want = []
    for i, (pl, r) in enumerate(zip(planes, recs)):
        c = crops[i] if isinstance(crops, list) else crops
        sy, suv = S.to_nv12(fmt, pl, iw, ih, c, dst, tw, th, r["ox"], r["oy"])
        if moved_too:  # at 1:1 and 2:1 the displaced base tables are the moved crop's
            my, muv = G.to_nv12(fmt, pl, iw, ih, (c[0] + r["ox"], c[1] + r["oy"], c[2], c[3]), dst, tw, th)
            assert np.array_equal(sy, my) and np.array_equal(suv, muv), i
        want.append((np.ascontiguousarray(sy[:th, :tw]), np.ascontiguousarray(suv[:th // 2, :tw])))
    return recs, want


def stabilising(E, target, crop, dst, setting=SET, keep_sar=False, **kw):
    return E.Encoder(target[0], target[1], gop=GOP, fixed_qp=QP, pipeline_depth=2, geometry=E.geometry(IN, crop=crop, dst=dst, keep_sar=keep_sar),
                     stabilize=dict(range=setting[0], leak=setting[1], margin=(setting[2], setting[3])), **kw)


@pytest.mark.parametrize("target, crop, keep_sar", [((128, 64), CROP, False), ((64, 32), CROP, False), ((100, 50), (20, 18, 120, 60), True)], ids=["1:1", "2:1", "6:5"])
def test_stream_equals_the_plain_encoder_fed_the_references_pictures(E, clip, target, crop, keep_sar):
    dst = (0, 0) + target
    recs, want = reference(G.FMT_NV12, [list(p) for p in clip], crop, dst, target, moved_too=not keep_sar)
    conditions(recs)
    ref = plain_stream(E, target[0], target[1], want)
    e = stabilising(E, target, crop, dst, keep_sar=keep_sar)
    assert e.debug_stabilize_bytes() == 0 and e.get_stabilize() == dict(range=8, leak=16, margin_x=16, margin_y=16)
    got, infos = run(e, lambda i: e.submit(*clip[i], pts=i), len(clip))
    assert e.debug_stabilize_bytes() > 8 * (IN[0] + IN[1]) * 4 and e.last_stabilize()[0] == e.get_stabilize()
    e.close()
    assert infos == recs
    same(got, ref)


SMALL = (64, 32)


@pytest.mark.parametrize("fmt", [G.FMT_I420, G.FMT_YUY2, G.FMT_UYVY], ids=["i420", "yuy2", "uyvy"])
def test_stream_through_submit_fmt(E, clip, fmt):
    planes = [planes_in(fmt, p) for p in clip]
    recs, want = reference(fmt, planes, CROP, (0, 0) + SMALL, SMALL)
    conditions(recs)
    ref = plain_stream(E, SMALL[0], SMALL[1], want)
    e = stabilising(E, SMALL, CROP, (0, 0) + SMALL)
    got, infos = run(e, lambda i: e.submit_fmt(fmt, planes[i], pts=i), len(clip))
    e.close()
    assert infos == recs
    same(got, ref)


def test_stream_through_submit_device_at_an_odd_address_and_stride(E, clip):
    iw, ih = IN
    recs, want = reference(G.FMT_NV12, [list(p) for p in clip], CROP, (0, 0) + SMALL, SMALL)
    ref = plain_stream(E, SMALL[0], SMALL[1], want)
    dev = [_device_container(E, p, [ih, ih // 2], [iw, iw], iw + 5, 3, 900 + i) for i, p in enumerate(clip)]
    e = stabilising(E, SMALL, CROP, (0, 0) + SMALL)
    got, infos = run(e, lambda i: e.submit_device(dev[i][2][0], iw + 5, dev[i][2][1], iw + 5, pts=i), len(clip))
    e.close()
    for hip, buf, _ in dev:
        hip.hipFree(buf)
    assert infos == recs
    same(got, ref)


def test_offsets_are_pre_orientation(E, clip):
    tw, th = SMALL
    recs, want = reference(G.FMT_NV12, [list(p) for p in clip], CROP, (0, 0) + SMALL, SMALL)
    w, h = orientref.size(1, tw, th)
    ref = plain_stream(E, w, h, [orientref.orient(y, uv, 1) for y, uv in want])
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, orientation="90r", geometry=E.geometry(IN, crop=CROP, dst=(0, 0) + SMALL), stabilize=dict(range=8, margin=16))
    got, infos = run(e, lambda i: e.submit(*clip[i], pts=i), len(clip))
    e.close()
    assert infos == recs
    same(got, ref)


def test_with_the_noise_filter_behind_it(E, clip):
    dn = dict(luma=8, chroma=8, motion=4)
    recs, want = reference(G.FMT_NV12, [list(p) for p in clip], CROP, (0, 0) + SMALL, SMALL)
    ref = plain_stream(E, SMALL[0], SMALL[1], want, denoise=dict(dn))
    e = stabilising(E, SMALL, CROP, (0, 0) + SMALL, denoise=dict(dn))
    got, infos = run(e, lambda i: e.submit(*clip[i], pts=i), len(clip))
    e.close()
    assert infos == recs
    same(got, ref)


def test_set_crop_between_pictures_moves_the_bounds_and_keeps_the_state(E, clip):
    crops = [CROP] * 4 + [(4, 8, 128, 64)] * 4 + [(28, 30, 128, 64)] * (len(clip) - 8)
    recs, want = reference(G.FMT_NV12, [list(p) for p in clip], crops, (0, 0) + SMALL, SMALL)
    conditions(recs, on_bound=False)
    assert recs[4]["sx"] == -4 * 256 and recs[4]["ox"] == -4  # the new bound cuts the state it met ...
    assert all(r["ox"] <= 4 and r["oy"] <= 2 for r in recs[8:]) and recs[-1]["ox"] == 4  # ... and the last crop has 4 / 2 samples of room
    ref = plain_stream(E, SMALL[0], SMALL[1], want)
    e = stabilising(E, SMALL, CROP, (0, 0) + SMALL)
    got, infos = run(e, lambda i: e.submit(*clip[i], pts=i), len(clip), before=lambda i: e.set_crop(*crops[i]))
    e.close()
    assert infos == recs
    same(got, ref)


def test_jpeg_stills_do_not_move(E):
    data = open(JPEG, "rb").read()
    geom = dict(crop=(8, 4, 56, 32), dst=(0, 0, 56, 32))
    a = E.Encoder(56, 32, gop=GOP, fixed_qp=QP, pipeline_depth=2, geometry=E.geometry((72, 40), **geom))
    ref, _ = run(a, lambda i: a.submit_jpeg(data, pts=i), 4)
    a.close()
    e = E.Encoder(56, 32, gop=GOP, fixed_qp=QP, pipeline_depth=2, geometry=E.geometry((72, 40), **geom), stabilize=dict(range=8, margin=4))
    got, infos = run(e, lambda i: e.submit_jpeg(data, pts=i), 4)
    e.close()
    assert infos[0] == dict.fromkeys(S.KEYS, 0)
    for r in infos[1:]:
        assert r["votes_x"] >= 3 and r["votes_y"] >= 3 and (r["mx"], r["my"], r["ox"], r["oy"], r["sx"], r["sy"]) == (0,) * 6
    same(got, ref)


# ---- off
def test_range_0_is_the_plain_geometry_stream_and_allocates_nothing(E, clip):
    a = E.Encoder(SMALL[0], SMALL[1], gop=GOP, fixed_qp=QP, pipeline_depth=2, geometry=E.geometry(IN, crop=CROP, dst=(0, 0) + SMALL))
    ref, _ = run(a, lambda i: a.submit(*clip[i], pts=i), 5)
    a.close()
    e = E.Encoder(SMALL[0], SMALL[1], gop=GOP, fixed_qp=QP, pipeline_depth=2, geometry=E.geometry(IN, crop=CROP, dst=(0, 0) + SMALL))
    e.set_stabilize(range=0, leak=100, margin=16)
    got, infos = run(e, lambda i: e.submit(*clip[i], pts=i), 5)
    assert e.debug_stabilize_bytes() == 0 and infos == [dict.fromkeys(S.KEYS, 0)] * 5
    for stage in (E.STAGE_STABILIZE_PROJECT, E.STAGE_STABILIZE_MATCH):
        with pytest.raises(E.EncoderError, match=r"\(-6\)"):
            e.time_stage(stage, 2)
    e.close()
    same(got, ref)


def test_on_off_on_primes_again(E, clip):
    n, off = len(clip), range(5, 7)
    lumas = [p[0] for p in clip]
    recs = S.run(lumas[:5], SET, CROP, *IN) + [dict.fromkeys(S.KEYS, 0)] * 2 + S.run(lumas[7:], SET, CROP, *IN)
    assert recs[7] == dict.fromkeys(S.KEYS, 0) and (recs[8]["mx"], recs[8]["my"]) == S.SCRIPT[8] and recs[8]["sx"] == 256 * recs[8]["mx"]
    want = []
    for p, r in zip(clip, recs):
        sy, suv = S.to_nv12(G.FMT_NV12, list(p), IN[0], IN[1], CROP, (0, 0) + SMALL, SMALL[0], SMALL[1], r["ox"], r["oy"])
        want.append((np.ascontiguousarray(sy[:SMALL[1], :SMALL[0]]), np.ascontiguousarray(suv[:SMALL[1] // 2, :SMALL[0]])))
    ref = plain_stream(E, SMALL[0], SMALL[1], want)
    e = stabilising(E, SMALL, CROP, (0, 0) + SMALL)
    got, infos = run(e, lambda i: e.submit(*clip[i], pts=i), n, before=lambda i: e.set_stabilize(range=0 if i in off else 8, margin=16))
    e.close()
    assert infos == recs
    same(got, ref)


def test_refusals(E, clip):
    e = E.Encoder(160, 96, fixed_qp=QP, pipeline_depth=2, stabilize=dict(range=8, margin=16))  # no geometry
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.submit(*clip[0])
    assert e.pending == 0
    e.set_stabilize(None)
    e.submit(*clip[0])
    e.collect()
    e.close()
    e = stabilising(E, SMALL, CROP, (0, 0) + SMALL, setting=(25, 16, 16, 16))  # 4 x 25 > 96
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        e.submit(*clip[0])
    assert e.pending == 0 and e.debug_stabilize_bytes() == 0
    e.set_stabilize(range=24, margin=16)
    e.submit(*clip[0])
    # both probes refuse pictures in flight
    luma = np.zeros((48, 64), np.uint8)
    sums = S.project(luma)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.stabilize_probe_project(luma)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.stabilize_probe_match(sums, sums, E.stabilize(range=4), (0, 0, 0, 0))
    e.collect()
    assert e.stabilize_probe_project(luma)[0].sum() == 0
    e.close()


def test_timed_stages_run_when_on_and_leave_the_state_unprimed(E, clip):
    e = stabilising(E, SMALL, CROP, (0, 0) + SMALL)
    e.submit(*clip[0], pts=0)
    e.submit(*clip[1], pts=1)
    e.collect(); e.collect()
    assert e.last_stabilize()[1]["mx"] == S.SCRIPT[1][0]
    assert e.time_stage(E.STAGE_STABILIZE_PROJECT, 3) > 0 and e.time_stage(E.STAGE_STABILIZE_MATCH, 3) > 0
    e.submit(*clip[2], pts=2)  # primes: the probes' sums are no picture's
    e.collect()
    assert e.last_stabilize()[1] == dict.fromkeys(S.KEYS, 0)
    e.close()


def test_rgb_is_measured_on_the_nv12_intermediate(E, clip):
    """RGB input is converted at the input size first; the estimate and the geometry launch read that NV12 picture"""
    iw, ih = IN
    rgb = [np.ascontiguousarray(np.repeat(p[0][:, :, None], 3, axis=2).reshape(ih, 3 * iw)) for p in clip]  # grey: R = G = B = the clip's luma
    conv = E.Encoder(iw, ih, fixed_qp=QP)
    mid = [conv.stage_csc(E.FMT_RGB, [a]) for a in rgb]  # (160 x 96 is whole macroblocks: the surfaces are the picture)
    conv.close()
    assert mid[0][0].shape == (ih, iw) and not np.array_equal(mid[0][0], clip[0][0])
    recs, want = reference(G.FMT_NV12, [list(m) for m in mid], CROP, (0, 0) + SMALL, SMALL)
    conditions(recs)
    ref = plain_stream(E, SMALL[0], SMALL[1], want)
    e = stabilising(E, SMALL, CROP, (0, 0) + SMALL)
    got, infos = run(e, lambda i: e.submit_fmt(E.FMT_RGB, [rgb[i]], pts=i), len(clip))
    e.close()
    assert infos == recs
    same(got, ref)


GENTLE = [(0, 0), (2, -1), (1, 2), (-3, 1), (2, 2), (3, -3), (-1, -2), (2, 1), (1, -3), (3, 2), (-2, 2), (1, 1)]  # any two neighbours stay inside range 8


def test_rate_conversion_hold_measures_between_the_kept_pictures(E):
    """hold at half rate: every other input is dropped before it is measured, so the motion between two kept pictures spans both intervals"""
    pics = S.clip(*IN, script=GENTLE)
    rate = (1, 120, 0)  # inputs at 120 pts units a second into a 60 fps stream
    e = stabilising(E, SMALL, CROP, (0, 0) + SMALL, rate=rate)
    counts = []
    got, infos = run(e, lambda i: counts.append(e.submit(*pics[i], pts=i)), len(pics))
    e.close()
    kept = [i for i, c in enumerate(counts) if c]
    assert set(counts) == {0, 1} and len(infos) == len(kept) and sum(b - a == 2 for a, b in zip(kept, kept[1:])) >= 4  # (which inputs the rule keeps is its own business)
    recs = S.run([pics[i][0] for i in kept], SET, CROP, *IN)
    for a, b, r in zip(kept, kept[1:], recs[1:]):  # the reference measures the scripted motion over both intervals
        assert (r["mx"], r["my"]) == tuple(sum(m[k] for m in GENTLE[a + 1:b + 1]) for k in (0, 1)) and r["votes_x"] >= 3 and r["votes_y"] >= 3
    assert len({(r["ox"], r["oy"]) for r in recs}) >= 4
    offs = dict(zip(kept, recs))
    want = []
    for i, p in enumerate(pics):  # (what a dropped input shows does not matter: the plain encoder drops it too)
        r = offs.get(i, dict(ox=0, oy=0))
        sy, suv = S.to_nv12(G.FMT_NV12, list(p), IN[0], IN[1], CROP, (0, 0) + SMALL, SMALL[0], SMALL[1], r["ox"], r["oy"])
        want.append((np.ascontiguousarray(sy[:SMALL[1], :SMALL[0]]), np.ascontiguousarray(suv[:SMALL[1] // 2, :SMALL[0]])))
    ref = plain_stream(E, SMALL[0], SMALL[1], want, rate=rate)
    assert infos == recs
    same(got, ref)
