"""GPU: temporal noise reduction on the way in bit for bit against tests/denoiseref.py: the step alone -- pictures and both histories --
at the smallest sizes at which each thing can go wrong and on content that sits on every knee of the rule; then inside streams: latched per input picture,
primed again behind a picture without it, in front of the picture controls, under a letterbox, under frame-rate conversion, from device planes, and off."""
import numpy as np
import pytest

from tests import denoiseref as D
from tests import rateref
from tests.inputref import device_free
from tests.test_adjust_gpu import want as adjusted_want
from tests.test_csc_formats_gpu import drain, same
from tests.test_yuv_convert_gpu import dev_get, dev_put

pytestmark = pytest.mark.gpu

# visible size, coded size.  16 x 16: one macroblock, four blocks, less than a wave; 42 x 26: partly visible blocks right and below, none wholly in the margin;
# 64 x 24: a whole block row in the margin; 520 x 16: 66 blocks a row (65 with visible samples and a block column wholly in the margin), so a wave's 16 blocks wrap rows
SIZES = [(16, 16, 16, 16), (42, 26, 48, 32), (64, 24, 64, 32), (520, 16, 528, 16)]
STRENGTHS = [(8, 8), (8, 0), (0, 8), (32, 3)]
QP, GOP = 28, 8


def noise16(rng, shape):
    return rng.integers(0, 4081, shape, dtype=np.uint16)


def contents(vw, vh, W, H, luma, chroma, seed):
    """name -> (y, uv, hist_y, hist_uv): coded surfaces and histories (a chroma history only where the chroma is filtered)"""
    rng = np.random.default_rng(seed)
    cs, out = (H // 2, W), {}
    huv = lambda a: a if chroma else None
    # noise against a noise history, margins and all: a block that is partly visible is computed from the surface as it lies
    out["noise"] = (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, cs, dtype=np.uint8), noise16(rng, (H, W)), huv(noise16(rng, cs)))
    # near the history, so that blocks are filtered with every weight; visible samples with replicated margins, as the encoder's surfaces are
    by, buv = D.with_margins(rng.integers(30, 226, (vh, vw), dtype=np.uint8), rng.integers(30, 226, (vh // 2, vw), dtype=np.uint8), W, H)
    hy, hc = 16 * by.astype(np.int64) + rng.integers(-8, 8, by.shape), 16 * buv.astype(np.int64) + rng.integers(-8, 8, buv.shape)
    amp = max(luma, chroma)
    near = lambda b, a: np.clip(b.astype(np.int64) + np.rint(rng.standard_normal(b.shape) * a), 0, 255).astype(np.uint8)
    out["near"] = (near(by, amp / 2), near(buv, amp / 2), hy.astype(np.uint16), huv(hc.astype(np.uint16)))
    out["equal"] = (by, buv, (16 * by.astype(np.uint16)), huv(16 * buv.astype(np.uint16)))
    # the knees of P: four samples a block differ by s, s + 1, 3 s - 1, 3 s (the block measure stays at s / 2: full block weight)
    y, uv = by.copy().astype(np.int64), buv.copy().astype(np.int64)
    for s, plane, rows in ((luma or chroma, y, 8), (chroma, uv, 4)):
        if s:
            for k, d in enumerate((s, s + 1, 3 * s - 1, 3 * s)):
                sign = np.where(plane[k % rows::rows, 2 * k + 1::8] > 128, -1, 1)
                plane[k % rows::rows, 2 * k + 1::8] += sign * d
    out["knees-P"] = (y.astype(np.uint8), uv.astype(np.uint8), 16 * by.astype(np.uint16), huv(16 * buv.astype(np.uint16)))
    # the knees of B: block sums with M >> 4 = 2 s, 2 s + 1, 6 s - 1, 6 s, spread evenly over the block's 64 samples
    s = luma or chroma
    y = by.astype(np.int64)
    targets = (2 * s, 2 * s + 1, 6 * s - 1, 6 * s)
    n = 0
    for r in range(0, H, 8):
        for c in range(0, W, 8):
            m = 16 * targets[n % 4] + (n // 4) % 16
            d = np.full(64, m // 64) + (np.arange(64) < m % 64)
            blk = y[r:r + 8, c:c + 8]
            blk += np.where(blk > 128, -1, 1) * d.reshape(8, 8)
            n += 1
    out["knees-B"] = (y.astype(np.uint8), near(buv, chroma / 2), 16 * by.astype(np.uint16), huv(16 * buv.astype(np.uint16)))
    # 0 <-> 255 with H at 0 and at 4080
    flip = lambda shape: rng.choice(np.array([0, 255], np.uint8), shape)
    flip16 = lambda shape: rng.choice(np.array([0, 4080], np.uint16), shape)
    out["flips"] = (flip((H, W)), flip(cs), flip16((H, W)), huv(flip16(cs)))
    out["prime"] = (out["noise"][0], out["noise"][1], None, None)
    if luma and chroma:  # the luma filtered beside a chroma that primes
        out["chroma-primes"] = out["near"][:3] + (None,)
    return out


def equal_or_none(got, ref, what):
    assert (got is None) == (ref is None), what
    if ref is not None:
        assert got.dtype == ref.dtype and np.array_equal(got, ref), (what, np.argwhere(got != ref)[:4])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("luma,chroma", STRENGTHS)
def test_stage_denoise_matches_numpy(E, size, luma, chroma):
    vw, vh, W, H = size
    e = E.Encoder(vw, vh, fixed_qp=30)
    assert (e.mbw * 16, e.mbh * 16) == (W, H)
    moved = set()
    for name, (y, uv, hy, huv) in contents(vw, vh, W, H, luma, chroma, 1000 * vw + 10 * luma + chroma).items():
        got = e.stage_denoise(dict(luma=luma, chroma=chroma), y, uv, hy, huv)
        ref = D.step(y, uv, hy, huv, luma, chroma, visible=(vw, vh))
        for g, r, what in zip(got, ref, ("y", "uv", "hist_y", "hist_uv")):
            equal_or_none(g, r, (name, what))
        if not np.array_equal(got[0][:vh, :vw], y[:vh, :vw]):  # (the visible part: a block wholly in the margin becomes a replica whatever it held)
            moved.add((name, "y"))
        if not np.array_equal(got[1][:vh // 2, :vw], uv[:vh // 2, :vw]):
            moved.add((name, "uv"))
        assert got[2].max() <= 4080 and (got[3] is None or got[3].max() <= 4080)
    # the cases do what they are there for: the filter moves the planes it is set for and no other; equal, flips and prime move nothing
    assert {n for n, _ in moved} <= {"noise", "near", "knees-P", "knees-B", "chroma-primes"}
    assert (("near", "y") in moved) == (luma > 0) and (("near", "uv") in moved) == (chroma > 0) and ("chroma-primes", "uv") not in moved
    assert (("knees-P", "y") in moved) == (luma > 0) and (("knees-B", "y") in moved) == (luma > 0)
    assert e.debug_denoise_bytes() == 0  # (the stage's histories are its own)
    e.close()


def test_stage_denoise_off_and_refused_values(E):
    e = E.Encoder(64, 48, fixed_qp=30)
    rng = np.random.default_rng(5)
    y, uv = rng.integers(0, 256, (48, 64), dtype=np.uint8), rng.integers(0, 256, (24, 64), dtype=np.uint8)
    got = e.stage_denoise({}, y, uv)
    same(got[:2], (y, uv))
    assert got[2] is None and got[3] is None
    for bad in (dict(luma=-1), dict(luma=33), dict(chroma=-1), dict(chroma=33)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.stage_denoise(bad, y, uv)
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.set_denoise(bad)
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):  # a chroma history without the luma's: nothing to measure against
        e.stage_denoise(dict(luma=8, chroma=8), y, uv, None, np.zeros(uv.shape, np.uint16))
    assert e.get_denoise() == dict(luma=0, chroma=0)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.last_denoise()
    e.close()


# ---- streams
def noisy_clip(w, h, n, seed, sigma=3.0):
    """static content plus seeded Gaussian noise: visible NV12 pictures"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 60 + xx + yy // 2 + 40 * ((xx // 16 + yy // 8) & 1)
    cbase = 128 + 24 * ((xx[:h // 2] // 8) & 1) - 10 * ((yy[:h // 2] // 4) & 1)
    noisy = lambda p: np.clip(np.rint(p + sigma * rng.standard_normal(p.shape)), 0, 255).astype(np.uint8)
    return [(noisy(base), noisy(cbase)) for _ in range(n)]


def coded(pics, w, h):
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    return [D.with_margins(y, uv, W, H) for y, uv in pics]


def sources(e, E):
    return e.fetch(E.FETCH_SOURCE_Y), e.fetch(E.FETCH_SOURCE_UV)


def test_a_stream_follows_the_chain_through_strength_changes_and_primes_again_behind_a_picture_without(E):
    w, h, depth = 64, 48, 2
    pics = noisy_clip(w, h, 6, 21)
    strengths = [(8, 8), (8, 8), (16, 4), (0, 0), (8, 8), (8, 8)]  # changed mid-stream with the history kept; off; 0 -> 8 primes again
    ref = D.chain(coded(pics, w, h), strengths)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(luma=8, chroma=8))
    assert e.get_denoise() == dict(luma=8, chroma=8)
    seen = []

    def check():
        e.collect()
        i = len(seen)
        same(sources(e, E), ref[i])
        assert e.last_denoise() == dict(luma=strengths[i][0], chroma=strengths[i][1])
        seen.append(i)
    for i in range(6):
        e.set_denoise(luma=strengths[i][0], chroma=strengths[i][1])
        e.submit(*pics[i], pts=i)
        if e.pending > depth:  # three in flight
            check()
    while e.pending:
        check()
    assert seen == list(range(6))
    # the cases do what they are here for: the first picture and the one behind the gap are their inputs, the others are not
    cp = coded(pics, w, h)
    assert all(np.array_equal(ref[i][0], cp[i][0]) and np.array_equal(ref[i][1], cp[i][1]) for i in (0, 3, 4))
    assert all(not np.array_equal(ref[i][0], cp[i][0]) and not np.array_equal(ref[i][1], cp[i][1]) for i in (1, 2, 5))
    assert e.debug_denoise_bytes() == 3 * 64 * 48
    e.close()


@pytest.mark.parametrize("strength", [(8, 0), (0, 8)], ids=["luma-only", "chroma-only"])
def test_a_stream_with_one_plane_and_then_the_other(E, strength):
    """a plane whose strength was 0 for the previous picture primes while the other goes on being filtered"""
    w, h = 64, 48
    pics = noisy_clip(w, h, 4, 22)
    strengths = [strength, strength, (8, 8), (8, 8)]
    ref = D.chain(coded(pics, w, h), strengths)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP)
    for i in range(4):
        e.set_denoise(luma=strengths[i][0], chroma=strengths[i][1])
        e.submit(*pics[i], pts=i)
        e.collect()
        same(sources(e, E), ref[i])
        if i == 1:
            assert e.debug_denoise_bytes() == (2 if strength[1] == 0 else 3) * 64 * 48  # (while only the chroma is filtered the luma's history follows the luma)
    e.close()


def test_the_filter_runs_in_front_of_the_picture_controls(E):
    w, h = 64, 48
    pics = noisy_clip(w, h, 3, 23)
    a = dict(sharpen=32, contrast=1100)
    ref = D.chain(coded(pics, w, h), [(8, 8)] * 3)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, denoise=dict(luma=8, chroma=8), adjust=a)
    for i in range(3):
        e.submit(*pics[i], pts=i)
        e.collect()
        same(sources(e, E), adjusted_want(E, ref[i][0], ref[i][1], a, visible=(w, h)))  # filtered, then sharpened: the history never sees a sharpened picture
    e.close()


def test_under_a_letterbox_the_border_keeps_its_bytes(E):
    w, h, dst = 128, 96, (20, 12, 88, 72)
    pics = noisy_clip(160, 96, 3, 24)
    kw = dict(gop=GOP, fixed_qp=QP, geometry=E.geometry((160, 96), dst=dst))
    plain, e = E.Encoder(w, h, **kw), E.Encoder(w, h, denoise=dict(luma=8, chroma=8), **kw)
    scaled = []
    for i in range(3):  # what the step finds: the scaled picture inside its border, from a handle without the filter
        plain.submit(*pics[i], pts=i)
        plain.collect()
        scaled.append(sources(plain, E))
    ref = D.chain(scaled, [(8, 8)] * 3)
    inside = np.zeros((h, w), bool)
    inside[dst[1]:dst[1] + dst[3], dst[0]:dst[0] + dst[2]] = True
    for i in range(3):
        e.submit(*pics[i], pts=i)
        e.collect()
        got = sources(e, E)
        same(got, ref[i])
        assert np.array_equal(got[0][~inside], scaled[i][0][~inside]) and np.array_equal(got[1][~inside[0::2]], scaled[i][1][~inside[0::2]])
        assert np.all(got[0][~inside] == 16) and (i == 0 or not np.array_equal(got[0][inside], scaled[i][0][inside]))
    plain.close(); e.close()


def test_hold_mode_repeats_the_filtered_picture_and_a_dropped_input_never_reaches_the_filter(E):
    w, h, ns = 64, 48, 10 ** 9
    pics = noisy_clip(w, h, 5, 25)
    cp = coded(pics, w, h)
    # 30 -> 60: the tick in between repeats the previous output picture, which was filtered once
    e = E.Encoder(w, h, fps=60, gop=GOP, fixed_qp=QP, pipeline_depth=2, rate=(rateref.HOLD, ns, 2), denoise=dict(luma=8, chroma=8))
    ref = D.chain(cp[:2], [(8, 8)] * 2)
    assert e.submit(*pics[0], pts=0) == 1
    e.collect()
    same(sources(e, E), ref[0])
    assert e.submit(*pics[1], pts=ns // 30) == 2
    e.collect()
    same(sources(e, E), ref[0])
    e.collect()
    same(sources(e, E), ref[1])
    assert e.rate_stats()["repeated"] == 1 and not np.array_equal(ref[1][0], cp[1][0])
    e.close()
    # 60 -> 30: every other input is dropped before transfer; "the previous picture" is the previous one that went through the step
    pts = [i * ns // 60 for i in range(5)]
    steps = rateref.run(rateref.HOLD, ns, 30, 1, 2, pts)
    kept = [i for i, (o, _, _) in enumerate(steps) if len(o)]
    assert 2 <= len(kept) < 5
    ref = dict(zip(kept, D.chain([cp[i] for i in kept], [(8, 8)] * len(kept))))
    e = E.Encoder(w, h, fps=30, gop=GOP, fixed_qp=QP, pipeline_depth=2, rate=(rateref.HOLD, ns, 2), denoise=dict(luma=8, chroma=8))
    for i in range(5):
        assert e.submit(*pics[i], pts=pts[i]) == (1 if i in kept else 0)
        if i in kept:
            e.collect()
            same(sources(e, E), ref[i])
    assert e.rate_stats()["dropped"] == 5 - len(kept)
    e.close()


def test_blend_mode_mixes_filtered_pictures(E):
    """the converting stream of the noisy pictures with the filter is, access unit for access unit, the converting stream of the pre-filtered pictures without"""
    w, h, ns, n = 64, 48, 10 ** 9, 6
    pics = noisy_clip(w, h, n, 26)
    pre = D.chain(coded(pics, w, h), [(8, 8)] * n)
    pts = [i * ns // 25 for i in range(n)]
    out = []
    for kw, src in ((dict(denoise=dict(luma=8, chroma=8)), pics), ({}, pre)):
        e = E.Encoder(w, h, fps=30, gop=GOP, fixed_qp=QP, pipeline_depth=2, rate=(rateref.BLEND, ns, 2), **kw)
        aus = []
        for i in range(n):
            while e.pending + max(e.rate_peek(pts[i]), 1) > 3:
                aus.append(e.collect()[:2])
            e.submit(np.ascontiguousarray(src[i][0][:h, :w]), np.ascontiguousarray(src[i][1][:h // 2, :w]), pts=pts[i])
        while e.pending:
            aus.append(e.collect()[:2])
        assert e.rate_stats()["blended"] >= 2
        out.append(aus)
        e.close()
    assert out[0] == out[1] and len(out[0]) >= n


def test_submit_device_never_filters_the_callers_planes(E):
    """64 x 48 on aligned planes would take the in-place exit: with the filter it must not, and the planes stay what they were"""
    w, h, depth = 64, 48, 2
    pics = noisy_clip(w, h, 3, 27)
    dev = [(dev_put(y), dev_put(uv)) for y, uv in pics]
    a = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(luma=8, chroma=8))
    b = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    got = drain(a, depth, lambda i: a.submit_device(dev[i][0], w, dev[i][1], w, pts=i), 3)
    pre = D.chain(coded(pics, w, h), [(8, 8)] * 3)
    assert got == drain(b, depth, lambda i: b.submit(pre[i][0], pre[i][1], pts=i), 3)
    assert not np.array_equal(pre[2][0], pics[2][0]) and not np.array_equal(pre[2][1], pics[2][1])
    for (dy, duv), (y, uv) in zip(dev, pics):
        assert np.array_equal(dev_get(dy, y.shape), y) and np.array_equal(dev_get(duv, uv.shape), uv)
    a.close(); b.close()
    for dy, duv in dev:
        device_free(dy); device_free(duv)


def test_off_is_off(E):
    w, h, depth = 64, 48, 2
    pics = noisy_clip(w, h, 4, 28)
    never = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    zero = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(luma=0, chroma=0))
    zero.set_denoise()
    ref = drain(never, depth, lambda i: never.submit(*pics[i], pts=i), 4)
    assert drain(zero, depth, lambda i: zero.submit(*pics[i], pts=i), 4) == ref
    assert never.debug_denoise_bytes() == 0 and zero.debug_denoise_bytes() == 0
    assert never.last_denoise() == dict(luma=0, chroma=0)
    on = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(luma=8, chroma=8))
    assert on.debug_denoise_bytes() == 0  # never before the first filtered picture
    on.submit(*pics[0], pts=0)
    on.collect()
    assert on.debug_denoise_bytes() == 3 * 64 * 48  # two bytes per luma and per chroma sample
    never.close(); zero.close(); on.close()


def test_a_filtered_stream_decodes_to_the_devices_reconstruction(E, oracle):
    w, h, depth, n = 64, 48, 2, 6
    pics = noisy_clip(w, h, n, 29)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(luma=8, chroma=8))
    plain = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    got = drain(e, depth, lambda i: e.submit(*pics[i], pts=i), n)
    dec = oracle.Decoder()
    for au, _ in got:
        dy, duv = dec.decode(au)
    assert np.array_equal(dy, e.fetch(E.FETCH_RECON_Y)) and np.array_equal(duv, e.fetch(E.FETCH_RECON_UV))
    ref = drain(plain, depth, lambda i: plain.submit(*pics[i], pts=i), n)
    assert got[0] == ref[0]  # the first picture primes: the same access unit
    assert got[1:] != ref[1:]
    print("bytes of the P pictures: filtered %d, plain %d" % (sum(len(a) for a, _ in got[1:]), sum(len(a) for a, _ in ref[1:])))  # (tools/denoise_price.py measures this properly)
    e.close(); plain.close()


@pytest.mark.parametrize("path", ["host", "device"])
def test_a_height_that_ends_inside_a_block_row_does_not_read_what_the_slots_held(E, path):
    """64 x 44 in 64 x 48: the width is a multiple of 16, so a plain NV12 copy pads nothing by itself, and rows 44 .. 47 lie in the block row 40 .. 47 whose
    measure the filter takes as the surface lies.  Slot 0's margin is made to differ from the other slots' (noise through a stage call, which uploads whole
    coded surfaces); the sources must still follow the chain over pictures with replicated margins."""
    w, h, depth, n = 64, 44, 2, 6
    pics = noisy_clip(w, h, n, 33)
    ref = D.chain(coded(pics, w, h), [(8, 8)] * n)
    assert any(not np.array_equal(ref[i][0][40:44], pics[i][0][40:44]) for i in range(1, n))  # (the bottom block row is filtered)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(luma=8, chroma=8))
    rng = np.random.default_rng(34)
    e.stage_denoise({}, rng.integers(0, 256, (48, 64), dtype=np.uint8), rng.integers(0, 256, (24, 64), dtype=np.uint8))
    dev = [(dev_put(y), dev_put(uv)) for y, uv in pics] if path == "device" else None
    seen = []

    def check():
        e.collect()
        same(sources(e, E), ref[len(seen)])
        seen.append(1)
    for i in range(n):
        if dev:
            e.submit_device(dev[i][0], w, dev[i][1], w, pts=i)
        else:
            e.submit(*pics[i], pts=i)
        if e.pending > depth:
            check()
    while e.pending:
        check()
    assert len(seen) == n
    e.close()
    for dy, duv in dev or ():
        device_free(dy); device_free(duv)


def test_a_stream_behind_a_timed_launch_primes(E):
    """mi355enc_time_stage 25 / 26 work on the handle's own history; the stream that follows must not filter against what they left"""
    w, h = 64, 48
    pics = noisy_clip(w, h, 2, 35)
    ref = D.chain(coded(pics, w, h), [(8, 8)] * 2)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, denoise=dict(luma=8, chroma=8))
    e.stage_denoise({}, *coded(noisy_clip(w, h, 1, 36), w, h)[0])  # slot 0 holds a picture near the stream's: a history of it would filter
    assert e.time_stage(E.STAGE_DENOISE, 2) > 0 and e.time_stage(E.STAGE_DENOISE_PRIME, 1) > 0
    for i in range(2):
        e.submit(*pics[i], pts=i)
        e.collect()
        same(sources(e, E), ref[i])
    e.close()
