"""GPU: the motion-compensated noise filter bit for bit against tests/denoisemcref.py: the search alone and the search with the compensated
filter at the sizes, ranges and strengths at which each thing can go wrong; then inside streams -- the range latched per input picture and changed between
pictures with the history kept, off, from device planes, under frame-rate conversion, through a recovery, behind a timed launch, and decoded."""
import numpy as np
import pytest

from tests import denoisemcref as M
from tests import denoiseref as D
from tests import rateref
from tests.inputref import device_free
from tests.test_csc_formats_gpu import drain, same
from tests.test_denoise_gpu import coded, equal_or_none, noise16, sources
from tests.test_yuv_convert_gpu import dev_get, dev_put

pytestmark = pytest.mark.gpu

# visible size, coded size.  32 x 32: at range 16 every restriction of the candidates bites; 42 x 26: margin columns, partly visible blocks; 64 x 44: the height ends
# inside a block row; 208 x 80: four tiles across and three down, more than one workgroup, the last tile column and row cut short
SIZES = [(32, 32, 32, 32), (42, 26, 48, 32), (64, 44, 64, 48), (208, 80, 208, 80)]
RANGES = [1, 4, 8, 16]
STRENGTHS = [(8, 8), (8, 0), (0, 8), (32, 32)]
QP, GOP = 28, 8


def contents(vw, vh, W, H, r, luma, chroma, seed):
    """name -> (y, uv, hist_y, hist_uv): coded surfaces and histories (a chroma history only where the chroma is filtered); noise in the margins throughout"""
    rng = np.random.default_rng(seed)
    cs, out = (H // 2, W), {}
    huv = lambda a: a if chroma else None
    # one picture shifted per quadrant by a vector of its own -- (r, -r) at the corner of the range, odd / odd for the chroma's four-tap case, one odd axis each
    # way -- plus sigma-3 noise, against a history within half a code of the unshifted one
    odd = r if r & 1 else r - 1
    vectors = [(odd, odd), (-(r & ~1), odd), (r, -r), (-odd, -(r & ~1))]  # per quadrant, pointing into the picture: the displaced blocks lie inside
    shifts = [(-vx, -vy) for vx, vy in vectors]
    big = np.kron(rng.integers(30, 226, ((H + 32) // 2, (W + 32) // 2)), np.ones((2, 2), np.int64))
    bigc = rng.integers(30, 226, (H // 2 + 16, W + 32))
    y, uv = np.empty((H, W), np.int64), np.empty(cs, np.int64)
    for q, (a, b) in enumerate(shifts):
        ys, xs = slice((q >> 1) * (H // 2), ((q >> 1) + 1) * (H // 2)), slice((q & 1) * (W // 2), ((q & 1) + 1) * (W // 2))
        y[ys, xs] = big[16 - b:16 - b + H, 16 - a:16 - a + W][ys, xs]
        cys = slice(ys.start // 2, ys.stop // 2)
        uv[cys, xs] = bigc[8 - (b >> 1):8 - (b >> 1) + H // 2, 16 - 2 * (a >> 1):16 - 2 * (a >> 1) + W][cys, xs]
    noisy = lambda p: np.clip(np.rint(p + 3.0 * rng.standard_normal(p.shape)), 0, 255).astype(np.uint8)
    hy = np.clip(16 * big[16:16 + H, 16:16 + W] + rng.integers(-8, 8, (H, W)), 0, 4080).astype(np.uint16)
    hc = np.clip(16 * bigc[8:8 + H // 2, 16:16 + W] + rng.integers(-8, 8, cs), 0, 4080).astype(np.uint16)
    out["quadrants"] = (noisy(y), noisy(uv), hy, huv(hc))
    # noise against a noise history: vectors of every kind, costs near the top
    out["noise"] = (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, cs, dtype=np.uint8), noise16(rng, (H, W)), huv(noise16(rng, cs)))
    # a constant picture on its own history: every candidate costs nothing, the rank must yield the zero vector
    out["constant"] = (np.full((H, W), 100, np.uint8), np.full(cs, 90, np.uint8), np.full((H, W), 1600, np.uint16), huv(np.full(cs, 1440, np.uint16)))
    # 0 <-> 255 against histories of 0 and 4080: the largest costs, the sums at their limits
    flip = lambda shape: rng.choice(np.array([0, 255], np.uint8), shape)
    flip16 = lambda shape: rng.choice(np.array([0, 4080], np.uint16), shape)
    out["flips"] = (flip((H, W)), flip(cs), flip16((H, W)), huv(flip16(cs)))
    out["extremes"] = (np.full((H, W), 255, np.uint8), np.zeros(cs, np.uint8), np.zeros((H, W), np.uint16), huv(np.full(cs, 4080, np.uint16)))
    if luma and chroma:  # the luma filtered with compensation beside a chroma that primes
        out["chroma-primes"] = out["quadrants"][:3] + (None,)
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("r", RANGES)
def test_stage_search_and_compensated_filter_match_numpy(E, size, r):
    vw, vh, W, H = size
    e = E.Encoder(vw, vh, fixed_qp=30)
    assert (e.mbw * 16, e.mbh * 16) == (W, H)
    found = set()
    for luma, chroma in STRENGTHS:
        d = dict(luma=luma, chroma=chroma)
        for name, (y, uv, hy, huv) in contents(vw, vh, W, H, r, luma, chroma, 1000 * vw + 100 * r + luma + chroma).items():
            ref = M.step(y, uv, hy, huv, luma, chroma, r, visible=(vw, vh), vectors=True)
            vec, m = e.stage_denoise_search(d, r, y, hy)
            assert np.array_equal(vec, ref[4]) and np.array_equal(m, ref[5]), (d, name, "search", np.argwhere(vec != ref[4])[:4], np.argwhere(m != ref[5])[:4])
            got = e.stage_denoise_mc(d, r, y, uv, hy, huv)
            for g, w, what in zip(got, ref, ("y", "uv", "hist_y", "hist_uv", "vec", "M")):
                equal_or_none(g, w, (d, name, what))
            assert got[2].max() <= 4080 and (got[3] is None or got[3].max() <= 4080)
            if name == "constant":
                assert not vec.any() and not m.any()
            if name in ("quadrants", "noise"):
                found |= {(int(a), int(b)) for a, b in vec.reshape(-1, 2)}
                if luma and name == "quadrants":
                    assert not np.array_equal(got[0][:vh, :vw], y[:vh, :vw])  # (it did filter)
    # the cases do what they are there for: vectors at the corner of the range and with both components odd were chosen
    assert any(abs(a) == r and abs(b) == r for a, b in found) and any(a & 1 and b & 1 for a, b in found)
    assert e.debug_denoise_bytes() == 0  # (the stage's buffers are its own)
    e.close()


def test_stage_range_0_is_the_plain_stage_and_values_outside_are_refused(E):
    e = E.Encoder(64, 48, fixed_qp=30)
    rng = np.random.default_rng(7)
    y, uv = rng.integers(0, 256, (48, 64), dtype=np.uint8), rng.integers(0, 256, (24, 64), dtype=np.uint8)
    hy, huv = noise16(rng, (48, 64)), noise16(rng, (24, 64))
    got = e.stage_denoise_mc(dict(luma=8, chroma=8), 0, y, uv, hy, huv)
    for g, w in zip(got[:4], e.stage_denoise(dict(luma=8, chroma=8), y, uv, hy, huv)):
        assert np.array_equal(g, w)
    assert not got[4].any() and not got[5].any()
    got = e.stage_denoise_mc(dict(luma=8, chroma=8), 8, y, uv)  # priming: no search
    for g, w in zip(got[:4], D.step(y, uv, None, None, 8, 8)):
        assert np.array_equal(g, w)
    assert not got[4].any()
    for bad in (-1, 17):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.stage_denoise_mc(dict(luma=8), bad, y, uv, hy)
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.set_denoise_motion(bad)
    for bad in (0, 17):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.stage_denoise_search(dict(luma=8), bad, y, hy)
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        e.stage_denoise_search({}, 4, y, hy)
    assert e.get_denoise_motion() == 0
    e.set_denoise_motion(16)
    e.set_denoise(luma=4)  # (the strengths' setter leaves the range alone)
    assert e.get_denoise_motion() == 16 and e.get_denoise() == dict(luma=4, chroma=0)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.last_denoise_motion()
    e.close()


# ---- streams
def moving_clip(w, h, n, seed, sigma=3.0, step=(3, -2)):
    """a texture that moves by `step` a picture, plus seeded Gaussian noise: visible NV12 pictures"""
    rng = np.random.default_rng(seed)
    big = np.kron(rng.integers(40, 216, ((h + 96) // 4, (w + 96) // 4)), np.ones((4, 4), np.int64))
    bigc = np.kron(rng.integers(90, 166, ((h + 96) // 4, (w + 96) // 4, 2)), np.ones((2, 2, 1), np.int64))
    noisy = lambda p: np.clip(np.rint(p + sigma * rng.standard_normal(p.shape)), 0, 255).astype(np.uint8)
    out = []
    for i in range(n):
        ox, oy = 48 - step[0] * i, 48 - step[1] * i
        c = bigc[oy // 2:oy // 2 + h // 2, ox // 2:ox // 2 + w // 2].reshape(h // 2, w)
        out.append((noisy(big[oy:oy + h, ox:ox + w]), noisy(c)))
    return out


def mc_bytes(W, H, chroma=True):
    """what a handle holds once a picture was filtered with a range: both histories twice, a word per block"""
    return 2 * (2 * W * H + (W * H if chroma else 0)) + W * H // 16


def test_a_stream_follows_the_chain_through_range_and_strength_changes(E):
    w, h, depth = 64, 48, 2
    pics = moving_clip(w, h, 8, 41)
    strengths = [(8, 8), (8, 8), (8, 8), (16, 4), (16, 4), (0, 0), (8, 8), (8, 8)]  # changed with the history kept; off; 0 -> 8 primes again
    ranges = [0, 0, 8, 8, 0, 0, 4, 4]  # 0 -> 8 -> 0 -> 4: in place, compensated into the other buffer, in place on that one, ...
    cp = coded(pics, w, h)
    ref = M.chain(cp, strengths, ranges)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(luma=8, chroma=8, motion=0))
    seen = []

    def check():
        e.collect()
        i = len(seen)
        same(sources(e, E), ref[i])
        assert e.last_denoise() == dict(luma=strengths[i][0], chroma=strengths[i][1]) and e.last_denoise_motion() == ranges[i]
        seen.append(i)
    for i in range(8):
        e.set_denoise(luma=strengths[i][0], chroma=strengths[i][1])
        e.set_denoise_motion(ranges[i])
        e.submit(*pics[i], pts=i)
        if e.pending > depth:
            check()
    while e.pending:
        check()
    assert seen == list(range(8))
    # the cases do what they are here for: the compensation changes the pictures it runs on, and everything behind them
    plain = D.chain(cp, strengths)
    assert all(np.array_equal(ref[i][0], plain[i][0]) for i in (0, 1, 5, 6)) and all(not np.array_equal(ref[i][0], plain[i][0]) for i in (2, 3, 4, 7))
    assert all(not np.array_equal(ref[i][1], plain[i][1]) for i in (2, 3, 7))
    assert e.debug_denoise_bytes() == mc_bytes(64, 48)
    e.close()


def test_a_range_without_strengths_is_off(E):
    w, h, depth = 64, 48, 2
    pics = moving_clip(w, h, 4, 42)
    never = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    ranged = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(motion=8))
    assert ranged.get_denoise_motion() == 8 and ranged.get_denoise() == dict(luma=0, chroma=0)
    ref = drain(never, depth, lambda i: never.submit(*pics[i], pts=i), 4)
    assert drain(ranged, depth, lambda i: ranged.submit(*pics[i], pts=i), 4) == ref
    assert ranged.debug_denoise_bytes() == 0 and ranged.last_denoise_motion() == 8 and never.last_denoise_motion() == 0
    never.close(); ranged.close()


def test_range_0_with_strengths_is_the_plain_filter_and_the_second_buffers_come_with_the_first_compensated_picture(E):
    w, h = 64, 48
    pics = moving_clip(w, h, 4, 43)
    cp = coded(pics, w, h)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, denoise=dict(luma=8, chroma=8))
    ref = D.chain(cp, [(8, 8)] * 4)
    for i in range(2):
        e.submit(*pics[i], pts=i)
        e.collect()
        same(sources(e, E), ref[i])
    assert e.debug_denoise_bytes() == 3 * 64 * 48
    e.close()
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, denoise=dict(luma=8, motion=8))
    assert e.debug_denoise_bytes() == 0
    e.submit(*pics[0], pts=0)
    e.collect()
    assert e.debug_denoise_bytes() == 2 * 64 * 48  # the first picture primes in place: no second buffer, no vectors
    e.submit(*pics[1], pts=1)
    e.collect()
    assert e.debug_denoise_bytes() == mc_bytes(64, 48, chroma=False)
    same(sources(e, E), M.chain(cp[:2], [(8, 0)] * 2, [8] * 2)[1])
    e.close()


def test_submit_device_never_filters_the_callers_planes(E):
    w, h, depth = 64, 48, 2
    pics = moving_clip(w, h, 3, 44)
    dev = [(dev_put(y), dev_put(uv)) for y, uv in pics]
    a = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(luma=8, chroma=8, motion=8))
    b = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    got = drain(a, depth, lambda i: a.submit_device(dev[i][0], w, dev[i][1], w, pts=i), 3)
    pre = M.chain(coded(pics, w, h), [(8, 8)] * 3, [8] * 3)
    assert got == drain(b, depth, lambda i: b.submit(pre[i][0], pre[i][1], pts=i), 3)
    assert not np.array_equal(pre[2][0], pics[2][0]) and not np.array_equal(pre[2][1], pics[2][1])
    for (dy, duv), (y, uv) in zip(dev, pics):
        assert np.array_equal(dev_get(dy, y.shape), y) and np.array_equal(dev_get(duv, uv.shape), uv)
    a.close(); b.close()
    for dy, duv in dev:
        device_free(dy); device_free(duv)


def test_hold_mode_repeats_the_picture_filtered_once(E):
    w, h, ns = 64, 48, 10 ** 9
    pics = moving_clip(w, h, 3, 45)
    ref = M.chain(coded(pics, w, h), [(8, 8)] * 3, [8] * 3)
    # 30 -> 60: the tick in between repeats the previous output picture; the history moved once per input picture
    e = E.Encoder(w, h, fps=60, gop=GOP, fixed_qp=QP, pipeline_depth=2, rate=(rateref.HOLD, ns, 2), denoise=dict(luma=8, chroma=8, motion=8))
    assert e.submit(*pics[0], pts=0) == 1
    e.collect()
    same(sources(e, E), ref[0])
    for i in (1, 2):
        assert e.submit(*pics[i], pts=i * ns // 30) == 2
        e.collect()
        same(sources(e, E), ref[i - 1])
        assert e.last_denoise_motion() == 8  # (the tick's slot carries the range too)
        e.collect()
        same(sources(e, E), ref[i])
    assert e.rate_stats()["repeated"] == 2 and not np.array_equal(ref[2][0], coded(pics, w, h)[2][0])
    e.close()


def test_a_recovery_enqueues_again_without_touching_the_history(E):
    """mi355enc_debug_trip_wait once, three pictures in flight: they come back through recover(), which encodes their filtered surfaces again; the step does not
    run again, so the pictures behind it are the chain's"""
    w, h, n, depth = 208, 124, 8, 2  # (no block row wholly in the margin: a priming picture leaves such rows as the input path made them)
    pics = moving_clip(w, h, n, 46)
    ref = M.chain(coded(pics, w, h), [(8, 8)] * n, [8] * n)
    e = E.Encoder(w, h, gop=40, fixed_qp=QP, pipeline_depth=depth, exclusive=True, denoise=dict(luma=8, chroma=8, motion=8))
    seen, keys = [], []

    def check():
        keys.append(bool(e.collect()[1]))
        same(sources(e, E), ref[len(seen)])
        seen.append(1)
    for i in range(n):
        if i == 4:
            e.debug_trip_wait(12)
        e.submit(*pics[i], pts=i)
        if e.pending > depth:
            check()
    while e.pending:
        check()
    assert len(seen) == n and e.stats().recoveries == 1 and sum(keys) == 2
    assert e.debug_denoise_bytes() == mc_bytes(208, 128)
    e.close()


def test_a_compensated_stream_decodes_to_the_devices_reconstruction(E, oracle):
    w, h, depth, n = 64, 44, 2, 6  # (the height ends inside a block row)
    pics = moving_clip(w, h, n, 47)
    ref = M.chain(coded(pics, w, h), [(8, 8)] * n, [8] * n)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(luma=8, chroma=8, motion=8))
    plain = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, denoise=dict(luma=8, chroma=8))
    got = drain(e, depth, lambda i: e.submit(*pics[i], pts=i), n)
    same(sources(e, E), ref[n - 1])
    dec = oracle.Decoder()
    for au, _ in got:
        dy, duv = dec.decode(au)
    assert np.array_equal(dy, e.fetch(E.FETCH_RECON_Y)) and np.array_equal(duv, e.fetch(E.FETCH_RECON_UV))
    other = drain(plain, depth, lambda i: plain.submit(*pics[i], pts=i), n)
    assert got[0] == other[0] and got[1:] != other[1:]  # the first picture primes: the same access unit
    print("bytes of the P pictures: compensated %d, plain filter %d" % (sum(len(a) for a, _ in got[1:]), sum(len(a) for a, _ in other[1:])))
    e.close(); plain.close()


def test_a_stream_behind_a_timed_launch_primes(E):
    """mi355enc_time_stage 27 / 28 work on the handle's own histories; the stream that follows must not filter against what they left"""
    w, h = 64, 48
    pics = moving_clip(w, h, 3, 48)
    ref = M.chain(coded(pics, w, h), [(8, 8)] * 3, [8] * 3)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, denoise=dict(luma=8, chroma=8))
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):  # (no range set)
        e.time_stage(E.STAGE_DENOISE_SEARCH, 1)
    e.set_denoise_motion(8)
    e.stage_denoise({}, *coded(moving_clip(w, h, 1, 49), w, h)[0])  # slot 0 holds a picture near the stream's: a history of it would filter
    assert e.time_stage(E.STAGE_DENOISE_SEARCH, 2) > 0 and e.time_stage(E.STAGE_DENOISE_MC, 3) > 0 and e.time_stage(E.STAGE_DENOISE, 1) > 0
    for i in range(3):
        e.submit(*pics[i], pts=i)
        e.collect()
        same(sources(e, E), ref[i])
    assert np.array_equal(ref[0][0], coded(pics, w, h)[0][0])
    e.close()
