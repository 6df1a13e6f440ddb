"""JPEG stills on the device: the kernel against tests/snapref.py bit for bit, on planes at any address and stride, and the stills a
running stream yields -- the coded source with text, an image layer and an orientation in it, the deblocked reconstruction at every picture type and pipeline
depth -- without one byte of the access units changing.  Everything is compared with ==."""
import numpy as np
import pytest

from tests import imageref, inputref, jpegref, orientref, overlayref, snapref

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (72, 40), (50, 34), (136, 72)]  # one MCU; a half MCU; width = 2 (mod 16) and a row remainder; more than one task per block row and several workgroups
KINDS = ("textured", "noise", "saturated")


@pytest.fixture
def enc(E):
    """a handle for the single-stage calls (they take planes of any size).  Per test, and the stream tests open theirs only after their streams are closed:
    an encoder overlaps its kernels on the device only while it is the process's only one"""
    e = E.Encoder(64, 48, fixed_qp=30)
    yield e
    e.close()


def _same(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("w,h", SIZES)
def test_stage_equals_the_rule_bit_for_bit(E, enc, w, h):
    """6: every size x reduction x quality x content.  72x40 by 8 is a 9x5 still with 5x3 chroma: odd sizes, blocks that lie wholly in the MCU padding."""
    for kind in KINDS:
        y, uv = snapref.picture(w, h, kind)
        for s in (1, 2, 4, 8):
            planes = snapref.reduced_planes(y, uv, s)
            for q in (1, 75, 100):
                want, qt, _ = snapref.levels_of_planes(planes, q)
                got, gqt = enc.stage_snapshot_blocks(y, uv, reduce=s, quality=q)
                assert np.array_equal(gqt, qt), (kind, s, q)
                assert _same(got, want), (kind, s, q, [int(np.abs(g.astype(int) - x).max()) for g, x in zip(got, want)])
            # the whole file: the per-block hints the kernel leaves must not change what the writer codes
            oh, ow = planes[0].shape
            assert enc.stage_snapshot(y, uv, reduce=s, quality=75) == snapref.write(*snapref.levels_of_planes(planes, 75)[:2], ow, oh), (kind, s)


def test_saturated_content_at_quality_100_reaches_the_limits_and_no_further(enc):
    """levels within what baseline Huffman codes (|AC| <= 1023, DC differences within 11 bits), from the device"""
    y, uv = snapref.picture(136, 72, "saturated")
    got, _ = enc.stage_snapshot_blocks(y, uv, reduce=1, quality=100)
    for c in got:
        ac = c.reshape(-1, 64)[:, 1:]
        assert np.abs(ac).max() <= 1023 and np.abs(c[..., 0, 0].astype(int)).max() <= 1024
    assert max(int(np.abs(c.reshape(-1, 64)[:, 1:]).max()) for c in got) > 500  # the content does go near them


@pytest.mark.parametrize("w,h,s", [(72, 40, 1), (50, 34, 2), (136, 72, 4), (72, 40, 8)])
def test_device_planes_at_an_odd_address_and_stride(E, enc, w, h, s):
    """7: the _device form on planes at an odd base address and a stride that is no multiple of four, inside a container of seeded noise: the byte path, and
    nothing outside the visible picture reaches the result"""
    y, uv = snapref.picture(w, h, "noise", seed=3)
    stride = w + 7 if (w + 7) % 4 else w + 9
    assert stride % 4 and stride >= w
    buf, y_off, uv_off = inputref.container(y, uv, stride, layout="apart", seed=11, offset=1)
    d = inputref.device_container(buf)
    try:
        assert (d + y_off) % 2 == 1
        got, _ = enc.stage_snapshot_blocks_device(d + y_off, stride, d + uv_off, stride, w, h, reduce=s, quality=75)
        want, _, _ = snapref.levels(y, uv, s, 75)
        assert _same(got, want)
        # ... and on aligned planes in the same container (the dword path beside the same poison)
        buf2, y2, uv2 = inputref.container(y, uv, stride + (4 - stride % 4), layout="uv_first", seed=12, offset=0)
        d2 = inputref.device_container(buf2)
        try:
            got2, _ = enc.stage_snapshot_blocks_device(d2 + y2, stride + (4 - stride % 4), d2 + uv2, stride + (4 - stride % 4), w, h, reduce=s, quality=75)
            assert _same(got2, want)
        finally:
            inputref.device_free(d2)
    finally:
        inputref.device_free(d)


# ------------------------------------------------------------------------------------------------ stills of a running stream
def _clip(w, h, n, seed=5):
    rng = np.random.default_rng(seed)
    base_y, base_uv = snapref.picture(w, h, "textured", seed=seed)
    out = []
    for i in range(n):
        y = np.roll(base_y, 2 * i, axis=1).copy()
        y[4:12, 4 + i:12 + i] = rng.integers(0, 256, (8, 8))
        out.append((y, np.roll(base_uv, 2 * i, axis=1).copy()))
    return out


def _run(E, w, h, frames, depth, arm=(), what=0, reduce=2, quality=60, setup=None, exclusive=False, metrics=False, qp=30, drops=None):
    """the stream's access units, and {picture: (still bytes, info)} for the armed pictures; every still is taken right after its picture's collect"""
    e = E.Encoder(w, h, fixed_qp=qp, gop=8, pipeline_depth=depth, exclusive=exclusive)
    try:
        if metrics:
            e.set_quality_metrics(True)
        if setup:
            setup(e)
        aus, stills, quality_ints, pend = [], {}, [], []

        def collect():
            au = e.collect()[0]
            i = pend.pop(0)
            aus.append(au)
            if metrics:
                quality_ints.append(e.last_quality().ints())
            if i in arm:
                got = e.take_snapshot()
                assert got is not None, i
                assert got[1]["index"] == i and got[1]["pts"] == 100 + i, got[1]
                stills[i] = got
        for i, (y, uv) in enumerate(frames):
            if drops is not None:
                e.set_fixed_drop(drops[i])
            if i in arm:
                e.request_snapshot(what=what, reduce=reduce, quality=quality)
            e.submit(y, uv, pts=100 + i)
            pend.append(i)
            if len(pend) > depth:
                collect()
        while pend:
            collect()
        return aus, stills, e.snapshot_bytes(), quality_ints
    finally:
        e.close()


@pytest.mark.parametrize("w,h", [(64, 48), (136, 72)])
@pytest.mark.parametrize("depth", [0, 2])
def test_source_stills_in_a_stream(E, w, h, depth):
    """8: with text, an image layer and an orientation set, the still of the coded source is the stage's still of the surface the references predict; the
    access units are those of the stream without any request; the handle that never asked holds nothing"""
    frames = _clip(h, w, 12)  # submitted pre-orientation: h x w, turned 90r into w x h
    rgba = np.random.default_rng(9).integers(0, 256, (12, 20, 4), dtype=np.uint8)

    def setup(e):
        e.set_orientation(E.ORIENT_90R)
        e.set_image(0, rgba, x=6, y=4, opacity=200)
        e.set_overlay_text("still 0123")

    arm = (0, 5, 11)
    plain, none, held0, _ = _run(E, w, h, frames, depth, setup=setup)
    aus, stills, held, _ = _run(E, w, h, frames, depth, arm=arm, what=0, reduce=2, quality=60, setup=setup)
    assert aus == plain and not none and held0 == 0 and held > 0
    enc = E.Encoder(64, 48, fixed_qp=30)
    for i in arm:
        y, uv = orientref.orient(*frames[i], E.ORIENT_90R)
        y, uv = imageref.blend(y, uv, [imageref.layer(rgba, 6, 4, 200)], imageref.coefficients(2, 0, w, h))
        y, uv = overlayref.draw(y, uv, "still 0123")
        want = enc.stage_snapshot(y, uv, reduce=2, quality=60)
        assert stills[i][0] == want, i
        assert (stills[i][1]["width"], stills[i][1]["height"], stills[i][1]["what"], stills[i][1]["quality"]) == (w // 2, h // 2, 0, 60)
    enc.close()


def _still_of_recon(e, E, w, h, s, q):
    """the rule applied to what mi355enc_fetch returns for the last collected picture"""
    ry, ruv = e.fetch(E.FETCH_RECON_Y)[:h, :w], e.fetch(E.FETCH_RECON_UV)[:h // 2, :w]
    return snapref.levels(ry, ruv, s, q)


DROPS = [0, 0, 0, 255, 0, 0]  # picture 3: one run of P_Skip macroblocks (it is its reference)


@pytest.mark.parametrize("w,h", [(64, 48), (136, 72)])
def test_decoded_stills_equal_the_fetched_reconstruction(E, w, h):
    """9, depth 0: the still of the reconstruction holds the levels the rule gives for mi355enc_fetch's planes -- for an IDR picture, a P picture and an all-skip picture"""
    frames = _clip(w, h, 6)
    e = E.Encoder(w, h, fixed_qp=32, gop=8, pipeline_depth=0)
    try:
        for i, (y, uv) in enumerate(frames):
            e.set_fixed_drop(DROPS[i])
            if i in (0, 2, 3):
                e.request_snapshot(what=E.SNAP_DECODED, reduce=1 if i != 2 else 2, quality=80)
            au, key = e.encode(y, uv, pts=i)
            if i in (0, 2, 3):
                assert key == (i == 0) and (e.last_drop == 255) == (i == 3)
                data, info = e.take_snapshot()
                want, qt, (ow, oh) = _still_of_recon(e, E, w, h, 1 if i != 2 else 2, 80)
                hdr, got, gqt = jpegref.entropy_decode(data)
                assert (hdr["width"], hdr["height"], info["index"], info["what"]) == (ow, oh, i, 1)
                assert np.array_equal(gqt[:2], qt) and _same(got, want), i
                assert data == snapref.write(want, qt, ow, oh)
    finally:
        e.close()


@pytest.mark.parametrize("metrics", [False, True])
def test_decoded_stills_with_three_pictures_in_flight(E, metrics):
    """9, depth 2 on a device of its own: three pictures are in flight and the ping-pong buffer a still reads is rewritten soon after -- the stills are the
    bytes of depth 0, the access units those of the stream without stills, and with quality metrics on (both launches behind the deblocking) those are unchanged"""
    w, h = 136, 72
    frames = _clip(w, h, 6) + _clip(w, h, 6, seed=6)
    drops = DROPS + DROPS
    arm = (0, 2, 3, 4, 7, 11)
    ref_aus, ref_stills, _, ref_q = _run(E, w, h, frames, 0, arm=arm, what=1, reduce=1, quality=70, metrics=metrics, qp=32, drops=drops)
    aus, stills, _, q = _run(E, w, h, frames, 2, arm=arm, what=1, reduce=1, quality=70, metrics=metrics, qp=32, drops=drops, exclusive=True)
    plain, _, held, plain_q = _run(E, w, h, frames, 2, metrics=metrics, qp=32, drops=drops, exclusive=True)
    assert held == 0 and aus == plain and q == plain_q
    assert sorted(stills) == sorted(ref_stills) == sorted(arm)
    for i in arm:
        assert stills[i][0] == ref_stills[i][0], i
    if metrics:
        assert len(q) == len(frames)


def test_call_order(E):
    """10"""
    w, h = 64, 48
    frames = _clip(w, h, 4)
    e = E.Encoder(w, h, fixed_qp=30, gop=8, pipeline_depth=1)
    try:
        with pytest.raises(E.EncoderError):
            e.request_snapshot(reduce=3)
        with pytest.raises(E.EncoderError):
            e.request_snapshot(quality=0)
        with pytest.raises(E.EncoderError):
            e.request_snapshot(what=2)
        assert e.take_snapshot() is None and e.snapshot_bytes() == 0
        e.request_snapshot(reduce=2, quality=50)
        e.request_snapshot(reduce=4, quality=90)          # replaces the first
        assert e.snapshot_bytes() == 0                    # (a request allocates nothing)
        e.submit(*frames[0], pts=7)
        assert e.take_snapshot() is None                  # not collected yet
        e.request_snapshot(reduce=1, quality=75)
        e.submit(*frames[1], pts=8)
        e.collect()
        a, info = e.take_snapshot()
        assert (info["index"], info["pts"], info["width"], info["height"], info["quality"]) == (0, 7, 16, 12, 90)
        assert e.take_snapshot()[0] == a                  # twice: the same bytes
        with pytest.raises(E.EncoderError) as ex:
            e.take_snapshot(cap=len(a) - 1)
        assert ex.value.need == len(a)
        with pytest.raises(E.EncoderError) as ex:
            e.take_snapshot(cap=0)
        assert ex.value.need == len(a)
        e.collect()                                       # picture 1's still replaces the one of picture 0
        b, info = e.take_snapshot()
        assert (info["index"], info["width"], info["quality"]) == (1, 64, 75) and b != a
        e.submit(*frames[2], pts=9)                       # no request: the ready still stays
        e.collect()
        assert e.take_snapshot()[0] == b
    finally:
        e.close()
    stage = E.Encoder(64, 48, fixed_qp=30)
    try:
        assert a == stage.stage_snapshot(*frames[0], reduce=4, quality=90) and b == stage.stage_snapshot(*frames[1], reduce=1, quality=75)
    finally:
        stage.close()


@pytest.mark.parametrize("depth,what", [(0, 0), (2, 1)])
def test_still_of_a_picture_that_is_encoded_again(E, depth, what):
    """10: a request that follows mi355enc_debug_trip_wait -- the armed picture comes back through the recovery path, launches its still again into the same
    block, and the still is that of the re-encoded picture"""
    w, h = 136, 72
    frames = _clip(w, h, 6)

    def run(trip):
        e = E.Encoder(w, h, fixed_qp=30, gop=8, pipeline_depth=depth, exclusive=True)
        try:
            stills, aus, pend = {}, [], []

            def collect():
                aus.append(e.collect()[0])
                if pend.pop(0) == 3:
                    stills[3] = e.take_snapshot()
            for i, (y, uv) in enumerate(frames):
                if i == 3:
                    if trip:
                        e.debug_trip_wait(12)
                    e.request_snapshot(what=what, reduce=2, quality=65)
                e.submit(y, uv, pts=i, force_idr=(i == 3 and not trip))
                pend.append(i)
                if len(pend) > depth:
                    collect()
            while pend:
                collect()
            return aus, stills, e.stats().recoveries
        finally:
            e.close()
    aus, stills, rec = run(True)
    ref_aus, ref_stills, ref_rec = run(False)  # the recovery starts with an IDR picture: the same stream with that picture forced
    assert (rec, ref_rec) == (1, 0) and aus == ref_aus
    assert stills[3] is not None and stills[3][0] == ref_stills[3][0] and stills[3][1]["index"] == 3
    if what == 0:
        stage = E.Encoder(64, 48, fixed_qp=30)
        try:
            assert stills[3][0] == stage.stage_snapshot(*frames[3], reduce=2, quality=65)
        finally:
            stage.close()
