"""MJPEG input on the GPU: the JPEG launch against tests/jpegref.py bit for bit -- whole pictures of every sampling, the
kernel alone on made-up coefficients (the wrap-around rule included) -- and whole streams against the streams of the planar pictures the
reference decodes."""
import glob
import os
import zlib

import numpy as np
import pytest

from tests import jpegref as J

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg", "*.jpg")))
SHAPES = [(16, 16, 0), (40, 24, 0), (72, 40, 2)]
SAMPLINGS = ["grey", "420", "422", "444"]


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _check_picture(E, data):
    hdr = J.parse(data)
    w, h = hdr["width"], hdr["height"]
    fmt, planes = J.decode(data)
    want = J.surfaces(fmt, planes, w, h)
    e = E.Encoder(w, h, fixed_qp=30)
    got = e.stage_jpeg(data)
    assert same(got, want)
    assert same(e.stage_csc(fmt, planes), got)  # ... which is the conversion stage's answer for the planar picture
    e.close()


@pytest.mark.parametrize("w,h,dri", SHAPES)
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_stage_jpeg_equals_the_reference_surfaces(E, sampling, w, h, dri):
    for seed, qts in ((1, (J.Q_LUMA, J.Q_CHROMA)), (2, (J.scaled_q(J.Q_LUMA, 10), J.scaled_q(J.Q_CHROMA, 10)))):
        data, _ = J.write_jpeg(J.subsample(*J.picture(w, h, seed, noise=60), sampling), sampling, qts=qts, dri=dri, dht=seed == 1)
        _check_picture(E, data)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_stage_jpeg_on_real_encoder_files(E, path):
    _check_picture(E, open(path, "rb").read())


def _made_up(kind, lay, rng):
    """coefficient blocks per component and the quantisation tables for one kind of made-up input"""
    qt = np.ones((3, 64), np.uint16)
    if kind == "dc":
        co = [np.zeros((bh, bw, 8, 8), np.int16) for bw, bh in lay]
        for c in co:
            c[..., 0, 0] = rng.integers(-1024, 1024, c.shape[:2])
        qt[:] = rng.integers(1, 17, (3, 64))
    elif kind == "single":  # one coefficient per block: position (block index mod 64), value +-1, +-1023 in turn
        co = [np.zeros((bh, bw, 64), np.int16) for bw, bh in lay]
        n = 0
        for c in co:
            for by in range(c.shape[0]):
                for bx in range(c.shape[1]):
                    c[by, bx, n % 64] = (1, -1, 1023, -1023)[(n // 64) % 4]
                    n += 1
        assert n >= 256  # every position with every value
        co = [c.reshape(c.shape[0], c.shape[1], 8, 8) for c in co]
        qt[:] = rng.integers(1, 4, (3, 64))
    elif kind == "legal":
        co = [rng.integers(-1023, 1024, (bh, bw, 8, 8)).astype(np.int16) // rng.integers(1, 64, (bh, bw, 1, 1)).astype(np.int16) for bw, bh in lay]
        qt[:] = rng.integers(1, 256, (3, 64))
    else:  # the whole int16 range with quantiser 255: products and sums leave 32 bits
        co = [rng.integers(-32768, 32768, (bh, bw, 8, 8)).astype(np.int16) for bw, bh in lay]
        qt[:] = 255
    return co, qt


@pytest.mark.parametrize("kind", ["dc", "single", "legal", "wrap"])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_stage_jpeg_blocks_equals_the_reference_idct(E, sampling, kind):
    w, h = (136, 128) if kind == "single" else (72, 40)  # (136 x 128: 272 luma blocks or more; several workgroups, a partial group of eight at the end of a row)
    nc, hs, vs = J.SAMPLING[sampling]
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    lay = [(mcux * (1 if c else hs), mcuy * (1 if c else vs)) for c in range(nc)]
    rng = np.random.default_rng(zlib.crc32((sampling + kind).encode()))
    co, qt = _made_up(kind, lay, rng)
    if kind == "wrap":  # (the case pins the wrap-around rule only if 32 bits are in fact left)
        assert int(np.abs(co[0].astype(np.int64)).max()) * 255 * 15137 > 2 ** 31
    fmt, planes = J.planar(J.planes_from_coefs(co, qt, w, h, hs, vs), w, h, hs, vs)
    e = E.Encoder(w, h, fixed_qp=30)
    got = e.stage_jpeg_blocks(hs, vs, nc, co, qt)
    assert same(got, J.surfaces(fmt, planes, w, h))
    e.close()


def drain(e, depth, feed, n):
    aus = []
    for i in range(n):
        feed(i)
        if e.pending > depth:
            aus.append(e.collect()[:2])
    while e.pending:
        aus.append(e.collect()[:2])
    return aus


def _clip(w, h, n, sampling):
    """n JPEG pictures of a moving scene and the planar pictures the reference decodes from them"""
    out = []
    for i in range(n):
        y, u, v = J.picture(w + 16, h, 3)
        data, _ = J.write_jpeg(J.subsample(*[np.ascontiguousarray(p[:, 2 * i:2 * i + w]) for p in (y, u, v)], sampling), sampling, dri=3 if i & 1 else 0, dht=i != 2)
        out.append((data,) + J.decode(data))
    return out


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("variant", ["plain", "overlay", "scaled"])
def test_jpeg_stream_equals_the_stream_of_the_decoded_pictures(E, oracle, variant, depth):
    w, h, n = 64, 48, 6
    iw, ih = (128, 96) if variant == "scaled" else (w, h)
    kw = dict(gop=4, fixed_qp=28, pipeline_depth=depth)
    if variant == "scaled":
        kw["input_size"] = (iw, ih)
    for sampling in ("422", "420") if variant == "plain" else ("422",):
        clip = _clip(iw, ih, n, sampling)
        a, b = E.Encoder(w, h, **kw), E.Encoder(w, h, **kw)
        if variant == "overlay":
            for e in (a, b):
                e.set_overlay_text("cam 1\n12.5 Mb/s")
        got = drain(a, depth, lambda i: a.submit_jpeg(clip[i][0], pts=i), n)
        ref = drain(b, depth, lambda i: b.submit_fmt(clip[i][1], clip[i][2], pts=i), n)
        assert got == ref and [k for _, k in got] == [i % 4 == 0 for i in range(n)]
        dec = oracle.Decoder()
        for au, _ in got:
            y, uv = dec.decode(au)
        assert np.array_equal(y, a.fetch(E.FETCH_RECON_Y)) and np.array_equal(uv, a.fetch(E.FETCH_RECON_UV))
        a.close(); b.close()


@pytest.mark.parametrize("depth", [0, 2])
def test_a_corrupt_picture_between_good_ones_leaves_no_trace(E, depth):
    w, h, n = 64, 48, 6
    clip = _clip(w, h, n, "422")
    kw = dict(gop=4, fixed_qp=28, pipeline_depth=depth)
    a, b = E.Encoder(w, h, **kw), E.Encoder(w, h, **kw)
    bad = clip[3][0][:len(clip[3][0]) // 2]  # the data ends before the last MCU
    refused = bytearray(clip[3][0])
    refused[refused.index(b"\xff\xc0") + 1] = 0xC2  # progressive

    def feed(i):
        if i == 3:
            for data in (bad, bytes(refused), b""):
                before = a.pending
                with pytest.raises(E.EncoderError, match=r"\(-1\)"):
                    a.submit_jpeg(data, pts=99)
                assert a.pending == before
        a.submit_jpeg(clip[i][0], pts=i)
    got = drain(a, depth, feed, n)
    ref = drain(b, depth, lambda i: b.submit_jpeg(clip[i][0], pts=i), n)
    assert got == ref and len(got) == n
    a.close(); b.close()


def test_size_mismatch_and_odd_dimensions_are_refused(E):
    e = E.Encoder(64, 48, fixed_qp=30)
    ok, _ = J.write_jpeg(J.subsample(*J.picture(64, 48, 1), "420"), "420")
    e.submit_jpeg(ok)
    e.collect()
    for w, h in ((48, 64), (64, 32), (80, 48), (63, 48), (64, 47)):
        data, _ = J.write_jpeg(J.subsample(*J.picture(w + (w & 1), h + (h & 1), 1), "444"), "444")
        if (w | h) & 1:  # the same picture, announced one sample smaller
            co = J.quantise(J.subsample(*J.picture(w + (w & 1), h + (h & 1), 1), "444"), "444", (J.Q_LUMA, J.Q_CHROMA))
            data = J.encode_coefs(co, w, h, "444")
            assert E.jpeg_info(data).width == w and E.jpeg_info(data).height == h
        for call in (e.submit_jpeg, e.stage_jpeg):
            with pytest.raises(E.EncoderError, match=r"\(-1\)"):
                call(data)
        assert e.pending == 0
    odd = E.Encoder(64, 48, fixed_qp=30, input_size=(128, 96))
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        odd.submit_jpeg(ok)  # the input size is what counts, not the coded size
    e.close(); odd.close()
