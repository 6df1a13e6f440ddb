"""HDR input tone-mapped to SDR on the device against tests/hdrref.py's restatement of the rule, bit for bit: the conversion launch alone in
the three 10-bit formats, on unaligned and aligned device planes, behind mi355enc_set_input_size, a whole stream, what a tone-mapping handle refuses, and that
a handle which never made the call is what it was."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import hdrref as H
from tests import scaleref as SR
from tests import yuvref as YR
from tests.spsref import sps_of
from tests.inputref import device_free
from tests.test_csc_formats_gpu import drain, same
from tests.test_yuv_convert_gpu import dev_get, dev_put

pytestmark = pytest.mark.gpu

JPEG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg", "q50_420_72x40.jpg")
FMTS = [H.FMT_P010, H.FMT_I420_10, H.FMT_V210]
IDS = ["P010", "I420_10", "v210"]
# 64 x 48: whole patches, the fast path.  50 x 34: a visible width that ends inside a patch and inside a v210 group, margin rows and columns.  16 x 16: one block.
SIZES = [(64, 48), (50, 34), (16, 16)]
COL = (0, 1, 1, 1)
_blocks = {}


def block(E, transfer, full=0, peak=0, target=0, out_matrix=1, out_full=0):
    """the exported parameter block, made once per parameter set and shared"""
    key = (transfer, full, peak, target, out_matrix, out_full)
    if key not in _blocks:
        _blocks[key] = E.hdr_tables(*key)
        _blocks[key].setflags(write=False)
    return _blocks[key]


def planes_of(fmt, w, h, seed, content="random", pad=0, offset=0):
    rng = np.random.default_rng(seed)
    planes = YR.random_planes(fmt, w, h, rng, pad=pad, offset=offset)  # every bit at random: P010's ignored low six, I420_10's high six, v210's bits 30 - 31
    if content == "zeros":
        for p in planes:
            p[:] = 0
    elif content == "ones":
        for p in planes:
            p[:] = 255
    elif content == "outside":  # codes below 64 and above 940 (and chroma far from grey) in every plane: the input clips
        y10 = np.where(rng.integers(0, 2, (h, w)) == 1, rng.integers(0, 64, (h, w)), rng.integers(941, 1024, (h, w)))
        c10 = [np.where(rng.integers(0, 2, (h // 2, w // 2)) == 1, rng.integers(0, 64, (h // 2, w // 2)), rng.integers(941, 1024, (h // 2, w // 2))) for _ in range(2)]
        if fmt == H.FMT_V210:
            planes = [YR.pack_v210(y10, np.repeat(c10[0], 2, 0), np.repeat(c10[1], 2, 0), rng)]
        else:
            sh = 6 if fmt == H.FMT_P010 else 0
            cc = [np.stack(c10, 2).reshape(h // 2, w)] if fmt == H.FMT_P010 else c10
            planes = [np.ascontiguousarray((p << sh).astype("<u2")).view(np.uint8).reshape(p.shape[0], -1) for p in [y10] + cc]
    return planes


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("transfer", [H.PQ, H.HLG], ids=["pq", "hlg"])
@pytest.mark.parametrize("fmt", FMTS, ids=IDS)
def test_stage_csc_tone_maps_bit_for_bit(E, fmt, transfer, w, h):
    e = E.Encoder(w, h, fixed_qp=30, colorimetry=COL, hdr_input=(transfer, 0, 0, 0))
    planes = [np.ascontiguousarray(p) for p in planes_of(fmt, w, h, fmt * 100 + w + transfer)]
    same(e.stage_csc(fmt, planes), H.tone_map_nv12(block(E, transfer), fmt, planes, w, h))
    e.close()


@pytest.mark.parametrize("content", ["zeros", "ones", "outside"])
@pytest.mark.parametrize("fmt", FMTS, ids=IDS)
def test_content_at_the_ends_of_the_code_range(E, fmt, content):
    w, h = 50, 34
    for transfer, full, target, col in ((H.PQ, 1, 100, (1, 1, 1, 6)), (H.HLG, 0, 400, (0, 6, 6, 5))):
        e = E.Encoder(w, h, fixed_qp=30, colorimetry=col, hdr_input=(transfer, full, 400, target))
        planes = [np.ascontiguousarray(p) for p in planes_of(fmt, w, h, 5 + fmt, content)]
        same(e.stage_csc(fmt, planes), H.tone_map_nv12(block(E, transfer, full, 400, target, col[3], col[0]), fmt, planes, w, h))
        e.close()


@pytest.mark.parametrize("w,h", [(64, 48), (50, 34)], ids=lambda v: str(v))
@pytest.mark.parametrize("fmt", FMTS, ids=IDS)
def test_device_planes_unaligned_and_aligned_give_the_same_bytes(E, fmt, w, h):
    """planes 2 bytes into their buffers at odd strides (the sample path), and 16-byte aligned (the fast path where the patch is whole)"""
    e = E.Encoder(w, h, fixed_qp=30, colorimetry=COL, hdr_input=(H.HLG, 0, 1000, 203))
    W, Hc = e.mbw * 16, e.mbh * 16
    tight = planes_of(fmt, w, h, 31 + fmt)
    want = H.tone_map_nv12(block(E, H.HLG, 0, 1000, 203), fmt, tight, w, h)
    got = []
    for pad, offset in ((0, 0), (1, 2)):  # stride: the row's bytes rounded up to 16, or that plus 1
        planes = []
        for p in tight:
            stride = (p.shape[1] + 15) // 16 * 16 + pad
            buf = np.zeros(offset + p.shape[0] * stride, np.uint8)
            v = np.lib.stride_tricks.as_strided(buf[offset:], p.shape, (stride, 1))
            v[:] = p
            planes.append((buf, stride))
        bufs = [dev_put(b) for b, _ in planes]
        oy, ouv = dev_put(np.zeros(Hc * W, np.uint8)), dev_put(np.zeros(Hc // 2 * W, np.uint8))
        e.stage_csc_device(fmt, [b + offset for b in bufs], [s for _, s in planes], oy, ouv)
        got.append((dev_get(oy, (Hc, W)), dev_get(ouv, (Hc // 2, W))))
        for d in bufs + [oy, ouv]:
            device_free(d)
    same(got[0], want)
    same(got[1], want)
    e.close()


@pytest.mark.parametrize("fmt", FMTS, ids=IDS)
def test_under_an_input_size_it_is_the_tone_map_then_the_nv12_scale(E, fmt):
    (iw, ih), (ow, oh) = (128, 96), (64, 48)
    e = E.Encoder(ow, oh, fixed_qp=30, colorimetry=COL, input_size=(iw, ih), hdr_input=(H.PQ, 0, 4000, 100))
    planes = [np.ascontiguousarray(p) for p in planes_of(fmt, iw, ih, 77 + fmt)]
    cy, cuv = H.tone_map_nv12(block(E, H.PQ, 0, 4000, 100), fmt, planes, iw, ih)
    same(e.stage_csc(fmt, planes), SR.to_nv12(SR.FMT_NV12, [cy[:ih, :iw], cuv[:ih // 2, :iw]], iw, ih, ow, oh))
    e.close()


def hdr_clip(w, h, n, seed):
    """P010 pictures that move: a PQ ramp with coloured noise on it"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        y = (np.add.outer(np.arange(h) * 5, np.arange(w) * 9) + 40 * i) % 900 + 64 + rng.integers(0, 24, (h, w))
        c = 512 + rng.integers(-160, 160, (h // 2, w))
        out.append([np.ascontiguousarray((p.astype(np.int64) << 6).astype("<u2")).view(np.uint8).reshape(p.shape[0], -1) for p in (y, c)])
    return out


@pytest.mark.parametrize("depth", [0, 2])
def test_stream_equals_the_stream_of_the_tone_mapped_pictures(E, depth):
    w, h, n, col = 64, 48, 5, (0, 6, 6, 6)
    clip = hdr_clip(w, h, n, 3)
    a = E.Encoder(w, h, gop=4, fixed_qp=28, pipeline_depth=depth, colorimetry=col, hdr_input=(H.PQ, 0, 1000, 203))
    b = E.Encoder(w, h, gop=4, fixed_qp=28, pipeline_depth=depth, colorimetry=col)
    ref = [H.tone_map_nv12(block(E, H.PQ, 0, 1000, 203, 6, 0), H.FMT_P010, p, w, h) for p in clip]
    got = drain(a, depth, lambda i: a.submit_fmt(E.FMT_P010, clip[i], pts=i), n)
    assert got == drain(b, depth, lambda i: b.submit(ref[i][0][:h, :w], ref[i][1][:h // 2, :w], pts=i), n)
    assert [k for _, k in got] == [i % 4 == 0 for i in range(n)]
    assert sps_of(got[0][0])[0]["colorimetry"] == col
    a.close(); b.close()


def test_a_tone_mapping_handle_refuses_every_other_input(E):
    w, h = 64, 48
    y, uv = np.full((h, w), 90, np.uint8), np.full((h // 2, w), 128, np.uint8)
    p010 = hdr_clip(w, h, 1, 9)[0]
    e = E.Encoder(w, h, fixed_qp=28)
    for bad in ((1, 0, 0, 0), (17, 0, 0, 0), (16, 2, 0, 0), (16, 0, 399, 0), (16, 0, 10001, 0), (18, 0, 2001, 0), (16, 0, 0, 99), (16, 0, 0, 401), (16, -1, 0, 0)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.set_hdr_input(*bad)
    e.set_hdr_input(E.HDR_PQ)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.set_input_colorimetry(0, 9)  # one meaning of the input per handle
    dy, duv = dev_put(y), dev_put(uv)
    u, v = np.ascontiguousarray(uv[:, 0::2]), np.ascontiguousarray(uv[:, 1::2])
    refused = [lambda: e.submit(y, uv), lambda: e.submit_fmt(E.FMT_NV12, [y, uv]), lambda: e.submit_fmt(E.FMT_I420, [y, u, v]), lambda: e.submit_fmt(E.FMT_YV12, [y, v, u]),
               lambda: e.submit_fmt(E.FMT_YUY2, [np.zeros((h, 2 * w), np.uint8)]), lambda: e.submit_fmt(E.FMT_Y42B, [y, np.repeat(u, 2, 0), np.repeat(v, 2, 0)]),
               lambda: e.submit_fmt(E.FMT_BGRX, [np.zeros((h, 4 * w), np.uint8)]), lambda: e.submit_fmt(E.FMT_RGB, [np.zeros((h, 3 * w), np.uint8)]),
               lambda: e.submit_fmt(E.FMT_GRAY8, [y]), lambda: e.submit_jpeg(open(JPEG, "rb").read()), lambda: e.submit_device(dy, w, duv, w),
               lambda: e.stage_csc(E.FMT_I420, [y, u, v])]
    for submit in refused:
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            submit()
        assert e.pending == 0
    e.set_colorimetry(0, 9, 16, 9)  # an output matrix the tone map does not convert to
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        e.submit_fmt(E.FMT_P010, p010)
    assert e.pending == 0
    e.set_colorimetry(*COL)
    e.submit_fmt(E.FMT_P010, p010)
    au, key = e.collect()[:2]
    assert key and sps_of(au)[0]["colorimetry"] == COL
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.set_hdr_input(E.HDR_HLG)  # after the first submit
    e.close()
    device_free(dy); device_free(duv)
    e = E.Encoder(w, h, fixed_qp=28, input_colorimetry=(0, 9))
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.set_hdr_input(E.HDR_PQ)  # ... in the other order
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.time_stage(E.STAGE_HDR_P010, 1)  # no tone map on this handle
    e.close()


def test_time_stage_runs_the_launch(E):
    e = E.Encoder(64, 48, fixed_qp=28, colorimetry=COL, hdr_input=(H.HLG, 0, 0, 0))
    for stage in (E.STAGE_HDR_P010, E.STAGE_HDR_I420_10, E.STAGE_HDR_V210, E.STAGE_DEEP_P010):
        assert 0 < e.time_stage(stage, 3) < 50
    e.close()


def test_a_handle_that_never_made_the_call_is_what_it_was(E):
    w, h, n = 64, 48, 5
    clip = hdr_clip(w, h, n, 4)
    a, b = E.Encoder(w, h, gop=4, fixed_qp=28), E.Encoder(w, h, gop=4, fixed_qp=28)
    ref = [YR.to_nv12(YR.FMT_P010, p, w, h) for p in clip]
    same(a.stage_csc(E.FMT_P010, clip[0]), ref[0])
    got = drain(a, 0, lambda i: a.submit_fmt(E.FMT_P010, clip[i], pts=i), n)
    assert got == drain(b, 0, lambda i: b.submit(ref[i][0][:h, :w], ref[i][1][:h // 2, :w], pts=i), n)
    a.close(); b.close()
