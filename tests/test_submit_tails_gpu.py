"""GPU: every submit entry point ends in the same tail -- image layers, then the text, then the upload event, then the stream schedule.  The exits that no
other file feeds with an image layer AND a text: MJPEG input, the scaled, the oriented and the copy + pad branch of submit_device, and pinned host input.  Each
one's stream is byte for byte the stream of a second encoder with the same settings that is fed the same visible pictures from contiguous pageable memory
through submit(), the exit tests/test_image_gpu.py::test_stream_with_a_text_overlay_on_top pins against the references."""
import numpy as np
import pytest

from tests.inputref import device_planes
from tests.test_jpeg_gpu import _clip as jpeg_clip
from tests.test_scale_gpu import clip

pytestmark = pytest.mark.gpu

N = 5
TEXT = "tail 0123"


def _encoder(E, w, h, **kw):
    e = E.Encoder(w, h, gop=4, fixed_qp=30, scenecut=False, pipeline_depth=2, **kw)
    e.set_overlay_text(TEXT)
    return e


def _run(e, feed):
    """-> [(au, key)]; the image moves with every picture, three pictures in flight; every picture reports the layer and the text it carried"""
    rgba = np.random.default_rng(9).integers(0, 256, (12, 20, 4), dtype=np.uint8)
    out = []

    def take(k):
        out.append(e.collect()[:2])
        assert e.last_image(0) == (20, 12, 6 + 3 * k, 4 + 2 * k, 200, 1) and e.last_overlay() == TEXT.encode(), k
    for i in range(N):
        if i == 0:
            e.set_image(0, rgba, 6, 4, 200)
        else:
            e.set_image_place(0, 6 + 3 * i, 4 + 2 * i, 200)
        feed(i)
        if e.pending > 2:
            take(len(out))
    while e.pending:
        take(len(out))
    return out


def _from_pageable(E, w, h, pics, **kw):
    """the second encoder: the same settings, the pictures through submit() from contiguous pageable memory"""
    e = _encoder(E, w, h, **kw)
    pics = [(np.ascontiguousarray(y), np.ascontiguousarray(uv)) for y, uv in pics]
    out = _run(e, lambda i: e.submit(*pics[i], pts=i))
    assert e.stats().pinned_inputs == 0
    e.close()
    return out


def _same(got, ref):
    assert len(got) == len(ref) == N and [k for _, k in got] == [i % 4 == 0 for i in range(N)]
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (i, len(g[0]), len(r[0]))


def test_jpeg_exit(E):
    w, h = 64, 48
    datas = [c[0] for c in jpeg_clip(w, h, N, "422")]
    d = E.Encoder(w, h, fixed_qp=30)
    pics = [d.stage_jpeg(data) for data in datas]  # (the decode itself is pinned by tests/test_jpeg_gpu.py)
    d.close()
    ref = _from_pageable(E, w, h, [(y[:h, :w], uv[:h // 2, :w]) for y, uv in pics])
    e = _encoder(E, w, h)
    got = _run(e, lambda i: e.submit_jpeg(datas[i], pts=i))
    e.close()
    _same(got, ref)


@pytest.mark.parametrize("case", ["scaled", "oriented", "pad"])
def test_device_exit(E, case):
    """scaled: 128 x 96 -> 64 x 48, read where the planes lie (odd address and stride); oriented: 48 x 64 turned right into 64 x 48, likewise; pad: 72 x 40,
    aligned planes at a stride of 16 n -- the width alone (and the decorations) send it through the copy and the margin launch"""
    (w, h), (iw, ih), kw, stride, off = {
        "scaled": ((64, 48), (128, 96), dict(input_size=(128, 96)), 128 + 5, 3),
        "oriented": ((64, 48), (48, 64), dict(orientation="90r"), 48 + 5, 3),
        "pad": ((72, 40), (72, 40), {}, 80, 0),
    }[case]
    pics = clip(iw, ih, N)
    ref = _from_pageable(E, w, h, pics, **kw)
    dev = [device_planes(E, [y, uv], [ih, ih // 2], [iw, iw], stride, off) for y, uv in pics]
    e = _encoder(E, w, h, **kw)
    got = _run(e, lambda i: e.submit_device(dev[i][2][0], stride, dev[i][2][1], stride, pts=i))
    e.close()
    for hip, buf, _ in dev:
        hip.hipFree(buf)
    _same(got, ref)


def test_pinned_host_exit(E):
    w, h = 64, 48
    pics = clip(w, h, N)
    ref = _from_pageable(E, w, h, pics)
    per = w * h * 3 // 2
    buf = E.PinnedBuffer(N * per)
    views = []
    for i, (y, uv) in enumerate(pics):
        a = buf.array[i * per:(i + 1) * per]
        a[:w * h], a[w * h:] = y.ravel(), uv.ravel()
        views.append((a[:w * h].reshape(h, w), a[w * h:].reshape(h // 2, w)))
    e = _encoder(E, w, h)
    got = _run(e, lambda i: e.submit(*views[i], pts=i))
    assert e.stats().pinned_inputs == N
    e.close()
    del views, a
    buf.free()
    _same(got, ref)
