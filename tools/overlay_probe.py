"""What the text overlay costs (profiles/overlay_price.md).

  python tools/overlay_probe.py kernel     the kernel alone: 200 single-stage calls per size, for a `rocprofv3 --kernel-trace --stats` run of its own
                                           (the stage call also copies the planes in and out: only the kernel's row of the statistics is of interest)
  python tools/overlay_probe.py stream     the 1080p IPPP stream at pipeline_depth 2, text off and on alternating in one process: device-resident
                                           pictures (with a text they are copied instead of read in place) and pictures in pinned host memory
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402
from ceracoder_amd import synth  # noqa: E402

LINE = "  b:  2048/ 1900 rtt:  40/ 38/ 45 bs:  12/ 10/ 14/ 11"  # the reference's 53-character statistics line


def kernel():
    for w, h in ((1920, 1080), (3840, 2160)):
        e = E.Encoder(w, h, fixed_qp=30)
        y, uv = np.full((e.mbh * 16, e.mbw * 16), 90, np.uint8), np.full((e.mbh * 8, e.mbw * 16), 128, np.uint8)
        for _ in range(200):
            e.stage_overlay(LINE, y, uv)  # default style: right, top, pads 16, automatic scale (2 at 1080p, 4 at 2160p)
        e.close()
        print("%dx%d: 200 launches" % (w, h))


def run(e, feed, n):
    t0 = time.perf_counter()
    for i in range(n):
        feed(i)
        if e.pending > 2:
            e.collect(copy=False)
    while e.pending:
        e.collect(copy=False)
    return n / (time.perf_counter() - t0)


def stream():
    import ctypes as C
    from tests.inputref import hip as hip_runtime
    w, h, n, uniq = 1920, 1080, 600, 16
    pics = list(synth.s2_frames(w, h, uniq))
    hip = hip_runtime()
    per = w * h * 3 // 2
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(per * uniq)) == 0
    pin = E.PinnedBuffer(per * uniq)
    for k, (y, uv) in enumerate(pics):
        pin.array[k * per:k * per + w * h] = y.reshape(-1)
        pin.array[k * per + w * h:(k + 1) * per] = uv.reshape(-1)
    assert hip.hipMemcpy(dev, C.c_void_p(pin.ptr), C.c_size_t(per * uniq), 1) == 0
    res = {}
    for rep in range(3):
        for path in ("device", "pinned"):
            for text in ("", LINE):
                e = E.Encoder(w, h, gop=60, fixed_qp=30, pipeline_depth=2, exclusive=True)
                e.set_overlay_text(text)
                if path == "device":
                    feed = lambda i: e.submit_device(dev.value + (i % uniq) * per, w, dev.value + (i % uniq) * per + w * h, w, pts=i)
                else:
                    def feed(i):
                        o = (i % uniq) * per
                        e.submit(pin.array[o:o + w * h].reshape(h, w), pin.array[o + w * h:o + per].reshape(h // 2, w), pts=i)
                run(e, feed, 60)
                res.setdefault((path, bool(text)), []).append(run(e, feed, n))
                e.close()
    for (path, on), v in sorted(res.items()):
        m = sum(v) / len(v)
        print("| %s | %s | %s | %.0f | %.0f | %.2f |" % (path, "on" if on else "off", " / ".join("%.0f" % x for x in v), m, max(v) - min(v), 1e6 / m))
    hip.hipFree(dev)
    pin.free()


if __name__ == "__main__":
    {"kernel": kernel, "stream": stream}[sys.argv[1]]()
