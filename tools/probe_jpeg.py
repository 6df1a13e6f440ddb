#!/usr/bin/env python3
"""What MJPEG input costs: python tools/probe_jpeg.py [--iters N] [--out profiles/jpeg_input_price.md]

Per size (720p, 1080p): the JPEG launch for a 4:2:2 picture (mi355enc_time_stage stage 12, HIP events around back-to-back launches) beside the
YUY2 conversion launch (stage 6) -- the path the same camera's raw mode takes -- and, on the host, the entropy decode of a synthetic 4:2:2
picture of roughly 250 KB with the coefficient bytes it hands over.  First measurements; no threshold is set."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ceracoder_amd import enc as E
from tests import jpegref as J


def synthetic(w, h, target=250_000):
    """a 4:2:2 picture near `target` bytes: noise on gradients, the quantiser scale searched"""
    best = None
    for percent in (100, 60, 40, 25, 15, 10):
        q = (J.scaled_q(J.Q_LUMA, percent), J.scaled_q(J.Q_CHROMA, percent))
        data, _ = J.write_jpeg(J.subsample(*J.picture(w, h, 5, noise=14), "422"), "422", qts=q, dht=False)
        if best is None or abs(len(data) - target) < abs(len(best) - target):
            best = data
        if len(data) >= target:
            break
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "jpeg_input_price.md"))
    args = ap.parse_args()
    rows = []
    for w, h in ((1280, 720), (1920, 1080)):
        e = E.Encoder(w, h, fixed_qp=30)
        data = synthetic(w, h)
        info, coefs, _ = E.jpeg_entropy_decode(data)
        L, buf = E.load(), np.frombuffer(data, np.uint8)
        coef = np.zeros(sum(c.size for c in coefs), np.int16)
        qt = np.zeros((3, 64), np.uint16)
        ms = []
        for _ in range(20):
            t0 = time.perf_counter()
            L.mi355enc_jpeg_entropy_decode(buf.ctypes.data, buf.size, coef.ctypes.data, coef.size, qt.ctypes.data, None)
            ms.append((time.perf_counter() - t0) * 1e3)
        e.stage_jpeg(data)  # the coefficient buffer holds a real picture
        jpeg = [e.time_stage(E.STAGE_JPEG, args.iters) for _ in range(3)]
        yuy2 = [e.time_stage(E.STAGE_CSC_YUY2, args.iters) for _ in range(3)]
        rows.append((w, h, len(data), min(jpeg), min(yuy2), float(np.median(ms)), min(ms), coef.nbytes))
        e.close()
    lines = ["# MJPEG input: first measurements", "",
             "`tools/probe_jpeg.py`: the JPEG launch (stage 12, 4:2:2) and the YUY2 conversion launch (stage 6) timed with HIP events over %d back-to-back launches "
             "(best of three series); the host entropy decode of a synthetic 4:2:2 picture on one core (median and best of 20). No threshold is set." % args.iters, "",
             "| size | JPEG bytes | JPEG launch (ms) | YUY2 launch (ms) | entropy decode, median (ms) | best (ms) | coefficient bytes |", "|---|---|---|---|---|---|---|"]
    for w, h, n, j, y, med, best, cb in rows:
        lines.append("| %dx%d | %d | %.4f | %.4f | %.2f | %.2f | %d |" % (w, h, n, j, y, med, best, cb))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
