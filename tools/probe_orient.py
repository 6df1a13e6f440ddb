#!/usr/bin/env python3
"""What orientation costs: python tools/probe_orient.py [--iters N] [--frames N] [--out profiles/orient_price.md]

Per size (1080p, 2160p): the orientation launch (mi355enc_time_stage stage 13, HIP events around back-to-back launches) for one transposing method
(90r) and one that is not (180), beside the I420 conversion launch of the same handle (stage 5) -- the yardstick: it moves the same 1.5 P in + 1.5 P out
and makes the same copy-speed claim.  Then the frames/s of a 1080p IPPP stream with and without orientation=90r, from this one process, alternating."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ceracoder_amd import enc as E
from ceracoder_amd import synth


def stream_fps(w, h, method, frames, pics):
    """frames/s of an IPPP stream at pipeline depth 2 from pinned host pictures (of the pre-orientation size), first picture excluded"""
    e = E.Encoder(w, h, gop=frames + 1, fixed_qp=30, pipeline_depth=2, orientation=method)
    pw, ph = e.input_size
    per = pw * ph * 3 // 2
    buf = E.PinnedBuffer(len(pics) * per)
    views = []
    for i, (y, uv) in enumerate(pics):
        a = buf.array[i * per:(i + 1) * per]
        sy, suv = (y, uv) if (pw, ph) == (w, h) else (np.ascontiguousarray(np.rot90(y, 1)), np.ascontiguousarray(np.rot90(uv.reshape(h // 2, w // 2, 2), 1)).reshape(ph // 2, pw))
        a[:pw * ph] = sy.ravel()
        a[pw * ph:] = suv.ravel()
        views.append((a[:pw * ph].reshape(ph, pw), a[pw * ph:].reshape(ph // 2, pw)))
    e.submit(*views[0], pts=0)
    e.collect(copy=False)
    t0 = time.perf_counter()
    for i in range(1, frames + 1):
        e.submit(*views[i % len(views)], pts=i)
        if e.pending > 2:
            e.collect(copy=False)
    while e.pending:
        e.collect(copy=False)
    dt = time.perf_counter() - t0
    e.close()
    del views, a
    buf.free()
    return frames / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "orient_price.md"))
    args = ap.parse_args()
    rows = []
    for w, h in ((1920, 1080), (3840, 2160)):
        r = [w, h]
        for method in ("90r", "180"):
            e = E.Encoder(w, h, fixed_qp=30, orientation=method)
            r.append(min(e.time_stage(E.STAGE_ORIENT, args.iters) for _ in range(3)))
            if method == "90r":
                csc = min(e.time_stage(E.STAGE_CSC_I420, args.iters) for _ in range(3))
            e.close()
        rows.append(tuple(r) + (csc,))
    w, h = 1920, 1080
    pics = list(synth.s2_frames(w, h, 8))
    fps = {0: [], 1: []}
    for _ in range(3):  # alternating: plain, 90r, plain, 90r, ...
        for method in (0, 1):
            fps[method].append(stream_fps(w, h, method, args.frames, pics))
    lines = ["# Orientation on the way in: first measurements", "",
             "`tools/probe_orient.py`: the orientation launch (stage 13) for 90r (through LDS) and 180 (no LDS) and the I420 conversion launch (stage 5) of the same handle, "
             "timed with HIP events over %d back-to-back launches (best of three series)." % args.iters, "",
             "| size | 90r launch (ms) | 180 launch (ms) | I420 conversion launch (ms) | 90r / conversion |", "|---|---|---|---|---|"]
    for w_, h_, t90, t180, c in rows:
        lines.append("| %dx%d | %.4f | %.4f | %.4f | %.2f |" % (w_, h_, t90, t180, c, t90 / c))
    lines += ["", "1080p IPPP, fixed QP 30, pipeline depth 2, pinned host input, %d pictures per run, three runs each, alternating in one process (frames/s):" % args.frames, "",
              "| orientation | runs | best |", "|---|---|---|",
              "| none | %s | %.0f |" % (", ".join("%.0f" % v for v in fps[0]), max(fps[0])),
              "| 90r | %s | %.0f |" % (", ".join("%.0f" % v for v in fps[1]), max(fps[1]))]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
