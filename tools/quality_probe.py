#!/usr/bin/env python3
"""What the quality metrics (mi355enc_set_quality_metrics) cost: python tools/quality_probe.py [--frames N] [--reps R] [--out FILE]

1. The kernel alone at 1080p and 2160p: HIP events around back-to-back launches on the surfaces a short encode left behind
   (mi355enc_time_stage, stage 11), and the host's view of one synchronised launch through mi355enc_stage_quality_device.
2. The 1080p IPPP stream on device-resident pictures at pipeline_depth 2 (exclusive_device, fixed QP: bench.py's timed path) with metrics
   off and on, alternating in one process; the spread between the runs of one kind is the margin a difference has to exceed.
Writes both as markdown to --out (default profiles/quality_metrics_price.md).  Needs an MI355X; there is no fallback."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ceracoder_amd import enc as E
from ceracoder_amd import synth


def kernel_alone(iters):
    rows = []
    for w, h in ((1920, 1080), (3840, 2160)):
        e = E.Encoder(w, h, fixed_qp=30, gop=60)
        for i, (y, uv) in enumerate(synth.s2_frames(w, h, 3)):
            e.encode(y, uv, pts=i)
        e.time_stage(E.STAGE_QUALITY, 20)  # warm: code object loaded, both pictures resident in the Infinity Cache
        ev = [e.time_stage(E.STAGE_QUALITY, iters) * 1e3 for _ in range(3)]
        W, H = e.mbw * 16, e.mbh * 16
        sy, suv = torch.randint(0, 256, (h * W + 16,), dtype=torch.uint8, device="cuda"), torch.randint(0, 256, (h // 2 * W + 16,), dtype=torch.uint8, device="cuda")  # (+ 16: room for the offset)
        ry, ruv = torch.randint(0, 256, (H * W,), dtype=torch.uint8, device="cuda"), torch.randint(0, 256, (H // 2 * W,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        host = {}
        for name, off in (("aligned", 0), ("byte-wise (source 1 byte in)", 1)):
            args = (sy.data_ptr() + off, suv.data_ptr() + off, W, ry.data_ptr(), ruv.data_ptr())
            for _ in range(20):
                e.stage_quality_device(*args)
            t0 = time.perf_counter()
            for _ in range(iters):
                e.stage_quality_device(*args)
            host[name] = (time.perf_counter() - t0) / iters * 1e6
        e.close()
        rows.append((w, h, 3.0 * w * h / 1e6, ev, host))
    return rows


def stream(frames, reps):
    w, h, warm = 1920, 1080, 60
    clip = list(synth.s2_frames(w, h, 32))
    dev = [(torch.from_numpy(np.ascontiguousarray(y)).cuda(), torch.from_numpy(np.ascontiguousarray(uv)).cuda()) for y, uv in clip]
    torch.cuda.synchronize()
    fps = {False: [], True: []}
    last = None
    for rep in range(reps):
        for on in (False, True):
            e = E.Encoder(w, h, gop=60, fixed_qp=30, pipeline_depth=2, exclusive=True, slices=None, slice_deblock=None)
            if on:
                e.set_quality_metrics(True)
            for i in range(frames + warm):
                if i == warm:
                    t0 = time.perf_counter()
                y, uv = dev[i % len(dev)]
                e.submit_device(y.data_ptr(), w, uv.data_ptr(), w, pts=i)
                if e.pending > 2:
                    e.collect(copy=False)
            while e.pending:
                e.collect(copy=False)
            fps[on].append(frames / (time.perf_counter() - t0))
            if on:
                last = e.quality_totals()
            e.close()
    return fps, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "quality_metrics_price.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    rows = kernel_alone(a.iters)
    fps, tot = stream(a.frames, a.reps)
    out = ["## The kernel alone (tools/quality_probe.py)", "",
           "`quality_kernel`, %d back-to-back launches between two HIP events (three repeats), on the source and reconstruction a short encode left in HBM;" % a.iters,
           "and the host clock around one synchronised launch through `mi355enc_stage_quality_device` (launch and synchronise included: a cross-check).", "",
           "| size | algorithmic bytes (3.0 P) | per launch, HIP events | algorithmic rate | host, aligned | host, byte-wise path |", "|---|---|---|---|---|---|"]
    for w, h, mb, ev, host in rows:
        out.append("| %dx%d | %.2f MB | %s us | %.2f TB/s | %.1f us | %.1f us |" % (w, h, mb, " / ".join("%.2f" % v for v in ev), mb / min(ev), host["aligned"],
                                                                                 host["byte-wise (source 1 byte in)"]))
    off, on = fps[False], fps[True]
    out += ["", "## The stream: 1080p IPPP, pipeline_depth 2, device-resident input, fixed QP 30, %d pictures per run, off and on alternating in one process" % a.frames, "",
            "| metrics | frames/s per run | mean | spread (max - min) |", "|---|---|---|---|",
            "| off | %s | %.0f | %.0f |" % (" / ".join("%.0f" % v for v in off), np.mean(off), max(off) - min(off)),
            "| on | %s | %.0f | %.0f |" % (" / ".join("%.0f" % v for v in on), np.mean(on), max(on) - min(on)), "",
            "Per picture: %.2f us with metrics off, %.2f us with them on: %+.2f us." % (1e6 / np.mean(off), 1e6 / np.mean(on), 1e6 / np.mean(on) - 1e6 / np.mean(off)),
            "The last run's totals: PSNR-Y %.2f dB, Cb %.2f, Cr %.2f, mean SSIM %.4f over %d pictures." % (tot.psnr[0], tot.psnr[1], tot.psnr[2], tot.ssim, tot.pictures), ""]
    text = "\n".join(out)
    print(text, flush=True)
    if a.out != "-":
        head = ""
        if os.path.exists(a.out):  # everything above the first measured section stays
            head = open(a.out).read().split("## The kernel alone (tools/quality_probe.py)")[0]
        open(a.out, "w").write(head + text)


if __name__ == "__main__":
    main()
