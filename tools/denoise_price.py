"""What the temporal noise filter buys and costs.

Default: the benchmark's clip (synth.s2_frames, 1080p) plus seeded Gaussian noise of sigma 3 on every plane, coded IPPP at fixed QP 26 / 32 / 38 with the filter
off, at strength 4 and at strength 8 (luma = chroma).  Per case, over the P pictures: bytes per picture, the share of macroblocks coded without a residual
(inter 16 x 16 with no coefficient: P_Skip or a bare vector -- the records do not tell the two apart), and PSNR-Y of the reconstruction (which the independent
decoder reproduces: tests/test_denoise_gpu.py) against the CLEAN clip, not the noisy source.  Then the same with the clip's first picture held still -- the camera
on a tripod the filter is for; the benchmark's clip pans, and a filter without motion compensation has little to work with there.  Prints two markdown tables.

--fps STRENGTH: frames/s of the benchmark's 1080p IPPP configuration (60 pictures/s, GOP 60, 6 Mbit/s, three pictures in flight, pictures from device memory)
with the filter at STRENGTH (0: off) in this process; one JSON line.  Run it in alternating processes to compare.

--motion R [R ...]: the motion-compensated form -- the pan's table alone, with the filter off, at strength 8, and at strength 8 with each
search range R; with --fps, the one range the filter runs with."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402
from ceracoder_amd import synth  # noqa: E402

W, H, SIGMA = 1920, 1080, 3.0


def clips(n, still, seed=2400):
    rng = np.random.default_rng(seed)
    clean = [(y.copy(), uv.copy()) for y, uv in synth.s2_frames(W, H, n)]
    if still:
        clean = [clean[0]] * n
    noisy = [tuple(np.clip(np.rint(p + SIGMA * rng.standard_normal(p.shape, dtype=np.float32)), 0, 255).astype(np.uint8) for p in f) for f in clean]
    return clean, noisy


def price(n, still, cases=((0, 0), (4, 0), (8, 0))):
    """cases: (strength, search range) per row"""
    clean, noisy = clips(n, still)
    print("%s, %d pictures, Gaussian noise sigma %g:\n" % ("The clip's first picture held still (a camera on a tripod)" if still else "The benchmark's clip (a pan with moving objects)", n, SIGMA))
    print("| QP | filter | bytes / P picture | macroblocks without residual | PSNR-Y against the clean clip (dB) | PSNR-Y of the source against the clean clip (dB) |")
    print("|---|---|---|---|---|---|")
    for qp in (26, 32, 38):
        for s, r in cases:
            e = E.Encoder(W, H, fps=60, gop=n, fixed_qp=qp, denoise=dict(luma=s, chroma=s, motion=r))
            size, bare, psnr, src = [], [], [], []
            for i in range(n):
                au = e.encode(*noisy[i], pts=i)[0]
                if i == 0:
                    continue
                mb = e.fetch(E.FETCH_MBINFO)
                size.append(len(au))
                bare.append(float(np.mean((mb["mb_type"] == 1) & (mb["nzmask"] == 0) & (mb["i16_mode"] == 0))))
                psnr.append(synth.psnr(e.fetch(E.FETCH_RECON_Y)[:H, :W], clean[i][0]))
                src.append(synth.psnr(e.fetch(E.FETCH_SOURCE_Y)[:H, :W], clean[i][0]))
            e.close()
            print("| %d | %s | %d | %.1f %% | %.2f | %.2f |" % (qp, ("%d, range %d" % (s, r) if r else s) if s else "off", round(np.mean(size)), 100 * np.mean(bare), np.mean(psnr), np.mean(src)), flush=True)


def fps(strength, steps, warmup, unique=32, motion=0):
    import torch
    frames = np.empty((unique, H * 3 // 2, W), np.uint8)
    rng = np.random.default_rng(2400)
    for i, (y, uv) in enumerate(synth.s2_frames(W, H, unique)):
        frames[i, :H], frames[i, H:] = y, uv
    frames = np.clip(np.rint(frames + SIGMA * rng.standard_normal(frames.shape, dtype=np.float32)), 0, 255).astype(np.uint8)
    dev = torch.from_numpy(frames).cuda()
    base, fbytes = dev.data_ptr(), dev.stride(0)
    e = E.Encoder(W, H, fps=60, gop=60, bitrate_bps=6_000_000, pipeline_depth=2, exclusive=True, denoise=dict(luma=strength, chroma=strength, motion=motion))

    def run(n, first):
        for i in range(first, first + n):
            k = i % (2 * unique - 2)
            p = base + (k if k < unique else 2 * unique - 2 - k) * fbytes
            e.submit_device(p, W, p + H * W, W, pts=i)
            if e.pending > 2:
                e.collect(copy=False)
        while e.pending:
            e.collect(copy=False)
    run(warmup, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps, warmup)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(denoise=strength, motion=motion, steps=steps, frames_per_s=round(steps / dt, 2), history_bytes=e.debug_denoise_bytes())), flush=True)
    e.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fps", type=int, default=None, metavar="STRENGTH")
    ap.add_argument("--pictures", type=int, default=16)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--warmup", type=int, default=120)
    ap.add_argument("--motion", type=int, nargs="+", default=None, metavar="R")
    a = ap.parse_args()
    if a.fps is not None:
        fps(a.fps, a.steps, a.warmup, motion=a.motion[0] if a.motion else 0)
    elif a.motion:
        price(a.pictures, False, [(0, 0), (8, 0)] + [(8, r) for r in a.motion])
    else:
        price(a.pictures, False)
        print()
        price(a.pictures, True)
