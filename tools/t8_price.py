#!/usr/bin/env python3
"""GPU: what the per-macroblock transform size choice (cfg.transform8x8 = 2, element property dct8x8-adaptive) costs and buys against the 8x8 transform for
every coded inter macroblock (transform8x8 = 1) and against Constrained Baseline (0).
 (a) quality at EQUAL fixed QP 26 / 32 / 38, 1080p, S2 and S4: kbit/s and PSNR-Y for the three modes with the superfast toolset otherwise (i8x8 + aq-mode 1;
     mode 0 has neither, it cannot), plus QP 32 with aq off;
 (b) pictures/s under CBR with three pictures in flight and the device exclusive (sources resident in HBM), 1080p and 2160p, mode 1 against mode 2, the two
     alternated three times (best of three each).
    python tools/t8_price.py [out.md]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from ceracoder_amd import enc as E, synth

lines = []
def say(s=""):
    print(s, flush=True); lines.append(s)

def clip_of(kind, w, h):
    return list(synth.s2_frames(w, h, 16)) if kind == "S2" else list(synth.s4_frames(w, h, 16))

def speed(w, h, n, **kw):
    clip = clip_of("S2", w, h)
    bufs = [torch.from_numpy(np.concatenate([y.reshape(-1), uv.reshape(-1)])).cuda() for y, uv in clip]
    torch.cuda.synchronize()
    e = E.Encoder(w, h, fps=60, gop=60, pipeline_depth=2, exclusive=True, **kw)
    def run(cnt, base):
        nb = 0
        for i in range(cnt):
            k = (base + i) % 30
            p = bufs[k if k < 16 else 30 - k].data_ptr()
            e.submit_device(p, w, p + w * h, w, pts=base + i)
            if e.pending > 2: nb += e.collect(copy=False)[0]
        while e.pending: nb += e.collect(copy=False)[0]
        return nb
    run(60, 0)
    t0 = time.perf_counter(); nb = run(n, 60); t = time.perf_counter() - t0
    rec = e.stats().recoveries
    e.close()
    assert rec == 0
    return n / t, nb * 8 * 60 / n

def quality(kind, w, h, n, **kw):
    clip = clip_of(kind, w, h)
    e = E.Encoder(w, h, fps=60, gop=60, pipeline_depth=0, **kw)
    ps, nb, n8, n4 = [], 0, 0, 0
    for i in range(n):
        k = i % 30
        y, uv = clip[k if k < 16 else 30 - k]
        e.submit(y, uv, pts=i)
        au, key, pts, qp = e.collect(copy=False)
        ps.append(synth.psnr(y, e.fetch(E.FETCH_RECON_Y)[:h, :w])); nb += au
        if not key:
            m = e.fetch(E.FETCH_MBINFO)
            coded = (m["mb_type"] == 1) & ((m["nzmask"] & 0xFFFF) != 0)
            t8 = (m["nzmask"] & (1 << 27)) != 0
            n8 += int((coded & t8).sum()); n4 += int((coded & ~t8).sum())
    e.close()
    return nb * 8 * 60 / n, float(np.mean(ps)), (n8 / max(1, n8 + n4))

BASE = dict(slices=None, slice_deblock=None)
MODES = ((0, "0: Constrained Baseline", dict(transform8x8=0)), (1, "1: 8x8 for every coded inter MB", dict(transform8x8=1, i8x8=True)),
         (2, "2: 4x4 / 8x8 per MB", dict(transform8x8=2, i8x8=True)))
w, h = 1920, 1080
say("## (a) fixed QP, 1080p60, 60 pictures (one IDR), library-default slices; aq-mode 1 unless marked")
say("| clip | QP | aq | transform8x8 | kbit/s | PSNR-Y | coded inter MBs with 8x8 | mode 2 vs 1: bits | PSNR-Y |")
say("|---|---|---|---|---|---|---|---|---|")
for kind in ("S2", "S4"):
    for qp, aq in ((26, True), (32, True), (38, True), (32, False)):
        if not aq and kind == "S4":
            continue
        r = {}
        for mode, name, kw in MODES:
            rate, p, f8 = quality(kind, w, h, 60, fixed_qp=qp, aq=aq, **BASE, **kw)
            r[mode] = (rate, p)
            rel = "%+.2f %% | %+.3f dB" % (100.0 * (rate / r[1][0] - 1), p - r[1][1]) if mode == 2 else " | "
            say("| %s | %d | %s | %s | %.0f | %.3f | %.0f %% | %s |" % (kind, qp, "on" if aq else "off", name, rate / 1e3, p, 100 * f8, rel))
say()
say("## (b) pictures/s, CBR, 3 in flight, exclusive device, S2, dct8x8 + i8x8 + aq-mode 1 (best of three, alternated)")
say("| geometry | Mbit/s | transform8x8 = 1 | transform8x8 = 2 | 2 vs 1 |")
say("|---|---|---|---|---|")
for (w, h, bps, n) in ((1920, 1080, 6_000_000, 600), (3840, 2160, 20_000_000, 300)):
    best = {1: 0.0, 2: 0.0}
    for _ in range(3):
        for mode in (1, 2):
            fps, _ = speed(w, h, n, bitrate_bps=bps, transform8x8=mode, i8x8=True, aq=True, **BASE)
            best[mode] = max(best[mode], fps)
    say("| %dx%d | %.0f | %.0f | %.0f | %+.1f %% |" % (w, h, bps / 1e6, best[1], best[2], 100.0 * (best[2] / best[1] - 1)))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
