"""The motion-compensated noise filter's launches alone, in one process at 1080p and 2160p, HIP events, with tools/probe_denoise.py's
protocol: a still picture plus Gaussian noise of sigma 3, uploaded afresh with new noise in front of every burst of BURST launches, the handle's history kept; a
figure is the mean over BURSTS bursts.  Per size and range (4, 8, 16): mi355enc_time_stage 27 (denoise_search_kernel alone) and 28 (the search and
denoise_mc_kernel<1, 2>), the compensated filter as their difference, beside 25 (the in-place filter, both planes) and 0 (me_kernel: the same number of
candidate-samples per picture as the search at range 16).  The search is a full search: its time does not depend on the content.  Algorithmic bytes: the search
reads the luma (P) and its history (2 P) and writes a word per block (P / 16); the compensated filter moves the in-place filter's 9 P and reads those words.
Prints one JSON line per launch, size and range; --once: one burst of one launch each."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402

ONCE = "--once" in sys.argv
BURST, BURSTS = (1, 1) if ONCE else (10, 30)


def timed(e, stage, base, rng):
    ms = []
    for _ in range(BURSTS):
        y, uv = (np.clip(np.rint(p + 3.0 * rng.standard_normal(p.shape, dtype=np.float32)), 0, 255).astype(np.uint8) for p in base)
        e.stage_denoise({}, y, uv)  # (off: uploads the planes into slot 0's surfaces and launches nothing)
        ms.append(e.time_stage(stage, BURST))
    ms.sort()
    return dict(us_mean=round(1000 * float(np.mean(ms)), 2), us_min=round(1000 * ms[0], 2), us_median=round(1000 * ms[len(ms) // 2], 2), us_max=round(1000 * ms[-1], 2))


def report(name, size, rng_, r, nbytes):
    r.update(launch=name, size="%dx%d" % size, range=rng_, launches=BURST * BURSTS, algorithmic_bytes=nbytes, gb_per_s=round(nbytes / r["us_mean"] / 1000.0, 1) if nbytes else None)
    print(json.dumps(r), flush=True)


for w, h in ((1920, 1080), (3840, 2160)):
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    rng = np.random.default_rng(w)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = (60 + 0.05 * xx + 0.04 * yy + 40 * (((xx // 32) + (yy // 32)) % 2), 128 + 24 * ((xx[:H // 2] // 16) % 2))
    P = W * H
    e = E.Encoder(w, h, fps=30, fixed_qp=28, denoise=dict(luma=8, chroma=8))
    for name, stage, nbytes in (("denoise both, in place", E.STAGE_DENOISE, 9 * P), ("me_kernel", E.STAGE_ME, 0)):
        timed(e, stage, base, rng)  # warm: allocations, code objects, a converged history
        report(name, (w, h), 0, timed(e, stage, base, rng), nbytes)
    for r_ in (4, 8, 16):
        e.set_denoise_motion(r_)
        timed(e, E.STAGE_DENOISE_MC, base, rng)
        s = timed(e, E.STAGE_DENOISE_SEARCH, base, rng)
        b = timed(e, E.STAGE_DENOISE_MC, base, rng)
        report("denoise search", (w, h), r_, s, 3 * P + P // 16)
        report("denoise search + compensated filter", (w, h), r_, dict(b), 12 * P + P // 8)
        f = {k: round(b[k] - s[k], 2) for k in ("us_mean", "us_median")}  # (min and max of a difference mean nothing)
        report("compensated filter (difference)", (w, h), r_, f, 9 * P + P // 16)
    e.close()
