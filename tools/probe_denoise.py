"""The temporal noise filter's launch alone, in one process at 1080p and 2160p, HIP events: mi355enc_time_stage 26 (priming, both planes),
25 with the luma alone and with both planes, beside 23 (adjust_point_kernel, luma table + chroma rotation) and 17 (yuv_convert_kernel) -- pure streaming kernels
with the same ownership, reading and writing 1.5 P bytes each.  The launch works in place on slot 0's surfaces and on the handle's history, so a long run would
time a picture filtered over and over (input = history: every look-up at difference 0): the content is a still picture plus Gaussian noise of sigma 3 (what
strength 8 is for), uploaded afresh with new noise in front of every burst of BURST launches; the history stays, so the first launch of a burst filters a new
noisy picture against a converged history and the others what it left.  A figure is the mean over BURSTS bursts.  Prints one JSON line per launch and size;
--once: one burst of one launch each."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402

ONCE = "--once" in sys.argv
BURST, BURSTS = (1, 1) if ONCE else (10, 30)
POINT = dict(brightness=1, hue=1000)  # (tools/probe_adjust.py's: an identity table that is looked up all the same, a half-turn of the chroma)


def timed(e, stage, base, rng):
    ms = []
    for _ in range(BURSTS):
        y, uv = (np.clip(np.rint(p + 3.0 * rng.standard_normal(p.shape, dtype=np.float32)), 0, 255).astype(np.uint8) for p in base)
        e.stage_denoise({}, y, uv)  # (off: uploads the planes into slot 0's surfaces and launches nothing)
        ms.append(e.time_stage(stage, BURST))
    ms.sort()
    return dict(us_mean=round(1000 * float(np.mean(ms)), 2), us_min=round(1000 * ms[0], 2), us_median=round(1000 * ms[len(ms) // 2], 2), us_max=round(1000 * ms[-1], 2))


for w, h in ((1920, 1080), (3840, 2160)):
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    rng = np.random.default_rng(w)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = (60 + 0.05 * xx + 0.04 * yy + 40 * (((xx // 32) + (yy // 32)) % 2), 128 + 24 * ((xx[:H // 2] // 16) % 2))
    P = W * H
    cases = (("denoise prime", E.STAGE_DENOISE_PRIME, dict(denoise=dict(luma=8, chroma=8)), 9 * P // 2),  # reads the slot (1.5 P), writes the history (3 P)
             ("denoise luma", E.STAGE_DENOISE, dict(denoise=dict(luma=8)), 6 * P),                         # reads P + 2 P, writes P + 2 P
             ("denoise both", E.STAGE_DENOISE, dict(denoise=dict(luma=8, chroma=8)), 9 * P),               # reads 1.5 P + 3 P, writes 1.5 P + 3 P
             ("adjust pointwise", E.STAGE_ADJUST_POINT, dict(adjust=POINT), 3 * P),
             ("yuv_convert", E.STAGE_YUV_CONVERT, dict(colorimetry=(0, 1, 1, 1), input_colorimetry=(1, 6)), 3 * P))
    for name, stage, kw, nbytes in cases:
        e = E.Encoder(w, h, fps=30, fixed_qp=28, **kw)
        timed(e, stage, base, rng)  # warm: allocations, code objects, a converged history
        r = timed(e, stage, base, rng)
        r.update(launch=name, size="%dx%d" % (w, h), launches=BURST * BURSTS, algorithmic_bytes=nbytes, gb_per_s=round(nbytes / r["us_mean"] / 1000.0, 1))
        print(json.dumps(r), flush=True)
        e.close()
