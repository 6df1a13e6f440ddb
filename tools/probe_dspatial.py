"""The spatial noise filter's launches alone, in one process at 1080p and 2160p, HIP events: mi355enc_time_stage 36 with a manual setting
(the luma launch alone, and both planes' launches) and 37 with an automatic one (measure + decide alone, with both bounds 0; and the whole step), beside 24
(adjust_sharpen_kernel, the 3 x 3 stencil of the same shape on the luma plane).  The filter launches exchange slot 0's planes with the scratch planes, so a long
run would time a picture filtered again and again: the content -- a smooth scene under Gaussian noise of 3 codes, what the step is for -- is uploaded afresh
in front of every burst of BURST launches, and a figure is the mean over BURSTS bursts.  Prints one JSON line per launch and size, and writes them to
profiles/dspatial_probe.txt; --once: one burst of one launch each."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ceracoder_amd import enc as E  # noqa: E402

ONCE = "--once" in sys.argv
BURST, BURSTS = (1, 1) if ONCE else (10, 30)


def timed(e, stage, y, uv):
    ms = []
    for _ in range(BURSTS):
        e.stage_adjust({}, y, uv)  # (neutral: uploads the planes into slot 0's surfaces and launches nothing)
        ms.append(e.time_stage(stage, BURST))
    ms.sort()
    return dict(us_mean=round(1000 * float(np.mean(ms)), 2), us_min=round(1000 * ms[0], 2), us_median=round(1000 * ms[len(ms) // 2], 2), us_max=round(1000 * ms[-1], 2))


lines = []
for w, h in ((1920, 1080), (3840, 2160)):
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    rng = np.random.default_rng(w)
    xx, yy = np.meshgrid(np.arange(W), np.arange(H))
    y = np.clip(np.rint(120 + 40 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 3 * rng.standard_normal((H, W))), 0, 255).astype(np.uint8)
    uv = np.clip(np.rint(128 + 3 * rng.standard_normal((H // 2, W))), 0, 255).astype(np.uint8)
    P = W * H
    cases = (("dspatial filter, luma", E.STAGE_DENOISE_SPATIAL, dict(denoise_spatial=dict(luma=6)), 2 * P),  # P read, P written to the scratch plane
             ("dspatial filter, both planes", E.STAGE_DENOISE_SPATIAL, dict(denoise_spatial=dict(luma=6, chroma=6)), 3 * P),
             ("dspatial measure + decide", E.STAGE_DENOISE_SPATIAL_AUTO, dict(denoise_spatial=dict(auto_gain=2000)), P),  # the luma plane read once
             ("dspatial measure + decide + filter, both planes", E.STAGE_DENOISE_SPATIAL_AUTO, dict(denoise_spatial=dict(luma=32, chroma=32, auto_gain=2000)), 4 * P),
             ("adjust stencil, no table", E.STAGE_ADJUST_SHARPEN, dict(adjust=dict(sharpen=1)), 2 * P))
    for name, stage, kw, nbytes in cases:
        e = E.Encoder(w, h, fps=30, fixed_qp=28, **kw)
        timed(e, stage, y, uv)  # warm: allocations, code objects
        r = timed(e, stage, y, uv)
        r.update(launch=name, size="%dx%d" % (w, h), launches=BURST * BURSTS, algorithmic_bytes=nbytes, gb_per_s=round(nbytes / r["us_mean"] / 1000.0, 1))
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        e.close()
if not ONCE:
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dspatial_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
