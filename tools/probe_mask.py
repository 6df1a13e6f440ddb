"""The privacy masks' launches alone at 1080p, in one process, HIP events: mi355enc_time_stage 38 (the pixelate launch and the commit
launch) and 39 (the blur launches: four passes a batch) for three configurations -- one 320 x 320 pixelate with c = 16, one 320 x 320 blur with r = 16, eight
200 x 200 blurs with r = 32 -- beside 24, the sharpen stencil over the whole picture, as the yardstick from the same run.  The content is seeded noise, uploaded
afresh in front of every burst of BURST launches (the commit launch works in place).  The series alternate -- one burst of each per round -- and a figure is
the median over ROUNDS rounds.  Prints one JSON line per series.  --once: ten rounds of one launch each, for a kernel trace in a run of its own
(`rocprofv3 --kernel-trace --output-format csv -- python tools/probe_mask.py --once`): the cases differ in their grids."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402

ONCE = "--once" in sys.argv
BURST, ROUNDS = (1, 10) if ONCE else (10, 30)
W, H = 1920, 1080
CASES = [("pixelate 320x320 c=16", [(800, 380, 320, 320, 2, 16)], E.STAGE_MASK_CELLS, 320 * 320),
         ("blur 320x320 r=16", [(800, 380, 320, 320, 3, 16)], E.STAGE_MASK_BLUR, 4 * 320 * 320),
         ("commit of the 320x320 blur", [(800, 380, 320, 320, 3, 16), (0, 0, 2, 2, 1, 0)], E.STAGE_MASK_CELLS, 320 * 320),
         ("blur 8 x 200x200 r=32", [(100 + 220 * k, 200 + 60 * k, 200, 200, 3, 32) for k in range(8)], E.STAGE_MASK_BLUR, 4 * 8 * 200 * 200),
         ("sharpen stencil 1920x1080", None, E.STAGE_ADJUST_SHARPEN, W * H)]


def series(e, y, uv):
    ms = {name: [] for name, _, _, _ in CASES}
    for _ in range(ROUNDS):
        for name, regs, stage, _ in CASES:
            if regs:
                e.set_mask(regs)
            e.stage_adjust({}, y, uv)  # (neutral: uploads the planes into slot 0's surfaces and launches nothing)
            ms[name].append(e.time_stage(stage, BURST))
    return ms


rng = np.random.default_rng(W)
y, uv = rng.integers(0, 256, (1088, W), dtype=np.uint8), rng.integers(0, 256, (544, W), dtype=np.uint8)
e = E.Encoder(W, H, fps=30, fixed_qp=28, adjust=dict(sharpen=16))
series(e, y, uv)  # warm: allocations, code objects
ms = series(e, y, uv)
yard = float(np.median(ms["sharpen stencil 1920x1080"])) / (W * H)
for name, regs, stage, samples in CASES:
    v = sorted(ms[name])
    med = float(np.median(v))
    print(json.dumps(dict(series=name, stage=stage, launches=BURST * ROUNDS, us_median=round(1000 * med, 2), us_min=round(1000 * v[0], 2), us_max=round(1000 * v[-1], 2),
                          luma_samples_passed=samples, ps_per_sample=round(1e9 * med / samples, 2), times_sharpen_per_sample=round(med / samples / yard, 2))), flush=True)
e.close()
