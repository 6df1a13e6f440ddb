"""The picture controls' launches alone, in one process at 1080p and 2160p, HIP events: mi355enc_time_stage 23 (the pointwise form, luma
table + chroma rotation) and 24 (the stencil form: the launch into the scratch plane, which then changes places with the slot's) beside 17 (yuv_convert_kernel: the same read-and-write
of 1.5 P bytes as the pointwise form) and 18 (k_rate's mix).  Every launch works in place on slot 0's surfaces, so a long run would time whatever the content
has drifted to (a sharpened picture sharpened again ends at 0 and 255, where the table look-ups meet on few banks): the content is noise, uploaded afresh in
front of every burst of BURST launches, the parameters move it as little as active ones can (an identity table that is looked up all the same, a half-turn
of the chroma, sharpen 1), and a figure is the mean over BURSTS bursts.  Prints one JSON line per launch and size; --once: one burst of one launch each."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402

ONCE = "--once" in sys.argv
BURST, BURSTS = (1, 1) if ONCE else (10, 30)
NS = 10 ** 9
POINT = dict(brightness=1, hue=1000)  # L[v] = v (a thousandth of the scale rounds away) but not neutral: looked up; Cb, Cr -> their mirror images about 128
SHARP = dict(brightness=1, sharpen=1)


def timed(e, stage, y, uv):
    ms = []
    for _ in range(BURSTS):
        e.stage_adjust({}, y, uv)  # (neutral: uploads the planes into slot 0's surfaces and launches nothing)
        ms.append(e.time_stage(stage, BURST))
    ms.sort()
    return dict(us_mean=round(1000 * float(np.mean(ms)), 2), us_min=round(1000 * ms[0], 2), us_median=round(1000 * ms[len(ms) // 2], 2), us_max=round(1000 * ms[-1], 2))


for w, h in ((1920, 1080), (3840, 2160)):
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    rng = np.random.default_rng(w)
    y, uv = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
    P = W * H
    cases = (("adjust pointwise", E.STAGE_ADJUST_POINT, dict(adjust=POINT), 3 * P),
             ("adjust stencil", E.STAGE_ADJUST_SHARPEN, dict(adjust=SHARP), 2 * P),  # luma P read, P written to the scratch plane, which becomes the slot's; chroma neutral here (+ P when it is not)
             ("adjust stencil, no table", E.STAGE_ADJUST_SHARPEN, dict(adjust=dict(sharpen=1)), 2 * P),
             ("yuv_convert", E.STAGE_YUV_CONVERT, dict(colorimetry=(0, 1, 1, 1), input_colorimetry=(1, 6)), 3 * P),
             ("rate mix", E.STAGE_RATE, dict(pipeline_depth=1, rate=(2, NS, 1)), 6 * P))  # reads the keep buffer and the slot, writes the slot and the keep buffer: 4 x 1.5 P
    for name, stage, kw, nbytes in cases:
        e = E.Encoder(w, h, fps=30, fixed_qp=28, **kw)
        timed(e, stage, y, uv)  # warm: allocations, code objects
        r = timed(e, stage, y, uv)
        r.update(launch=name, size="%dx%d" % (w, h), launches=BURST * BURSTS, algorithmic_bytes=nbytes, gb_per_s=round(nbytes / r["us_mean"] / 1000.0, 1))
        print(json.dumps(r), flush=True)
        e.close()
