"""The 3D colour LUT launch alone, in one process at 1080p and 2160p, HIP events: mi355enc_time_stage 35 with each launch form forced
(mi355enc_debug_lut3d_form) -- direct and staged at N = 17 and 33, direct at N = 65 -- beside 23, the existing pointwise picture-control launch (the same
in-place read and write of 1.5 P bytes), and 31, the warp launch (the other gather of this code), as yardsticks from the same run.  Two contents: seeded noise
(every sample its own cell: the worst locality the table can meet) and a flat picture (every lane the same four nodes).  The table is seeded noise, so a graded
noise picture stays noise however often the launch runs on it in place; the content is uploaded afresh in front of every burst of BURST launches.  The series
alternate -- one burst of each launch per round -- and a figure is the median over ROUNDS rounds.  Prints one JSON line per launch, content and size; --once:
one round of one launch each."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402

ONCE = "--once" in sys.argv
BURST, ROUNDS = (1, 1) if ONCE else (10, 30)
POINT = dict(brightness=1, hue=1000)  # tools/probe_adjust.py's: an identity table that is looked up all the same, a half-turn of the chroma
LAUNCHES = [("adjust pointwise", None, None), ("warp barrel bicubic", None, None)] + [("lut3d N=%d %s" % (N, "staged" if form else "direct"), N, form)
                                                                              for N, form in ((17, 0), (17, 1), (33, 0), (33, 1), (65, 0))]


def table(N):
    return np.random.default_rng(N).integers(0, 1 << 30, N ** 3, dtype=np.uint32)


def series(e, y, uv):
    ms = {name: [] for name, _, _ in LAUNCHES}
    for _ in range(ROUNDS):
        for name, N, form in LAUNCHES:
            if N is not None:
                e.set_lut3d(table(N))
                e.debug_lut3d_form(form)
            e.stage_adjust({}, y, uv)  # (neutral: uploads the planes into slot 0's surfaces and launches nothing)
            ms[name].append(e.time_stage(E.STAGE_ADJUST_POINT if name.startswith("adjust") else E.STAGE_WARP if N is None else E.STAGE_LUT3D, BURST))
    return ms


for w, h in ((1920, 1080), (3840, 2160)):
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    rng = np.random.default_rng(w)
    contents = (("noise", rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)),
                ("flat", np.full((H, W), 97, np.uint8), np.tile(np.array([110, 140], np.uint8), (H // 2, W // 2))))
    e = E.Encoder(w, h, fps=30, fixed_qp=28, adjust=POINT)
    e.set_warp(dict(kind=E.WARP_BICUBIC), k1=-13107, k2=1966)  # (tools/probe_warp.py's barrel)
    for content, y, uv in contents:
        series(e, y, uv)  # warm: allocations, code objects
        ms = series(e, y, uv)
        yard = float(np.median(ms["adjust pointwise"]))
        for name, N, form in LAUNCHES:
            v = sorted(ms[name])
            med = float(np.median(v))
            print(json.dumps(dict(launch=name, content=content, size="%dx%d" % (w, h), launches=BURST * ROUNDS, us_median=round(1000 * med, 2), us_min=round(1000 * v[0], 2),
                                  us_max=round(1000 * v[-1], 2), times_adjust=round(med / yard, 2), plan=None if N is None else E.lut3d_plan(N))), flush=True)
    e.close()
