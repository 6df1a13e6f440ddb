"""The three launches of automatic levels and white balance alone, in one process at 1080p and 2160p, HIP events: mi355enc_time_stage
32 (measure), 33 (decide), 34 (apply) beside 23, the existing pointwise picture-control launch of the same build (the yardstick: the same in-place read and write
of 1.5 P bytes as apply).  Two contents: seeded noise (every LDS counter is hit about equally) and a flat picture (all of N in one bin: the contention case the
folding of equal codes is there for).  Apply works in place, so the content is uploaded afresh in front of every burst of BURST launches; the setting keeps
the luma table next to the identity (levels 1: looked up all the same) and takes the whole chroma cast out (balance 1000: offsets that are not zero, so the
chroma plane is read and written).  The series alternate -- one burst of each launch per round -- and a figure is the median over ROUNDS rounds.  Prints one
JSON line per launch, content and size; --once: one round of one launch each."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402

ONCE = "--once" in sys.argv
BURST, ROUNDS = (1, 1) if ONCE else (10, 30)
POINT = dict(brightness=1, hue=1000)  # tools/probe_adjust.py's: an identity table that is looked up all the same, a half-turn of the chroma
AUTO = dict(levels=1, balance=1000, speed=256, reach=127)
STAGES = (("adjust pointwise", E.STAGE_ADJUST_POINT), ("measure", E.STAGE_AUTOLEVEL_MEASURE), ("decide", E.STAGE_AUTOLEVEL_DECIDE), ("apply", E.STAGE_AUTOLEVEL_APPLY))


def series(e, y, uv):
    ms = {name: [] for name, _ in STAGES}
    for _ in range(ROUNDS):
        for name, stage in STAGES:
            e.stage_adjust({}, y, uv)  # (neutral: uploads the planes into slot 0's surfaces and launches nothing)
            ms[name].append(e.time_stage(stage, BURST))
    return ms


for w, h in ((1920, 1080), (3840, 2160)):
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    P = W * H
    rng = np.random.default_rng(w)
    contents = (("noise", rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 200, (H // 2, W), dtype=np.uint8)),
                ("flat", np.full((H, W), 97, np.uint8), np.tile(np.array([110, 140], np.uint8), (H // 2, W // 2))))
    nbytes = {"adjust pointwise": 3 * P, "measure": 3 * P // 2, "decide": 0, "apply": 3 * P}
    e = E.Encoder(w, h, fps=30, fixed_qp=28, adjust=POINT, autolevel=AUTO)
    for content, y, uv in contents:
        series(e, y, uv)  # warm: allocations, code objects
        ms = series(e, y, uv)
        yard = float(np.median(ms["adjust pointwise"]))
        for name, _ in STAGES:
            v = sorted(ms[name])
            med = float(np.median(v))
            r = dict(launch=name, content=content, size="%dx%d" % (w, h), launches=BURST * ROUNDS, us_median=round(1000 * med, 2), us_min=round(1000 * v[0], 2),
                     us_max=round(1000 * v[-1], 2), times_adjust=round(med / yard, 2), algorithmic_bytes=nbytes[name])
            if nbytes[name]:
                r["gb_per_s"] = round(nbytes[name] / (1000 * med) / 1000.0, 1)
            print(json.dumps(r), flush=True)
    e.close()
