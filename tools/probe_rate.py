"""The frame-rate conversion's mix launch alone: mi355enc_time_stage 18 at a few sizes, with the bytes the launch moves."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402

for w, h in ((1280, 720), (1920, 1080), (3840, 2160)):
    e = E.Encoder(w, h, fps=30, fixed_qp=28, pipeline_depth=1, rate=(E.RATE_BLEND, 10 ** 9, 1))
    e.time_stage(E.STAGE_RATE, 20)  # warm
    ms = sorted(e.time_stage(E.STAGE_RATE, 200) for _ in range(5))
    picture = e.mbw * e.mbh * 384
    print(json.dumps({"size": "%dx%d" % (w, h), "ms_median": round(ms[2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[4], 4),
                      "bytes": 3 * picture, "GB_per_s": round(3 * picture / ms[2] / 1e6, 1)}))
    e.close()
