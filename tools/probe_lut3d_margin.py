"""What the 3D LUT's margin rule costs (rule 6): mi355enc_time_stage 35 at 1920 x 1080 (eight margin rows, no margin column) and at
854 x 480 (ten margin columns, no margin row), N = 33, both launch forms, on seeded noise.  HIP events around 10 back-to-back launches, the content uploaded
afresh in front of every burst, 30 rounds, one burst of each form per round; prints one JSON line per size and form.  The library is the one MI355ENC_LIB
names (ceracoder_amd/enc.py), so the same script measures two builds in alternating processes:

    for i in 1 2 3; do MI355ENC_LIB=<parent build>/libmi355enc.so python tools/probe_lut3d_margin.py; python tools/probe_lut3d_margin.py; done"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402

BURST, ROUNDS, N = 10, 30, 33
nodes = np.random.default_rng(N).integers(0, 1 << 30, N ** 3, dtype=np.uint32)
for w, h in ((1920, 1080), (854, 480)):
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    rng = np.random.default_rng(w)
    y, uv = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
    e = E.Encoder(w, h, fps=30, fixed_qp=28)
    e.set_lut3d(nodes)
    ms = {0: [], 1: []}
    for r in range(ROUNDS + 2):  # (two rounds to warm: allocations, code objects)
        for form in (0, 1):
            e.debug_lut3d_form(form)
            e.stage_adjust({}, y, uv)  # (neutral: uploads the planes into slot 0's surfaces and launches nothing)
            t = e.time_stage(E.STAGE_LUT3D, BURST)
            if r >= 2:
                ms[form].append(t)
    for form in (0, 1):
        v = sorted(ms[form])
        print(json.dumps(dict(lib=os.environ.get("MI355ENC_LIB", "tree"), size="%dx%d" % (w, h), form="staged" if form else "direct", us_median=round(1000 * float(np.median(v)), 2),
                              us_min=round(1000 * v[0], 2), us_max=round(1000 * v[-1], 2))), flush=True)
    e.close()
