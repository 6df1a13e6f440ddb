"""The HDR tone map's conversion launch alone: mi355enc_time_stage 19 / 20 / 21 (P010, I420_10, v210) beside 22 (csc_deep_kernel<P010>, the
plain 10 -> 8 bit launch) at 1080p and 2160p, HIP events over 200 launches.  The launch reads the slot's raw staging buffer, which a stage_csc call in front
fills: with uniform noise over the whole code range (every gather goes somewhere else: the worst case for the tables) or with a smooth ramp plus a little noise
(what pictures look like).  MI355ENC_LIB=<another build of the library> times that build (tools/build_variant.sh hdrglobal k_hdr.hip -DHDR_TABLES_GLOBAL: the tables
gathered from global memory instead of staged into LDS); --once: a launch or two per case, for a kernel trace; --1080p: that size only."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E  # noqa: E402

E.LIB_PATH = os.environ.get("MI355ENC_LIB", E.LIB_PATH)
ONCE = "--once" in sys.argv
SIZES = ((1920, 1080),) if "--1080p" in sys.argv else ((1920, 1080), (3840, 2160))
V210_Y = ((0, 10), (1, 0), (1, 20), (2, 10), (3, 0), (3, 20))
V210_C = ((0, 0), (0, 20), (1, 10), (2, 0), (2, 20), (3, 10))


def picture(w, h, content, rng):
    """10-bit Y (h, w), Cb, Cr (h / 2, w / 2)"""
    if content == "noise":
        return rng.integers(0, 1024, (h, w)), rng.integers(0, 1024, (h // 2, w // 2)), rng.integers(0, 1024, (h // 2, w // 2))
    y = 64 + (np.add.outer(np.arange(h) * 300 // h, np.arange(w) * 560 // w) + rng.integers(0, 12, (h, w)))
    c = [512 + (np.add.outer(np.arange(h // 2) * k // h, np.arange(w // 2) * 160 // w) - 60 + rng.integers(0, 8, (h // 2, w // 2))) for k in (120, -90)]
    return y, c[0], c[1]


def planes_of(fmt, y, cb, cr):
    h, w = y.shape
    words = lambda a, sh: np.ascontiguousarray((a.astype(np.int64) << sh).astype("<u2"))
    if fmt == E.FMT_P010:
        return [words(y, 6), words(np.stack([cb, cr], 2).reshape(h // 2, w), 6)]
    if fmt == E.FMT_I420_10:
        return [words(y, 0), words(cb, 0), words(cr, 0)]
    g = (w + 5) // 6
    yy, cc = np.zeros((h, 6 * g), np.int64), np.zeros((h, 3 * g, 2), np.int64)
    yy[:, :w] = y
    cc[:, :w // 2, 0], cc[:, :w // 2, 1] = np.repeat(cb, 2, 0), np.repeat(cr, 2, 0)
    yy, cc, out = yy.reshape(h, g, 6), cc.reshape(h, g, 6), np.zeros((h, g, 4), np.int64)
    for k in range(6):
        out[:, :, V210_Y[k][0]] |= yy[:, :, k] << V210_Y[k][1]
        out[:, :, V210_C[k][0]] |= cc[:, :, k] << V210_C[k][1]
    return [np.ascontiguousarray(out.astype("<u4")).view(np.uint8).reshape(h, 16 * g)]


CASES = ((E.STAGE_HDR_P010, E.FMT_P010, "hdr P010"), (E.STAGE_HDR_I420_10, E.FMT_I420_10, "hdr I420_10"), (E.STAGE_HDR_V210, E.FMT_V210, "hdr v210"),
         (E.STAGE_DEEP_P010, E.FMT_P010, "plain P010"))
for w, h in SIZES:
    rng = np.random.default_rng(w)
    pics = {c: picture(w, h, c, rng) for c in ("ramp", "noise")}
    for transfer, tname in ((E.HDR_PQ, "pq"), (E.HDR_HLG, "hlg")):
        e = E.Encoder(w, h, fps=30, fixed_qp=28, colorimetry=(0, 1, 1, 1), hdr_input=(transfer, 0, 1000, 203))
        for stage, fmt, name in CASES:
            if stage == E.STAGE_DEEP_P010 and transfer != E.HDR_PQ:
                continue
            for content in ("ramp", "noise"):
                e.stage_csc(fmt, planes_of(fmt, *pics[content]))  # (leaves the picture's planes in the raw staging buffer, rows at multiples of 16 bytes)
                if ONCE:
                    e.time_stage(stage, 1)
                    continue
                e.time_stage(stage, 20)  # warm
                ms = sorted(e.time_stage(stage, 200) for _ in range(5))
                print(json.dumps({"lib": os.path.basename(E.LIB_PATH), "size": "%dx%d" % (w, h), "launch": name, "transfer": tname if stage != E.STAGE_DEEP_P010 else "-",
                                  "content": content, "ms_median": round(ms[2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[4], 4)}), flush=True)
        e.close()
