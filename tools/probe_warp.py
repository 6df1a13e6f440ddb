#!/usr/bin/env python3
"""What lens, roll and keystone correction costs: python tools/probe_warp.py [--iters N] [--out profiles/warp_price.md]

All launches are timed with mi355enc_time_stage (HIP events around back-to-back launches) on one handle per size, in alternating series in one process:
stage 31 (the warp set last, on slot 0's surfaces) under several settings and, beside it, stage 13 (the orientation launch, 90r: the same 1.5 P in and 1.5 P
out, this project's yardstick for a picture copied once).  Settings: barrel with both filters, a roll of 30 degrees, a shrink (zoom 2.5 at 1080p; 2 at 2160p, where 2.5 would put nodes left of the mesh's range; most tiles direct); barrel
and the roll also with staging switched off (mi355enc_debug_warp_staging), which is what the staged form has to beat."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E

SERIES = 7
SIZES = [("1080p", (1920, 1080), 163840), ("2160p", (3840, 2160), 131072)]  # (name, size, the shrink's zoom)
BARREL, ROLL30, SHRINK = dict(k1=-13107, k2=1966), dict(cos=56756, sin=32768), dict()
CASES = [  # (name, filter, parameters, staging)
    ("barrel, bicubic", 1, BARREL, True), ("barrel, bicubic, staging off", 1, BARREL, False), ("barrel, bilinear", 0, BARREL, True),
    ("roll 30 degrees, bicubic", 1, ROLL30, True), ("roll 30 degrees, bicubic, staging off", 1, ROLL30, False),
    ("shrink, bicubic", 1, SHRINK, True), ("shrink, bicubic, staging off", 1, SHRINK, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "warp_price.md"))
    args = ap.parse_args()
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["# Lens, roll and keystone correction: first measurements", "",
             "`tools/probe_warp.py`: `mi355enc_time_stage` with HIP events over %d back-to-back launches per series, %d alternating series per row on one handle per "
             "size.  Stage 31 is the warp launch (both planes, margin included), stage 13 the orientation launch (90r) of the same handle.  `staged / direct` are "
             "`mi355enc_warp_plan`'s counts of 32 x 32 tiles; with staging off every tile takes the direct form." % (args.iters, SERIES), ""]
    for name, (w, h), zoom in SIZES:
        SHRINK["zoom"] = zoom
        e = E.Encoder(w, h, fixed_qp=30)
        t = {c[0]: [] for c in CASES}
        t["orientation 90r (stage 13)"] = []
        plans = {}
        for _ in range(SERIES):
            t["orientation 90r (stage 13)"].append(e.time_stage(E.STAGE_ORIENT, args.iters))
            for cname, kind, p, staging in CASES:
                e.set_warp(dict(kind=kind), **p)
                e.debug_warp_staging(staging)
                t[cname].append(e.time_stage(E.STAGE_WARP, args.iters))
                plans[cname] = E.warp_plan(E.warp_build(w, h, **p), w, h)
        e.close()
        ref = med(t["orientation 90r (stage 13)"])
        lines += ["## %s (%d x %d; the shrink's zoom: %.1f)" % (name, w, h, zoom / 65536.0), "", "| launch | staged / direct | median (ms) | best (ms) | worst (ms) | spread (ms) | x stage 13 |", "|---|---|---|---|---|---|---|"]
        for cname in ["orientation 90r (stage 13)"] + [c[0] for c in CASES]:
            v = t[cname]
            lines.append("| %s | %s | %.4f | %.4f | %.4f | %.4f | %.2f |" % (cname, "%d / %d" % plans[cname] if cname in plans else "", med(v), min(v), max(v), max(v) - min(v), med(v) / ref))
        for a in ("barrel, bicubic", "roll 30 degrees, bicubic", "shrink, bicubic"):
            on, off = t[a], t[a + ", staging off"]
            lines.append("")
            lines.append("%s: staged %.4f ms against %.4f ms with staging off, a difference of %+.4f ms; the two series' spreads are %.4f and %.4f ms." %
                         (a, med(on), med(off), med(on) - med(off), max(on) - min(on), max(off) - min(off)))
        lines.append("")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
