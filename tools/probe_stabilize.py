#!/usr/bin/env python3
"""What electronic image stabilisation costs: python tools/probe_stabilize.py [--iters N] [--out profiles/stabilize_price.md]

All launches are timed with mi355enc_time_stage (HIP events around back-to-back launches), on one handle per shape, in alternating series in one process:
stage 29 (the clear and the projection launch at the input size), stage 30 (the match launch) and, beside them, stage 14 (the geometry launch of the same
handle, which the offset feeds).  Shapes: 2160p -> 1080p and 1080p -> 1080p, each with a margin of 32 samples per side and the default range 16."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E

SERIES = 7
MARGIN = 32
SHAPES = [("2160p -> 1080p", (3840, 2160)), ("1080p -> 1080p", (1920, 1080))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stabilize_price.md"))
    args = ap.parse_args()
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["# Electronic image stabilisation: first measurements", "",
             "`tools/probe_stabilize.py`: `mi355enc_time_stage` with HIP events over %d back-to-back launches per series, %d alternating series per stage on one "
             "handle per shape; margin %d per side, range 16.  Stage 29 is the clear and the projection launch, stage 30 the match launch, stage 14 the geometry "
             "launch of the same handle." % (args.iters, SERIES, MARGIN), ""]
    for name, (iw, ih) in SHAPES:
        e = E.Encoder(1920, 1080, fixed_qp=30, geometry=E.geometry((iw, ih), crop=(MARGIN, MARGIN, iw - 2 * MARGIN, ih - 2 * MARGIN), target=(1920, 1080)),
                      stabilize=dict(range=16, margin=MARGIN))
        t = {14: [], 29: [], 30: []}
        for _ in range(SERIES):
            for st in (E.STAGE_SCALE, E.STAGE_STABILIZE_PROJECT, E.STAGE_STABILIZE_MATCH):
                t[st].append(e.time_stage(st, args.iters))
        e.close()
        both = med(t[29]) + med(t[30])
        lines += ["## %s (input %d x %d)" % (name, iw, ih), "", "| launch | median (ms) | best (ms) | worst (ms) | spread (ms) |", "|---|---|---|---|---|"]
        for st, what in ((29, "clear + projection (stage 29)"), (30, "match (stage 30)"), (14, "geometry (stage 14)")):
            lines.append("| %s | %.4f | %.4f | %.4f | %.4f |" % (what, med(t[st]), min(t[st]), max(t[st]), max(t[st]) - min(t[st])))
        lines += ["", "Projection + match: %.4f ms, %.2f x the geometry launch's own time; the larger of the two is the %s launch." %
                  (both, both / med(t[14]), "projection" if med(t[29]) > med(t[30]) else "match"), ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
