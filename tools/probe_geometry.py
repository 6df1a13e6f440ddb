#!/usr/bin/env python3
"""What the input geometry costs: python tools/probe_geometry.py [--iters N] [--out profiles/geometry_price.md]

All launches are timed with mi355enc_time_stage (stage 14: the scale / geometry launch on an NV12 picture, HIP events around back-to-back launches):
- 2160p -> 1080p through the geometry form (full crop, full destination) beside the plain scale launch for the same picture, in one process, alternating
  series; the spread of the plain launch's series is the yardstick for the gap between the two;
- a 1080 x 1920 picture pillarboxed into 1920 x 1080 (mi355enc_fit_rect);
- a 2x upscale, 960 x 540 -> 1920 x 1080, beside the I420 conversion launch of the output size (stage 5), which moves as many output bytes."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E

SERIES = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "geometry_price.md"))
    args = ap.parse_args()
    plain = E.Encoder(1920, 1080, fixed_qp=30, input_size=(3840, 2160))
    geom = E.Encoder(1920, 1080, fixed_qp=30, geometry=E.geometry((3840, 2160), target=(1920, 1080)))
    a, b = [], []
    for _ in range(SERIES):  # alternating
        a.append(plain.time_stage(E.STAGE_SCALE, args.iters))
        b.append(geom.time_stage(E.STAGE_SCALE, args.iters))
    plain.close(); geom.close()
    pillar = E.Encoder(1920, 1080, fixed_qp=30, geometry=E.geometry((1080, 1920), dst=E.fit_rect(1080, 1920, 1920, 1080), keep_sar=True))
    p = [pillar.time_stage(E.STAGE_SCALE, args.iters) for _ in range(3)]
    pillar.close()
    up = E.Encoder(1920, 1080, fixed_qp=30, geometry=E.geometry((960, 540), target=(1920, 1080)))
    u = [up.time_stage(E.STAGE_SCALE, args.iters) for _ in range(3)]
    c = [up.time_stage(E.STAGE_CSC_I420, args.iters) for _ in range(3)]
    up.close()
    med = lambda v: sorted(v)[len(v) // 2]
    spread = max(a) - min(a)
    gap = med(b) - med(a)
    lines = ["# Input geometry: first measurements", "",
             "`tools/probe_geometry.py`: the scale / geometry launch (`mi355enc_time_stage` stage 14, NV12 input) timed with HIP events over %d back-to-back launches "
             "per series." % args.iters, "",
             "## 2160p -> 1080p, full crop and full destination, beside the plain scale launch (%d alternating series each)" % SERIES, "",
             "| launch | median (ms) | best (ms) | worst (ms) |", "|---|---|---|---|",
             "| plain scale (`set_input_size`) | %.4f | %.4f | %.4f |" % (med(a), min(a), max(a)),
             "| geometry (`set_input_geometry`) | %.4f | %.4f | %.4f |" % (med(b), min(b), max(b)), "",
             "Gap of the medians: %+.4f ms; run-to-run spread of the plain launch (worst - best): %.4f ms. Condition (gap <= spread): %s." %
             (gap, spread, "held" if gap <= spread else "NOT held"), "",
             "## Other shapes (best of three series)", "", "| shape | launch (ms) |", "|---|---|",
             "| 1080 x 1920 pillarboxed into 1920 x 1080 (608 x 1080 at x = 656) | %.4f |" % min(p),
             "| 960 x 540 -> 1920 x 1080 (2x upscale) | %.4f |" % min(u),
             "| I420 conversion launch at 1920 x 1080 (stage 5), for scale | %.4f |" % min(c), ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
