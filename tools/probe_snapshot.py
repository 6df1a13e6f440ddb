#!/usr/bin/env python3
"""What a JPEG still costs, measured on the device this runs on; writes profiles/snapshot_price.md (or --out).

  launch   mi355enc_time_stage(16) at 1080p and 2160p for reductions 1 and 4, beside the I420 conversion launch (stage 5) as the yardstick
  host     the Huffman coding of one still (mi355enc_take_snapshot) at those sizes, textured content, quality 75
  stream   a 1080p stream with three pictures in flight and a still every 30th picture, of the source and of the reconstruction, against the same
           stream without stills: alternating fresh processes, three rounds, pictures per second and the ratio
  headline with --parent-tree DIR (a built checkout of the parent commit): bench.py there and here, alternating (the order swaps every round),
           --headline-rounds rounds; the file states the parent's own run-to-run spread, both medians and how many of this tree's runs lie inside it

Every stream figure comes from a child process of its own; nothing here is asserted."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _frames(E, w, h, n=8):
    from ceracoder_amd import synth
    return list(synth.s2_frames(w, h, n))


def launch_and_host(w, h):
    from ceracoder_amd import enc as E
    fr = _frames(E, w, h, 2)
    out = {}
    e = E.Encoder(w, h, fixed_qp=30, gop=60, pipeline_depth=0, exclusive=True)
    try:
        for y, uv in fr:
            e.encode(y, uv)
        out["conversion_us"] = 1e3 * e.time_stage(E.STAGE_CSC_I420, 50)
        for s in (1, 4):
            e.request_snapshot(what=0, reduce=s, quality=75)
            out["launch_us_reduce%d" % s] = 1e3 * e.time_stage(E.STAGE_SNAPSHOT, 50)
            e.encode(*fr[0])  # the request armed this picture (and the stage calls made it an IDR picture)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                data, info = e.take_snapshot()
                ts.append(time.perf_counter() - t0)
            out["huffman_ms_reduce%d" % s] = 1e3 * min(ts)
            out["bytes_reduce%d" % s] = len(data)
    finally:
        e.close()
    return out


def child_stream(what, n=330, warm=30, every=30):
    """prints pictures per second of a 1080p stream at depth 2; what: -1 none, 0 source stills, 1 decoded stills"""
    from ceracoder_amd import enc as E
    w, h = 1920, 1080
    fr = _frames(E, w, h)
    e = E.Encoder(w, h, bitrate_bps=6_000_000, gop=60, pipeline_depth=2, exclusive=True)
    taken = 0
    try:
        t0 = None
        for i in range(n):
            if i == warm:
                t0 = time.perf_counter()
            if what >= 0 and i % every == 0:
                e.request_snapshot(what=what, reduce=4, quality=75)
            e.submit(*fr[i % len(fr)], pts=i)
            if e.pending > 2:
                e.collect(copy=False)
        while e.pending:
            e.collect(copy=False)
        dt = time.perf_counter() - t0
        taken = 1 if e.take_snapshot() is not None else 0
    finally:
        e.close()
    print(json.dumps({"what": what, "fps": (n - warm) / dt, "still_ready": taken}))


def _child(args, cwd=ROOT):
    r = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))  # (nothing more is started after a failure)
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_price.md"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--headline-rounds", type=int, default=8)
    ap.add_argument("--headline-only", action="store_true", help="keep the launch and stream figures of profiles/snapshot_price.md (its JSON block), measure the headline again")
    a = ap.parse_args()
    if a.child is not None:
        return child_stream(a.child)
    if a.headline_only:
        old = open(os.path.join(ROOT, "profiles", "snapshot_price.md")).read()
        res = json.loads(old[old.index("```json") + 7:old.index("```", old.index("```json") + 7)])
        res["headline"] = []
    else:
        res = {"launch": {"%dx%d" % s: launch_and_host(*s) for s in ((1920, 1080), (3840, 2160))}, "stream": [], "headline": []}
    for _ in range(0 if a.headline_only else a.rounds):
        res["stream"].append({k: _child([os.path.abspath(__file__), "--child", str(v)])["fps"] for k, v in (("none", -1), ("source", 0), ("decoded", 1))})
    if a.parent_tree:
        for i in range(a.headline_rounds):
            row = {}
            order = (("parent", a.parent_tree), ("this", ROOT))
            for k, tree in (order if i % 2 == 0 else order[::-1]):
                row[k] = _child(["bench.py", "--gpus", "1", "--steps", "300", "--warmup", "30"], cwd=tree)["value"]
            res["headline"].append(row)
    lines = ["# What a JPEG still costs", "", "Written by tools/probe_snapshot.py (every line of this file); what the figures mean for the design: DESIGN.md section 18.", "",
             "The raw figures:", "", "```json", json.dumps(res, indent=1), "```", ""]
    lines += ["## Launch and host", "", "time_stage(16) times the kernel alone (the 1 KB table is on the device before the loop), 50 launches back to back; the levels go to pinned host memory.", "", "| size | conversion launch (I420), us | still launch reduce 1, us | reduce 4, us | Huffman reduce 1, ms (bytes) | reduce 4, ms (bytes) |", "|---|---|---|---|---|---|"]
    for k, v in res["launch"].items():
        lines.append("| %s | %.1f | %.1f | %.1f | %.2f (%d) | %.2f (%d) |" % (k, v["conversion_us"], v["launch_us_reduce1"], v["launch_us_reduce4"], v["huffman_ms_reduce1"],
                                                                         v["bytes_reduce1"], v["huffman_ms_reduce4"], v["bytes_reduce4"]))
    lines += ["", "## Stream price (1080p, three pictures in flight, a still of reduce 4 every 30th picture)", "", "| round | none, pictures/s | source stills | decoded stills | source / none | decoded / none |", "|---|---|---|---|---|---|"]
    for i, r in enumerate(res["stream"]):
        lines.append("| %d | %.0f | %.0f | %.0f | %.4f | %.4f |" % (i, r["none"], r["source"], r["decoded"], r["source"] / r["none"], r["decoded"] / r["none"]))
    if res["stream"]:
        per = [1e6 * 30 * (1 / r["decoded"] - 1 / r["none"]) for r in res["stream"]]
        lines += ["", "Per armed picture the decoded kind costs %s us of stream time (30 pictures' difference; the metrics launch in the same place: +53 us per picture on record)." % ", ".join("%.0f" % p for p in per)]
    if res["headline"]:
        import statistics
        par, this = [r["parent"] for r in res["headline"]], [r["this"] for r in res["headline"]]
        lo, hi = min(par), max(par)
        inside = sum(lo <= v <= hi for v in this)
        lines += ["", "## Headline (bench.py --gpus 1 --steps 300 --warmup 30, no request made; frames/s)", "",
                  "Alternating fresh processes of the parent commit's tree and this one on one device; the order swaps every round." + (" Measured in a run of its own." if a.headline_only else ""), "", "| round | parent | this |", "|---|---|---|"]
        for i, r in enumerate(res["headline"]):
            lines.append("| %d | %.2f | %.2f |" % (i, r["parent"], r["this"]))
        lines += ["", "The parent's own run-to-run spread: %.2f .. %.2f (%.1f %% of its median %.2f)." % (lo, hi, 100 * (hi - lo) / statistics.median(par), statistics.median(par)),
                  "This tree: %.2f .. %.2f, median %.2f (%+.2f %% against the parent's median); %d of its %d runs lie inside the parent's spread, %d above it, %d below it." % (
                      min(this), max(this), statistics.median(this), 100 * (statistics.median(this) / statistics.median(par) - 1), inside, len(this), sum(v > hi for v in this), sum(v < lo for v in this)),
                  "This tree's median lies %s the parent's spread." % ("inside" if lo <= statistics.median(this) <= hi else "OUTSIDE")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
