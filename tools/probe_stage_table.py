#!/usr/bin/env python3
"""Every stage of mi355enc_time_stage at 1920 x 1080, for comparing two builds of the library (dev tool; profiles/stage_table_check.md).

    MI355ENC_LIB=<build> python tools/probe_stage_table.py run <label> [n]  one process, one JSON line: {"label": ..., "ms": {stage: average ms over n launches}}
    python tools/probe_stage_table.py report <lines.jsonl> <parent> <new>   the table: per stage the parent's runs, its min .. max widened by its own spread
                                                                            (max - min) on both sides, this build's median, and whether it lies inside

A stage runs on the handle that has what it needs: a plain one, one with an input size, an input colorimetry, blend-mode rate conversion, an image on layer 0,
picture controls and the noise filter with a range, or one with HDR input.  Each handle has coded an IDR and a P picture first."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, ITERS, NS = 1920, 1080, 20, 10 ** 9


def run(label, iters=ITERS):
    import numpy as np
    from ceracoder_amd import enc as E, synth
    kw = dict(gop=60, fixed_qp=30, pipeline_depth=2)
    plain = E.Encoder(W, H, **kw)
    conf = E.Encoder(W, H, colorimetry=(0, 1, 1, 1), input_colorimetry=(1, 6), input_size=(2560, 1440), rate=(2, NS, 2), adjust=dict(brightness=100, saturation=1300),
                     denoise=dict(luma=8, chroma=8, motion=8), **kw)
    conf.set_image(0, np.random.default_rng(1).integers(0, 256, (128, 256, 4), dtype=np.uint8), 64, 64, 200)
    hdr = E.Encoder(W, H, colorimetry=(0, 1, 1, 1), hdr_input=(E.HDR_PQ, 0, 1000, 100), **kw)
    for e in (plain, conf, hdr):
        for i, (y, uv) in enumerate(synth.s2_frames(*e.input_size, 2)):
            if e is hdr:
                e.submit_fmt(E.FMT_P010, [y.astype("<u2") << 8, uv.astype("<u2") << 8], pts=i * NS // 60)
            else:
                e.submit(y, uv, pts=i * NS // 60)
        while e.pending:
            e.collect()
    ms = {}
    for s in range(29):
        e = hdr if E.STAGE_HDR_P010 <= s <= E.STAGE_DEEP_P010 else conf if s in (E.STAGE_SCALE, E.STAGE_IMAGE, E.STAGE_YUV_CONVERT, E.STAGE_RATE) or s >= 23 else plain
        if s in (E.STAGE_ADJUST_POINT, E.STAGE_ADJUST_SHARPEN):
            conf.set_adjust(dict(brightness=100, saturation=1300, sharpen=16 if s == E.STAGE_ADJUST_SHARPEN else 0))
        ms[s] = e.time_stage(s, iters)
    print(json.dumps({"label": label, "iters": iters, "ms": ms}), flush=True)
    for e in (plain, conf, hdr):
        e.close()


def report(path, parent, new):
    runs = {parent: [], new: []}
    for line in open(path):
        if line.startswith("{"):
            d = json.loads(line)
            runs[d["label"]].append(d["ms"])
    print("| stage | %s runs (ms) | accepted (ms) | %s runs (ms) | %s median | inside |\n|---|---|---|---|---|---|" % (parent, new, new))
    bad = []
    for s in map(str, range(29)):
        p, n = [r[s] for r in runs[parent]], [r[s] for r in runs[new]]
        lo, hi, med = min(p) - (max(p) - min(p)), max(p) + (max(p) - min(p)), statistics.median(n)
        if not lo <= med <= hi:
            bad.append(s)
        fmt = lambda v: " ".join("%.4f" % x for x in v)
        print("| %s | %s | %.4f .. %.4f | %s | %.4f | %s |" % (s, fmt(p), lo, hi, fmt(n), med, "yes" if lo <= med <= hi else "**no**"))
    print("\noutside: %s" % (", ".join(bad) or "none"))


if __name__ == "__main__":
    run(sys.argv[2], *map(int, sys.argv[3:4])) if sys.argv[1] == "run" else report(*sys.argv[2:5])
