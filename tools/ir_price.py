#!/usr/bin/env python3
"""GPU: what periodic intra refresh (mi355enc_set_intra_refresh, element property intra-refresh) costs against periodic IDR pictures, at 1080p and
2160p, 6 Mbit/s CBR, key-int-max / refresh period 60, S2 clip.  Refresh on and off alternate three times in one process (best of three each):
 (a) pictures/s over whole cycles / GOPs (600 pictures) with three pictures in flight and the device exclusive (sources resident in HBM);
 (b) bytes, PSNR-Y, largest and mean access unit (one pass, host input, reconstruction fetched per picture);
 (c) submit -> collect latency at live pace (60 pictures/s, pipeline_depth 0): p50 / p99;
 (d) the intra macroblocks of P pictures (stage timers on every 4th picture): ms per P picture.
    python tools/ir_price.py [out.md]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from ceracoder_amd import enc as E, synth

lines = []
def say(s=""):
    print(s, flush=True); lines.append(s)

BPS, GOP = 6_000_000, 60
LIB = dict(slices=None, slice_deblock=None)  # the library's (and the element's) defaults: P pictures in slices of about 17 rows, slice-local deblocking

def pic(clip, i):
    k = i % (2 * len(clip) - 2)
    return clip[k if k < len(clip) else 2 * len(clip) - 2 - k]

def speed(w, h, clip, on, n=600):
    bufs = [torch.from_numpy(np.concatenate([y.reshape(-1), uv.reshape(-1)])).cuda() for y, uv in clip]
    torch.cuda.synchronize()
    e = E.Encoder(w, h, fps=60, gop=GOP, bitrate_bps=BPS, pipeline_depth=2, exclusive=True, intra_refresh=on, **LIB)
    def run(cnt, base):
        nb = 0
        for i in range(cnt):
            k = (base + i) % (2 * len(bufs) - 2)
            p = bufs[k if k < len(bufs) else 2 * len(bufs) - 2 - k].data_ptr()
            e.submit_device(p, w, p + w * h, w, pts=base + i)
            if e.pending > 2: nb += e.collect(copy=False)[0]
        while e.pending: nb += e.collect(copy=False)[0]
        return nb
    run(GOP, 0)  # (warm-up: one whole GOP / cycle, so that the timed run starts on a cycle boundary)
    t0 = time.perf_counter(); nb = run(n, GOP); t = time.perf_counter() - t0
    rec = e.stats().recoveries
    e.close()
    assert rec == 0
    return n / t, nb * 8 * 60 / n

def quality(w, h, clip, on, n=240):
    e = E.Encoder(w, h, fps=60, gop=GOP, bitrate_bps=BPS, pipeline_depth=0, intra_refresh=on, **LIB)
    sizes, ps = [], []
    for i in range(n):
        y, uv = pic(clip, i)
        au, _ = e.encode(y, uv, pts=i)
        sizes.append(len(au))
        ps.append(synth.psnr(e.fetch(E.FETCH_RECON_Y)[:h, :w], y))
    e.close()
    s = np.array(sizes[1:], float)
    return sum(sizes), float(np.mean(ps)), int(s.max()), float(s.mean())

def latency(w, h, clip, on, n=240):
    e = E.Encoder(w, h, fps=60, gop=GOP, bitrate_bps=BPS, pipeline_depth=0, intra_refresh=on, **LIB)
    lat, t_next = [], time.perf_counter()
    for i in range(n):
        while time.perf_counter() < t_next: pass
        t_next += 1 / 60
        y, uv = pic(clip, i)
        t0 = time.perf_counter()
        e.encode(y, uv, pts=i)
        lat.append((time.perf_counter() - t0) * 1e3)
    e.close()
    lat = np.array(lat[GOP:])
    return float(np.percentile(lat, 50)), float(np.percentile(lat, 99))

def intra_p(w, h, clip, on, n=240):
    e = E.Encoder(w, h, fps=60, gop=GOP, bitrate_bps=BPS, pipeline_depth=0, profile_events=4, intra_refresh=on, **LIB)
    for i in range(n):
        y, uv = pic(clip, i)
        e.encode(y, uv, pts=i)
    st = e.stats()
    e.close()
    return st.ms_intra_p / max(st.n_inter, 1)

def main():
    if "--one-slice" in sys.argv:
        LIB.update(slices=1, slice_deblock=False)
        sys.argv.remove("--one-slice")
    for w, h in ((1920, 1080), (3840, 2160)):
        clip = list(synth.s2_frames(w, h, 16))
        fps = {True: [], False: []}
        for rnd in range(3):
            for on in (False, True):
                fps[on].append(speed(w, h, clip, on))
        say("## %dx%d, %.0f Mbit/s, period %d, %s" % (w, h, BPS / 1e6, GOP, "P pictures in one slice" if LIB["slices"] == 1 else "default slices"))
        say("")
        say("| | IDR every %d (off) | intra refresh (on) |" % GOP)
        say("|---|---|---|")
        say("| frames/s, whole GOPs / cycles, best of 3 | %.0f | %.0f |" % (max(f for f, _ in fps[False]), max(f for f, _ in fps[True])))
        say("| frames/s, the three runs | %s | %s |" % (" ".join("%.0f" % f for f, _ in fps[False]), " ".join("%.0f" % f for f, _ in fps[True])))
        say("| Mbit/s (CBR pass) | %.2f | %.2f |" % (fps[False][0][1] / 1e6, fps[True][0][1] / 1e6))
        q = {on: quality(w, h, clip, on) for on in (False, True)}
        say("| bytes, 240 pictures | %d | %d |" % (q[False][0], q[True][0]))
        say("| PSNR-Y dB | %.2f | %.2f |" % (q[False][1], q[True][1]))
        say("| largest / mean AU after picture 0, bytes | %d / %.0f | %d / %.0f |" % (q[False][2], q[False][3], q[True][2], q[True][3]))
        lt = {on: latency(w, h, clip, on) for on in (False, True)}
        say("| latency at live pace p50 / p99, ms | %.2f / %.2f | %.2f / %.2f |" % (lt[False] + lt[True]))
        ip = {on: intra_p(w, h, clip, on) for on in (False, True)}
        say("| p_intra_macroblocks, ms per P picture | %.4f | %.4f |" % (ip[False], ip[True]))
        say("| cycle / GOP-weighted ratio on : off | | %.3f |" % (max(f for f, _ in fps[True]) / max(f for f, _ in fps[False])))
        say("")
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")

if __name__ == "__main__":
    main()
