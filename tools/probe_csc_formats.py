#!/usr/bin/env python3
"""The conversion launch of every input format that has one, old and new, at 1080p and 2160p on device-resident input (no upload in the
timed part): python tools/probe_csc_formats.py [--iters N] [--host-fps]

Meant to run under `rocprofv3 --kernel-trace --stats`, which gives each kernel's mean time; the table printed here is the host's view
(a synchronising call per launch: launch-bound, a cross-check only) with the algorithmic bytes per picture the trace rows are divided by:
what the format holds per pixel plus 1.5 bytes of NV12 written.  --host-fps: host-input pictures per second of 1080p BGRx against
1080p NV12 through submit / collect (PCIe carries 8.3 MB against 3.1 MB per picture).  --yuv [--out FILE]: the colour step and the launches of the 10-bit
and grey formats alone at 1080p, beside csc_kernel's I420 launch in the same run, timed with HIP events; FILE: the table as markdown."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ceracoder_amd import enc as E

# name, format, bytes per pixel read, plane shapes as (rows per picture row, bytes per pixel column)
FORMATS = [("I420", E.FMT_I420, 1.5, [(1, 1), (.5, .5), (.5, .5)]), ("YUY2", E.FMT_YUY2, 2, [(1, 2)]), ("UYVY", E.FMT_UYVY, 2, [(1, 2)]),
           ("Y42B", E.FMT_Y42B, 2, [(1, 1), (1, .5), (1, .5)]), ("Y444", E.FMT_Y444, 3, [(1, 1), (1, 1), (1, 1)]), ("YV12", E.FMT_YV12, 1.5, [(1, 1), (.5, .5), (.5, .5)]),
           ("NV21", E.FMT_NV21, 1.5, [(1, 1), (.5, 1)]), ("BGRx", E.FMT_BGRX, 4, [(1, 4)]), ("RGBx", E.FMT_RGBX, 4, [(1, 4)]), ("xRGB", E.FMT_XRGB, 4, [(1, 4)]),
           ("xBGR", E.FMT_XBGR, 4, [(1, 4)]), ("BGR", E.FMT_BGR, 3, [(1, 3)]), ("RGB", E.FMT_RGB, 3, [(1, 3)])]


def kernels(args):
    for (w, h) in ((1920, 1080), (3840, 2160)):
        e = E.Encoder(w, h, fixed_qp=30)
        W, H = e.mbw * 16, e.mbh * 16
        oy, ouv = torch.empty(H * W, dtype=torch.uint8, device="cuda"), torch.empty(H // 2 * W, dtype=torch.uint8, device="cuda")
        for name, fmt, bpp, shapes in FORMATS:
            planes, strides = [], []
            for rows, cols in shapes:
                stride = (int(w * cols) + 15) & ~15
                planes.append(torch.randint(0, 256, (int(h * rows) * stride,), dtype=torch.uint8, device="cuda"))
                strides.append(stride)
            ptrs = [p.data_ptr() for p in planes]
            for _ in range(20):  # warm: code object loaded, the planes resident in the Infinity Cache
                e.stage_csc_device(fmt, ptrs, strides, oy.data_ptr(), ouv.data_ptr())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                e.stage_csc_device(fmt, ptrs, strides, oy.data_ptr(), ouv.data_ptr())
            dt = (time.perf_counter() - t0) / args.iters
            print("%dx%d %-4s fmt %2d: %.1f B/pixel in + 1.5 out = %.2f MB per picture; %.1f us per synchronised launch (host clock)"
                  % (w, h, name, fmt, bpp, (bpp + 1.5) * w * h / 1e6, dt * 1e6), flush=True)
        e.close()


def host_fps(args):
    w, h, n = 1920, 1080, 600
    rng = np.random.default_rng(1)
    for name, fmt, planes in (("NV12", E.FMT_NV12, [rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)]),
                              ("BGRx", E.FMT_BGRX, [rng.integers(0, 256, (h, 4 * w), dtype=np.uint8)])):
        for rep in range(3):
            e = E.Encoder(w, h, fixed_qp=36, pipeline_depth=2, exclusive=True, slices=None, slice_deblock=None)
            for i in range(n + 60):
                if i == 60:
                    t0 = time.perf_counter()
                e.submit_fmt(fmt, planes, pts=i)
                if e.pending > 2:
                    e.collect(copy=False)
            while e.pending:
                e.collect(copy=False)
            dt = time.perf_counter() - t0
            print("host input 1080p %s (pageable memory, pipeline_depth 2, the same picture every time): %.0f pictures/s (run %d)" % (name, n / dt, rep), flush=True)
            e.close()


DEEP = [("P010", E.FMT_P010, 3.0, [(1, 2), (.5, 2)]), ("I420_10", E.FMT_I420_10, 3.0, [(1, 2), (.5, 1), (.5, 1)]), ("v210", E.FMT_V210, 8 / 3, [(1, 8 / 3)]), ("GRAY8", E.FMT_GRAY8, 1.0, [(1, 1)])]


def _launch_us(e, hip, fmt, w, h, shapes, oy, ouv, iters):
    """mean time of a synchronising stage_csc_device call, host clock: the launch and its wait, the same overhead for every row, the I420 row included"""
    import ctypes as C
    bufs, strides = [], []
    rng = np.random.default_rng(fmt)
    for rows, cols in shapes:
        stride = (int(np.ceil(w * cols)) + 15) & ~15
        host = rng.integers(0, 256, int(h * rows) * stride, dtype=np.uint8)
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(host.nbytes)) == 0 and hip.hipMemcpy(d, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) == 0
        bufs.append(d.value)
        strides.append(stride)
    for _ in range(20):
        e.stage_csc_device(fmt, bufs, strides, oy, ouv)
    t0 = time.perf_counter()
    for _ in range(iters):
        e.stage_csc_device(fmt, bufs, strides, oy, ouv)
    dt = (time.perf_counter() - t0) / iters * 1e6
    for d in bufs:
        hip.hipFree(C.c_void_p(d))
    return dt


def yuv(args):
    w, h = 1920, 1080
    e = E.Encoder(w, h, fixed_qp=30, colorimetry=(0, 1, 1, 1), input_colorimetry=(1, 6))
    W, H = e.mbw * 16, e.mbh * 16
    rows = []
    # HIP events around back-to-back launches on the handle's stream: the kernels alone
    i420 = 1e3 * e.time_stage(E.STAGE_CSC_I420, args.iters)
    step = 1e3 * e.time_stage(E.STAGE_YUV_CONVERT, args.iters)
    rows.append(("csc_kernel I420 (yardstick)", "events", 1.5, 1.5, i420))
    rows.append(("colour step (yuv_convert_kernel)", "events", 1.5, 1.5, step))
    # a synchronising call per launch (host clock: launch-bound, comparable among themselves)
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")  # (the runtime the library itself runs on)
    out = []
    for n in (H * W, H // 2 * W):
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(n)) == 0
        out.append(d.value)
    for name, fmt, bpp, shapes in [("I420", E.FMT_I420, 1.5, [(1, 1), (.5, .5), (.5, .5)])] + DEEP:
        rows.append(("%s launch" % name, "host", bpp, 1.5, _launch_us(e, hip, fmt, w, h, shapes, out[0], out[1], args.iters)))
    e.close()
    lines = ["| launch (1080p) | clock | bytes/pixel in | out | us |", "|---|---|---|---|---|"]
    lines += ["| %s | %s | %.2f | %.1f | %.1f |" % r for r in rows]
    lines += ["", "colour step / I420 conversion launch (events): %.2f" % (step / i420)]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-fps", action="store_true")
    ap.add_argument("--yuv", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    yuv(a) if a.yuv else host_fps(a) if a.host_fps else kernels(a)
