"""The single-stage entry points of the C ABI as one table: per entry point its name and arguments (behind the handle) that pass its own argument checks on
a handle of 72 x 80.  tests/test_stage_frame_cpu.py calls every one of them without a handle, tests/test_stage_frame_gpu.py with pictures in flight.  A new
entry point is one line here."""
import ctypes as C

import numpy as np

W, H = 72, 80          # the handle the arguments are valid for: coded 80 x 80, 5 x 5 macroblocks
STRIDE = 128           # of every caller-owned plane below
BUF_BYTES = 4 << 20    # host memory the arguments point into: inputs in the first half, outputs in eight parts of the second
DEV_BYTES = 1 << 20    # device memory likewise: inputs in the first half, outputs in the second


def entries(E, buf, dev):
    """[(name, arguments, device)] for host memory `buf` (uint8, BUF_BYTES) and the device address `dev` (DEV_BYTES; without a device: any address).
    device: the entry point works on the device, so it is refused with pictures in flight.  The ctypes objects the arguments point to live in the list."""
    assert buf.dtype == np.uint8 and buf.size >= BUF_BYTES and dev % 8 == 0
    i = buf.ctypes.data
    o = [i + BUF_BYTES // 2 + k * (BUF_BYTES // 16) for k in range(8)]
    d, do = dev, [dev + DEV_BYTES // 2, dev + 3 * DEV_BYTES // 4]
    planes, dplanes, strides = (C.c_void_p * 3)(i, i, i), (C.c_void_p * 3)(d, d, d), (C.c_int * 3)(STRIDE, STRIDE, STRIDE)
    q, n = E.Quality(), C.c_size_t(0)
    adj, dn, sty = E.adjust(brightness=100), E.denoise(luma=8, chroma=8), E.overlay_style()
    img = E.image_layer(np.full((4, 4, 4), 200, np.uint8), 2, 2)
    snap = (W, H, 1, 75)  # w, ht, reduce, quality
    return [
        ("mi355enc_stage_me", (i, i, 26, o[0], o[1]), True),
        ("mi355enc_stage_me_select", (i, i, 26, o[0]), True),
        ("mi355enc_stage_me_select_next", (i, i, i, 26, o[0]), True),
        ("mi355enc_stage_subpel", (i, i, 26, o[0]), True),
        ("mi355enc_stage_inter", (i, i, i, i, 26, o[0], o[1], o[2], o[3]), True),
        ("mi355enc_stage_pmb", (i, i, i, i, 26, 0, 1, i, i, None, 0, o[0], o[1], o[2], o[3]), True),
        ("mi355enc_stage_intra", (i, i, 26, 0, o[0], o[1], o[2], o[3]), True),
        ("mi355enc_stage_intra_analyse", (i, i, 26, o[0], o[1]), True),
        ("mi355enc_stage_deblock", (o[0], o[1], i), True),
        ("mi355enc_stage_quality", (i, i, i, i, C.byref(q)), True),
        ("mi355enc_stage_quality_device", (d, d, STRIDE, d, d, C.byref(q)), True),
        ("mi355enc_stage_csc", (E.FMT_I420, planes, strides, o[0], o[1]), True),
        ("mi355enc_stage_csc_device", (E.FMT_I420, dplanes, strides, do[0], do[1]), True),
        ("mi355enc_stage_scale", (E.FMT_NV12, planes, strides, o[0], o[1]), True),
        ("mi355enc_stage_geometry", (E.FMT_NV12, planes, strides, o[0], o[1]), True),
        ("mi355enc_stage_yuv_convert", (o[0], o[1]), True),
        ("mi355enc_stage_adjust", (C.byref(adj), o[0], o[1]), True),
        ("mi355enc_stage_denoise", (C.byref(dn), i, i, o[0], o[1], o[2], o[3]), True),
        ("mi355enc_stage_denoise_search", (C.byref(dn), 4, i, i, o[0]), True),
        ("mi355enc_stage_denoise_mc", (C.byref(dn), 4, i, i, o[0], o[1], o[2], o[3], o[4]), True),
        ("mi355enc_stage_jpeg", (i, 64, o[0], o[1]), True),
        ("mi355enc_stage_jpeg_blocks", (2, 1, 3, i, i, o[0], o[1]), True),
        ("mi355enc_stage_orient", (E.ORIENT_90R, i, STRIDE, i, STRIDE, o[0], o[1]), True),
        ("mi355enc_stage_orient_device", (E.ORIENT_90R, d, STRIDE, d, STRIDE, do[0], do[1]), True),
        ("mi355enc_stage_overlay", (b"stage", C.byref(sty), o[0], o[1]), True),
        ("mi355enc_stage_image", (C.byref(img), 1, o[0], o[1]), True),
        ("mi355enc_stage_snapshot_blocks", (i, STRIDE, i, STRIDE) + snap + (o[0], o[1]), True),
        ("mi355enc_stage_snapshot_blocks_device", (d, STRIDE, d, STRIDE) + snap + (o[0], o[1]), True),
        ("mi355enc_stage_snapshot", (i, STRIDE, i, STRIDE) + snap + (o[0], BUF_BYTES // 16, C.byref(n)), True),
        ("mi355enc_stage_rate", (128, i, i, i, i, o[0], o[1]), True),
        ("mi355enc_stage_set_slice_rows", (0,), False),      # (what the stage entry points use: a setting of the handle, no device work)
        ("mi355enc_stage_set_slice_deblock", (0,), False),
    ]
