"""Input containers for the input-path tests (tests/test_input_paths_cpu.py, tests/test_input_paths_gpu.py): a visible w x h NV12 picture
placed inside a larger block of memory in which every byte that is not a visible sample is poison -- seeded noise that is checked to differ
from what edge replication would put in its place, so that a kernel that reads a row or a column it must not read cannot produce the right
stream by coincidence.  The numpy part needs no device; the device helpers go through the HIP runtime by ctypes."""
import ctypes as C

import numpy as np

LAYOUTS = ("bench", "apart", "uv_first", "interleaved_rows")
QPS = [30, 24, 40, 26, 33, 51, 10, 28, 36]  # per picture, low and high mixed: the GPU cases and the CPU sensitivity evidence code the same stream
MIN_GUARD = 4096  # bytes of poison in front of the first and behind the last plane, whatever the stride


def _r16(v):
    return (v + 15) // 16 * 16


def noise(nbytes, seed):
    """nbytes of seeded noise"""
    return np.random.default_rng(seed).integers(0, 256, int(nbytes), dtype=np.uint8)


def visible(buf, off, rows, w, stride):
    """the rows x w samples of a plane that starts at byte `off` of `buf` (a view)"""
    return np.lib.stride_tricks.as_strided(buf[off:], (rows, w), (stride, 1))


def coded_read(buf, off, rows, cols, stride):
    """what a reader without any clamp takes for a rows x cols plane at `off`: the container's bytes as they lie (a copy)"""
    idx = off + np.arange(rows)[:, None] * stride + np.arange(cols)[None, :]
    return buf[idx]


def assert_poisoned(buf, y_off, uv_off, y, uv, stride, uv_stride=None):
    """Every row of the container below the visible height of a plane (down to the coded height) differs from the plane's last visible row,
    and in every visible row the bytes [w, stride) differ from the replicated last sample (chroma: the last Cb, Cr pair)."""
    uv_stride = uv_stride or stride
    h, w = y.shape
    H = _r16(h)
    for off, p, rows, coded, st in ((y_off, y, h, H, stride), (uv_off, uv, h // 2, H // 2, uv_stride)):
        for r in range(rows, coded):
            below = buf[off + r * st:off + r * st + w]
            assert not np.array_equal(below, p[rows - 1]), "the row %d below a plane of %d rows equals its last row" % (r, rows)
        if st > w:
            tail = visible(buf, off + w, rows, st - w, st)
            if p is y:
                rep = np.broadcast_to(p[:, w - 1:w], tail.shape)
            else:
                rep = np.tile(p[:, w - 2:w], (1, (st - w + 1) // 2))[:, :st - w]
            same = (tail == rep).all(axis=1)
            assert not same.any(), "row %d: the bytes behind the visible width equal the replicated last sample" % int(np.argmax(same))


def container(y, uv, stride, guard_rows=16, layout="bench", seed=0, uv_stride=None, offset=0):
    """-> (buf, y_off, uv_off): `buf` (uint8, one dimension) holds the picture's planes with rows `stride` (chroma: `uv_stride`, default the same)
    bytes apart, the first plane `offset` bytes behind a 16-byte boundary; everything else is noise from `seed`.
      "bench"            the chroma plane starts at luma row h (bench.py's buffer)
      "apart"            guard_rows rows of poison between and around the planes
      "uv_first"         like "apart", the chroma plane at the lower address
      "interleaved_rows" like "apart" with stride >= 2 * w: every second line of w bytes is poison
    guard_rows >= 16, so that the rows a reader without a clamp would take below a plane lie inside the container.  Asserts assert_poisoned()."""
    assert layout in LAYOUTS and guard_rows >= 16
    h, w = y.shape
    assert uv.shape == (h // 2, w) and stride >= w
    uv_stride = uv_stride or stride
    assert uv_stride >= w
    if layout == "interleaved_rows":
        assert stride >= 2 * w and uv_stride >= 2 * w
    if layout == "bench":
        assert uv_stride == stride
    guard = _r16(max(guard_rows * max(stride, uv_stride), MIN_GUARD))
    ysz, csz = _r16(h * stride), _r16((h // 2) * uv_stride)
    if layout == "bench":
        y_off = guard + offset
        uv_off, end = y_off + h * stride, guard + offset + h * stride + csz
    elif layout == "uv_first":
        uv_off = guard + offset
        y_off = guard + csz + guard + offset
        end = y_off + ysz
    else:
        y_off = guard + offset
        uv_off = guard + ysz + guard + offset
        end = uv_off + csz
    buf = noise(_r16(end) + guard, seed)
    visible(buf, y_off, h, w, stride)[:] = y
    visible(buf, uv_off, h // 2, w, uv_stride)[:] = uv
    assert_poisoned(buf, y_off, uv_off, y, uv, stride, uv_stride)
    return buf, y_off, uv_off


# ---- device memory
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so.7")  # (the runtime the library itself runs on)
    return _hip


def device_planes(E, host, rows, cols, stride, offset):
    """`host` (rows x cols per plane, in order) copied into one hipMalloc'd buffer at `stride` from byte `offset` on; -> (buffer, plane pointers)"""
    hip = C.CDLL("libamdhip64.so.7")  # (the runtime the library itself runs on; a handle of its own, returned to the caller: moved here unchanged)
    size = offset + sum(r * stride for r in rows)
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(size)) == 0
    ptrs, o = [], offset
    for a, r, w in zip(host, rows, cols):
        a = np.ascontiguousarray(a)
        assert hip.hipMemcpy2D(C.c_void_p(buf.value + o), C.c_size_t(stride), a.ctypes.data_as(C.c_void_p), C.c_size_t(w), C.c_size_t(w),
                               C.c_size_t(r), 1) == 0  # hipMemcpyHostToDevice
        ptrs.append(buf.value + o)
        o += r * stride
    return hip, buf, ptrs


def device_container(buf):
    """a whole container in device memory, uploaded in one hipMemcpy; -> its device address (hipMalloc: 256-byte aligned)"""
    buf = np.ascontiguousarray(buf)
    d = C.c_void_p()
    assert hip().hipMalloc(C.byref(d), C.c_size_t(buf.nbytes)) == 0
    assert hip().hipMemcpy(d, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.nbytes), 1) == 0  # hipMemcpyHostToDevice, synchronous
    return d.value


def device_overwrite(dptr, nbytes, seed):
    """the whole device container at `dptr` overwritten with new poison (a synchronous hipMemcpy)"""
    fresh = noise(nbytes, seed)
    assert hip().hipMemcpy(C.c_void_p(dptr), fresh.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes), 1) == 0


def device_free(dptr):
    assert hip().hipFree(C.c_void_p(dptr)) == 0
