"""GPU: every way an NV12 picture reaches the encoder unscaled, against the oracle's stream of the clean visible pictures.

The pictures lie in containers of tests/inputref.py: everything around the visible samples is poison that differs from edge replication,
fresh for every picture, and every picture of a stream lies at another address than the one before it (a ring of containers).  Every case
compares the access units byte for byte, the keyframe flags, and the encoder's final reconstruction with oracle.Decoder's over the whole
stream.  tests/test_input_paths_cpu.py shows on the oracle alone that reading the poison instead of replicating changes the IDR picture and
the first P picture of every padded geometry used here: the evidence that these cases are sensitive to what a kernel reads.

  a  mi355enc_submit_device, read in place (width a multiple of 16, equal strides that are multiples of 16, 16-byte aligned addresses)
  b  the same through every toolset, so that every kernel instance that addresses ctx->src_y / src_uv / src_stride / vis_h is visited:
       default        me_kernel (current macroblock rows by scalar loads, and the padded copy d_psrc for the next picture's search),
                      subpel refinement + pmb_preload / pmb_mb (k_motion.hip), chroma_block (kernels_common.hpp), copy_luma_kernel (I pictures),
                      intra_analyse_mb in intra_analyse_kernel and intra_analyse_gated_kernel, intra_rows_kernel's prefetch and intra_compute
                      (intra_mb.hpp), and -- the clip has flashes, so P pictures carry intra macroblocks -- ip_src / intra_p_row (intra_p_kernel)
       aq             aq_kernel (k_handover.hip)
       intra_in_p=2   intra_p_row's Intra_4x4 branch
       t8 + i8x8      pmb_luma_t8, and intra_rows_kernel<true> (a build of its own) with i8_tq8
       t8 = 2         pmb_pick_t8's instance of pmb_mb
       partitions     the partition search's instance of pmb_mb
       intra_mode 1   intra_kernel (one launch per diagonal, replayed from a graph: the context is read from device memory)
       intra_mode 2   intra_band_kernel (its own source prefetch)
       deblock_mode 1 the per-diagonal deblocker's graph beside the in-place source (replays must see this picture's context)
       no graphs      the same launches issued directly
       no subpel      pmb_kernel without the refinement's source reads
       intra refresh  pmb_mb / intra_p_row with forced columns
       single_stream  all kernels of a picture on one stream (no front stream that could outlive collect())
       exclusive      the bench's configuration: kernels waiting for each other on the device, three pictures in flight
       one slice      slices=1, slice_deblock=False (one slice per P picture, the filter across slice boundaries): row_has_top() of the
                      source aprons differs
     (k_inter.hip's two-kernel form is not on the stream path: out of scope)
  c  mi355enc_submit_device through its copy (odd address / stride, y_stride != uv_stride) and through pad_kernel (width not a multiple of 16)
  d  host rows with a stride larger than the width: hipMemcpy2DAsync at depth 0, the staged pieces at depths 1 and 2 with the helper
     threads on and off (MI355ENC_NO_STAGE_THREADS, read when the encoder is opened)
  e  pinned memory transferred in place
  f  ownership: a ring of exactly depth + 1 containers, each overwritten with new poison the moment collect() has returned its picture
  g  recovery (one injected trip) re-reads the caller's buffers of the pictures in flight
  h  refused calls (ERR_ARG, ERR_STATE) leave no trace in the stream

Toolsets the oracle's encoder has no switch for (transform8x8 = 2, intra refresh) are compared with a second encoder fed the same pictures
through contiguous host submit -- the path tests/test_t8_adaptive_gpu.py and tests/test_intra_refresh_gpu.py pin -- and with the decoder.

Scene-cut detection (on by default in the library, and the oracle applies the same rule) is off on both sides: its decision lands a number of
pictures later that depends on the pipeline depth, so one expected stream per geometry could not serve every depth, and it has nothing to do
with how a picture is addressed.  Everything else mirrors mi355enc_default_cfg.

Case d switches the helper threads with MI355ENC_NO_STAGE_THREADS (ceracoder_amd/csrc/enc_handle.cpp reads it when an encoder is opened).  The
handle exposes no flag that says which variant ran: if that variable is ever renamed, both parametrisations run the threaded path and this
file must follow the rename.

No case provokes a fault: every address handed to the library lies inside an allocation with at least 4096 bytes of guard on both sides.
What this cannot see: a read beyond the documented extent that does not change the result (a value loaded and never used)."""
import ctypes as C

import numpy as np
import pytest

from tests import inputref as R
from tests.util import flash_clip

pytestmark = pytest.mark.gpu

GOP = 4
QPS = R.QPS
LIBRARY_DEFAULTS = dict(slices=None, slice_deblock=None, scenecut=False)

# name -> lib: Encoder arguments on top of the library's defaults; stream: the toolset whose stream it must produce; orc: how the oracle is told
# (None: no oracle switch -- a second encoder through contiguous host submit)
TOOLS = {
    "default": dict(lib={}, orc={}),
    "aq": dict(lib=dict(aq=True), orc=dict(aq=True)),
    "i4p": dict(lib=dict(intra_in_p=2), orc=dict(feat="F_I4P")),
    "t8i8": dict(lib=dict(transform8x8=1, i8x8=True), orc=dict(t8=True, i8=True)),
    "t8adaptive": dict(lib=dict(transform8x8=2), orc=None),
    "partitions": dict(lib=dict(partitions=True), orc=dict(feat="F_PART")),
    "intra_mode1": dict(lib=dict(intra_mode=1), stream="default"),
    "intra_mode2": dict(lib=dict(intra_mode=2), stream="default"),
    "deblock_mode1": dict(lib=dict(deblock_mode=1), stream="default"),
    "no_graphs": dict(lib=dict(use_graphs=False), stream="default"),
    "no_subpel": dict(lib=dict(subpel=False), orc=dict(subpel=False)),
    "intra_refresh": dict(lib=dict(intra_refresh=True), orc=None),
    "single_stream": dict(lib=dict(single_stream=True), stream="default"),
    "exclusive": dict(lib=dict(exclusive=True), stream="default"),
    "one_slice": dict(lib=dict(slices=1, slice_deblock=False), orc=dict(one_slice=True)),
}


def n_of(w, h):
    return 3 if (w, h) == (3840, 2160) else 9  # (nine pictures: two whole GOPs and the IDR picture of a third)


def lib_kwargs(tool):
    kw = dict(LIBRARY_DEFAULTS)
    kw.update(TOOLS[tool]["lib"])
    return kw


_clips, _streams = {}, {}


def clip_of(w, h):
    if (w, h) not in _clips:
        _clips[(w, h)] = flash_clip(w, h, n_of(w, h))
    return _clips[(w, h)]


@pytest.fixture(scope="module")
def expected(E, oracle):
    """expected(w, h, tool) -> [(access unit, keyframe)] of the clean visible pictures; made once per geometry and stream"""
    def get(w, h, tool, force_idr_at=()):
        tool = TOOLS[tool].get("stream", tool)
        key = (w, h, tool) + tuple(force_idr_at)
        if key in _streams:
            return _streams[key]
        clip, orc = clip_of(w, h), TOOLS[tool]["orc"]
        out = []
        if orc is None:
            e = E.Encoder(w, h, gop=GOP, fixed_qp=30, **lib_kwargs(tool))
            for i, (y, uv) in enumerate(clip):
                e.set_fixed_qp(QPS[i % len(QPS)])
                out.append(e.encode(np.ascontiguousarray(y), np.ascontiguousarray(uv), pts=i, force_idr=i in force_idr_at))
            e.close()
        else:
            oracle.set_features(oracle.F_ALL | (getattr(oracle, orc["feat"]) if "feat" in orc else 0))
            oracle.set_transform8x8(orc.get("t8", False))
            oracle.set_i8x8(orc.get("i8", False))
            try:
                one = orc.get("one_slice", False)
                ns = 1 if one else oracle.auto_slices((h + 15) // 16)
                oe = oracle.Encoder(w, h, gop=GOP, threads=16, aq=orc.get("aq", False), intra_slices=0, p_slices=ns, slice_deblock_local=not one,
                                    scenecut=False, subpel=orc.get("subpel", True))
                for i, (y, uv) in enumerate(clip):
                    out.append(oe.encode(y, uv, QPS[i % len(QPS)], force_idr=i in force_idr_at))
                oe.close()
            finally:
                oracle.set_features(oracle.F_ALL)
                oracle.set_transform8x8(False)
                oracle.set_i8x8(False)
        _streams[key] = out
        return out
    return get


def check(E, oracle, e, got, want, recoveries=0):
    """got: collect()'s tuples in order.  Access units, keyframe flags, and the decoder's last picture against the encoder's reconstruction."""
    assert [g[2] for g in got] == list(range(len(want))), "one access unit per picture, in order"
    for i, (g, wnt) in enumerate(zip(got, want)):
        assert g[1] == wnt[1], ("keyframe flag", i)
        assert g[0] == wnt[0], ("access unit", i, len(g[0]), len(wnt[0]))
    dec = oracle.Decoder()
    for g in got:
        dy, duv = dec.decode(g[0])
    ry, ruv = e.fetch(E.FETCH_RECON_Y), e.fetch(E.FETCH_RECON_UV)
    assert np.array_equal(dy, ry[:dy.shape[0], :dy.shape[1]]) and np.array_equal(duv, ruv[:duv.shape[0], :duv.shape[1]]), "decoder against the reconstruction"
    st = e.stats()
    assert st.recoveries == recoveries and (recoveries or st.last_error_word == 0)


def drive(e, n, depth, feed, collected=None, before=None):
    got = []

    def take():
        got.append(e.collect())
        if collected:
            collected(len(got) - 1)
    for i in range(n):
        e.set_fixed_qp(QPS[i % len(QPS)])
        if before:
            before(i)
        feed(i)
        if e.pending > depth:
            take()
    while e.pending:
        take()
    return got


class DeviceRing:
    """`slots` device containers of one geometry; put(i) uploads picture i's container (poison of its own) into slot i % slots"""

    def __init__(self, clip, stride, layout, slots, uv_stride=None, offset=0):
        self.clip, self.stride, self.uv_stride, self.layout, self.offset = clip, stride, uv_stride or stride, layout, offset
        self.ptr, self.size = [], None
        for k in range(slots):
            buf, self.yo, self.uo = self.host(k)
            self.size = buf.nbytes
            self.ptr.append(R.device_container(buf))
        assert len(set(self.ptr)) == slots

    def host(self, i):
        y, uv = self.clip[i % len(self.clip)]
        return R.container(y, uv, self.stride, layout=self.layout, seed=1000 + 7 * i, uv_stride=self.uv_stride, offset=self.offset)

    def put(self, i):
        buf, yo, uo = self.host(i)
        assert (buf.nbytes, yo, uo) == (self.size, self.yo, self.uo)
        d = self.ptr[i % len(self.ptr)]
        assert R.hip().hipMemcpy(C.c_void_p(d), buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.nbytes), 1) == 0
        return d + yo, d + uo

    def submit(self, e, i, **kw):
        py, puv = self.put(i)
        e.submit_device(py, self.stride, puv, self.uv_stride, pts=i, **kw)

    def poison(self, i):
        R.device_overwrite(self.ptr[i % len(self.ptr)], self.size, 5000 + i)

    def free(self):
        for d in self.ptr:
            R.device_free(d)
        self.ptr = []


def device_case(E, oracle, expected, w, h, stride, layout, depth, tool="default", own=False, uv_stride=None, offset=0, direct=None, **extra):
    clip, n = clip_of(w, h), n_of(w, h)
    want = expected(w, h, tool)
    if direct is not None:  # which branch of mi355enc_submit_device the case is there for (include/mi355enc.h)
        us = uv_stride or stride
        assert direct == (w % 16 == 0 and stride == us and stride % 16 == 0 and offset % 16 == 0)
    ring = DeviceRing(clip, stride, layout, depth + 1 if own else depth + 2, uv_stride, offset)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=30, pipeline_depth=depth, **dict(lib_kwargs(tool), **extra))
    try:
        got = drive(e, n, depth, lambda i: ring.submit(e, i), collected=ring.poison if own else None)
        check(E, oracle, e, got, want)
    finally:
        e.close()
        ring.free()


# ---- a. in place, device
def _a_cases():
    out = []
    for w, h in [(1280, 720), (320, 180), (64, 48), (16, 16)]:
        W = (w + 15) // 16 * 16
        out += [(w, h, s, lay) for s in (W, W + 16, W + 64) for lay in ("bench", "apart", "uv_first")] + [(w, h, 2 * W, "interleaved_rows")]
    out += [(1920, 1080, s, "bench") for s in (1920, 1936, 1984)] + [(1920, 1080, 1984, "apart"), (1920, 1080, 1984, "uv_first"), (1920, 1080, 3840, "interleaved_rows")]
    return out


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("w,h,stride,layout", _a_cases())
def test_a_device_input_in_place(E, oracle, expected, w, h, stride, layout, depth):
    device_case(E, oracle, expected, w, h, stride, layout, depth, direct=True)


def test_a_device_input_in_place_2160p(E, oracle, expected):
    device_case(E, oracle, expected, 3840, 2160, 3840 + 64, "bench", 2, direct=True)


# ---- b. in place, every kernel that reads the source
def _b_cases():
    out = []
    for tool in TOOLS:
        out.append((320, 180, tool, 2 if tool == "exclusive" else 0))
    out += [(320, 180, "default", 2), (1920, 1080, "aq", 0), (1920, 1080, "t8i8", 0), (1920, 1080, "exclusive", 2)]
    return out


@pytest.mark.parametrize("w,h,tool,depth", _b_cases())
def test_b_in_place_through_every_toolset(E, oracle, expected, w, h, tool, depth):
    device_case(E, oracle, expected, w, h, w + 64, "bench", depth, tool=tool, direct=True)


def test_b_the_clip_puts_intra_macroblocks_into_p_pictures(E, expected):
    """(what makes case b visit intra_p_kernel: after the in-place stream's last P picture the records hold intra macroblocks)"""
    w, h = 320, 180
    clip = clip_of(w, h)
    ring = DeviceRing(clip, w + 64, "bench", 2)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=30, **lib_kwargs("default"))
    try:
        intra = 0
        for i in range(6):  # picture 5: a P picture that is a flash
            ring.submit(e, i)
            key = e.collect()[1]
            if not key:
                intra = max(intra, int((e.fetch(E.FETCH_MBINFO)["mb_type"] != 1).sum()))
        assert intra > 0
    finally:
        e.close()
        ring.free()


# ---- c. copied, device
C_CASES = [
    dict(w=320, h=180, stride=323, layout="apart", offset=1),                 # an odd address and stride w + 3: the device-to-device copy
    dict(w=320, h=180, stride=336, layout="apart", uv_stride=384),            # y_stride != uv_stride, both multiples of 16: the copy
    dict(w=322, h=182, stride=336, layout="bench"),                           # the copy and pad_kernel
    dict(w=50, h=34, stride=64, layout="bench"),
]


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("case", C_CASES, ids=lambda c: "%dx%d-%d" % (c["w"], c["h"], c["stride"]))
def test_c_device_input_copied(E, oracle, expected, case, depth):
    device_case(E, oracle, expected, depth=depth, direct=False, **case)


# ---- d. host rows with a stride larger than the width
def host_views(clip, i, w, h, kind):
    """picture i of the clip as strided views: rows w + 2 or w + 64 apart, or a window of a taller and wider array"""
    y, uv = clip[i]
    if kind == "window":
        g = np.random.default_rng(900 + i)
        big_y, big_uv = g.integers(0, 256, (h + 11, w + 70), dtype=np.uint8), g.integers(0, 256, (h // 2 + 7, w + 38), dtype=np.uint8)
        vy, vuv = big_y[5:5 + h, 33:33 + w], big_uv[3:3 + h // 2, 9:9 + w]
        vy[:], vuv[:] = y, uv
        return vy, vuv
    stride = w + (2 if kind == "w+2" else 64)
    buf, yo, uo = R.container(y, uv, stride, layout="apart", seed=2000 + i)
    return R.visible(buf, yo, h, w, stride), R.visible(buf, uo, h // 2, w, stride)


@pytest.mark.parametrize("mode", ["encode", "submit0", "submit1", "submit2", "submit1-nothreads", "submit2-nothreads"])
@pytest.mark.parametrize("kind", ["w+2", "w+64", "window"])
@pytest.mark.parametrize("w,h", [(322, 182), (1920, 1080), (18, 18)])
def test_d_host_rows_with_a_stride(E, oracle, expected, monkeypatch, w, h, kind, mode):
    """depth 0: hipMemcpy2DAsync from pageable memory; depths 1 and 2: stage_piece's row loop, three pieces on the caller's thread
    (MI355ENC_NO_STAGE_THREADS) or six shared with the helper threads"""
    clip, n, want = clip_of(w, h), n_of(w, h), expected(w, h, "default")
    depth = 0 if mode == "encode" else int(mode[6])
    if mode.endswith("nothreads"):
        monkeypatch.setenv("MI355ENC_NO_STAGE_THREADS", "1")
    else:
        monkeypatch.delenv("MI355ENC_NO_STAGE_THREADS", raising=False)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=30, pipeline_depth=depth, **lib_kwargs("default"))
    keep = []
    try:
        if mode == "encode":
            got = []
            for i in range(n):
                e.set_fixed_qp(QPS[i % len(QPS)])
                vy, vuv = host_views(clip, i, w, h, kind)
                assert vy.strides[0] > w and not vy.flags["C_CONTIGUOUS"]
                au, key = e.encode(vy, vuv, pts=i)
                got.append((au, key, i, QPS[i % len(QPS)]))
        else:
            def feed(i):
                vy, vuv = host_views(clip, i, w, h, kind)
                keep.append((vy, vuv))
                del keep[:-4]
                e.submit(vy, vuv, pts=i)
            got = drive(e, n, depth, feed)
        assert e.stats().pinned_inputs == 0
        check(E, oracle, e, got, want)
    finally:
        e.close()


# ---- e. pinned memory, transferred in place
class PinnedRing:
    def __init__(self, E, clip, stride, layout, slots):
        self.clip, self.stride, self.layout = clip, stride, layout
        b, self.yo, self.uo = self.host(0)
        self.size = (b.nbytes + 4095) // 4096 * 4096
        self.buf = E.PinnedBuffer(slots * self.size)
        self.slots = slots

    def host(self, i):
        y, uv = self.clip[i % len(self.clip)]
        return R.container(y, uv, self.stride, layout=self.layout, seed=3000 + 7 * i)

    def slot(self, i):
        k = i % self.slots
        return self.buf.array[k * self.size:(k + 1) * self.size]

    def submit(self, e, i):
        b, yo, uo = self.host(i)
        s = self.slot(i)
        s[:b.nbytes] = b
        (h, w) = self.clip[0][0].shape
        e.submit(R.visible(s, yo, h, w, self.stride), R.visible(s, uo, h // 2, w, self.stride), pts=i)

    def poison(self, i):
        self.slot(i)[:] = R.noise(self.size, 7000 + i)  # written from the host


def pinned_case(E, oracle, expected, w, h, stride, layout, depth, own=False):
    clip, n, want = clip_of(w, h), n_of(w, h), expected(w, h, "default")
    ring = PinnedRing(E, clip, stride, layout, depth + 1)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=30, pipeline_depth=depth, **lib_kwargs("default"))
    try:
        got = drive(e, n, depth, lambda i: ring.submit(e, i), collected=ring.poison if own else None)
        assert e.stats().pinned_inputs == n
        check(E, oracle, e, got, want)
    finally:
        e.close()
        ring.buf.free()


E_CASES = [(1920, 1080, 1920, "bench"), (1920, 1080, 1984, "apart"), (322, 182, 322, "bench"), (322, 182, 324, "apart"), (320, 180, 320, "bench"), (320, 180, 384, "uv_first")]


@pytest.mark.parametrize("depth", [0, 1, 2])
@pytest.mark.parametrize("w,h,stride,layout", E_CASES)
def test_e_pinned_input(E, oracle, expected, w, h, stride, layout, depth):
    """stride == w in the "bench" layout: one contiguous NV12 picture; otherwise strided"""
    pinned_case(E, oracle, expected, w, h, stride, layout, depth)


# ---- f. ownership: the caller's memory is the caller's again when collect() has returned
F_DEVICE = [dict(w=1920, h=1080, stride=1920, layout="bench"), dict(w=1920, h=1080, stride=1984, layout="bench"), dict(w=1280, h=720, stride=1296, layout="uv_first"),
            dict(w=320, h=180, stride=384, layout="bench"), dict(w=64, h=48, stride=128, layout="interleaved_rows"), dict(w=16, h=16, stride=16, layout="bench")] + C_CASES


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("case", F_DEVICE, ids=lambda c: "%dx%d-%d-%s%s" % (c["w"], c["h"], c["stride"], c["layout"], "-uv%d" % c["uv_stride"] if "uv_stride" in c else ""))
def test_f_device_containers_are_overwritten_after_collect(E, oracle, expected, case, depth):
    """the search of picture i + 1 runs against the encoder's copy of picture i's luma (d_psrc), never the caller's buffer: that buffer is noise by then"""
    device_case(E, oracle, expected, depth=depth, own=True, **case)


@pytest.mark.parametrize("exclusive", [False, True])
def test_f_device_containers_overwritten_in_the_bench_configuration(E, oracle, expected, exclusive):
    device_case(E, oracle, expected, 1920, 1080, 1920, "bench", 2, tool="exclusive" if exclusive else "single_stream", own=True)


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("w,h,stride,layout", E_CASES)
def test_f_pinned_containers_are_overwritten_after_collect(E, oracle, expected, w, h, stride, layout, depth):
    pinned_case(E, oracle, expected, w, h, stride, layout, depth, own=True)


# ---- g. recovery with in-place input
def test_g_recovery_reads_the_callers_buffers_again(E, oracle, expected):
    """One injected trip (as tests/test_recovery_gpu.py does it) between two submits at depth 2: the pictures in flight are re-encoded from the
    caller's containers, which are still valid (a ring of depth + 1; poisoned only after their collect()).  The QP changes with every picture:
    a re-encoded picture keeps the QP it was submitted under (recover() used to code it at the QP in force when it ran -- found by this case)."""
    w, h, depth = 320, 180, 2
    clip, n = clip_of(w, h), n_of(w, h)
    ring = DeviceRing(clip, w + 64, "bench", depth + 1)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=30, pipeline_depth=depth, **lib_kwargs("exclusive"))
    try:
        got = drive(e, n, depth, lambda i: ring.submit(e, i), collected=ring.poison, before=lambda i: e.debug_trip_wait(12) if i == 5 else None)
        st = e.stats()
        assert st.recoveries == 1 and st.last_error_word == 12 and st.safe_level == 1
        # the whole stream is the oracle's of the clean clip with an IDR picture forced where the first picture in flight was re-encoded: the
        # re-enqueued pictures 5, 6 and 7 were read again from the caller's containers, at the caller's stride
        check(E, oracle, e, got, expected(w, h, "default", force_idr_at=(5,)), recoveries=1)
        assert [i for i, g in enumerate(got) if g[1]] == [0, 4, 5]
    finally:
        e.close()
        ring.free()


# ---- h. the argument contract
def test_h_refused_calls_leave_no_trace(E, oracle, expected):
    w, h, depth = 64, 48, 1
    clip, n, want = clip_of(w, h), n_of(w, h), expected(w, h, "default")
    ring = DeviceRing(clip, w + 16, "apart", depth + 2)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=30, pipeline_depth=depth, **lib_kwargs("default"))
    hy, huv = np.ascontiguousarray(clip[0][0]), np.ascontiguousarray(clip[0][1])
    vp = C.c_void_p

    def refusals(i):
        py, puv = ring.ptr[i % 3] + ring.yo, ring.ptr[i % 3] + ring.uo
        L, s = e.L, ring.stride
        assert L.mi355enc_submit_device(e.h, vp(py), w - 1, vp(puv), s, 99, 0) == E.ERR_ARG
        assert L.mi355enc_submit_device(e.h, vp(py), s, vp(puv), w - 16, 99, 0) == E.ERR_ARG
        assert L.mi355enc_submit_device(e.h, None, s, vp(puv), s, 99, 0) == E.ERR_ARG
        assert L.mi355enc_submit_device(e.h, vp(py), s, None, s, 99, 0) == E.ERR_ARG
        assert L.mi355enc_submit(e.h, vp(hy.ctypes.data), w - 1, vp(huv.ctypes.data), w, 99, 1) == E.ERR_ARG
        assert L.mi355enc_submit(e.h, vp(hy.ctypes.data), w, vp(huv.ctypes.data), w - 2, 99, 1) == E.ERR_ARG
        assert L.mi355enc_submit(e.h, None, w, vp(huv.ctypes.data), w, 99, 1) == E.ERR_ARG
        assert L.mi355enc_submit(e.h, vp(hy.ctypes.data), w, None, w, 99, 1) == E.ERR_ARG
    try:
        got = []
        for i in range(n):
            e.set_fixed_qp(QPS[i % len(QPS)])
            pending = e.pending
            refusals(i)
            assert e.pending == pending
            ring.submit(e, i)
            if e.pending == depth + 1:  # full: one more is refused, by either entry point, and nothing changes
                py, puv = ring.ptr[(i + 1) % 3] + ring.yo, ring.ptr[(i + 1) % 3] + ring.uo
                assert e.L.mi355enc_submit_device(e.h, vp(py), ring.stride, vp(puv), ring.stride, 99, 1) == E.ERR_STATE
                assert e.L.mi355enc_submit(e.h, vp(hy.ctypes.data), w, vp(huv.ctypes.data), w, 99, 1) == E.ERR_STATE
                assert e.pending == depth + 1
                got.append(e.collect())
        while e.pending:
            got.append(e.collect())
        check(E, oracle, e, got, want)
    finally:
        e.close()
        ring.free()
