"""The inputs of tests/test_extremes_gpu.py really are at the arithmetic limits: every condition below is asserted on the CPU oracle alone, with the
generators and seeds the GPU tests use (tests/extremes.py), so that a kernel can never pass there because its input missed the branch.  Also here:
the host writer on a picture whose every coefficient is +-2047.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from ceracoder_amd import enc as E
from tests import extremes as X
from tests.util import db_picture_sat, random_records

BIG = [g for g in X.GEOMS if g != (16, 16)]  # a single macroblock cannot promise what depends on a draw
ALIGNED = [(64, 48), (176, 144)]            # whole macroblocks: "interior" means what it says


def _rails(a):
    return bool((a == 0).any()) and bool((a == 255).any())


@pytest.mark.parametrize("w,h", X.GEOMS)
def test_sad_surface_reaches_the_top_of_its_u16_lanes(oracle, w, h):
    """16 x 16 blocks of 0 against 255: a SAD of 255 * 256 = 65 280 -- the top of v_qsad_pk_u16_u8's lanes and of select_min's cost << 12 key"""
    (cy, _), (ry, _) = X.sat_pair(w, h, 16)
    surf, _ = oracle.me_frame(cy, ry, 16, 30, threads=4)
    assert int(surf.max()) == 65280
    for kind in X.STRIPE_KINDS + X.SHIFT_KINDS:  # (nothing else may wrap either)
        (cy, _), (ry, _) = X.pair(kind, w, h)
        assert int(oracle.me_frame(cy, ry, 16, 30, threads=4)[0].max()) <= 65280


@pytest.mark.parametrize("w,h", BIG)
@pytest.mark.parametrize("blk", [16, 8])
@pytest.mark.parametrize("t8", [False, True])
def test_level_clamp_fires_and_reconstructions_reach_both_rails(oracle, w, h, blk, t8):
    """QP 0 on blocks of 0 / 255: the quantiser's |level| <= 2047 clamp fires in the intra stage and in the fused P stage (4x4 and 8x8 transform), and the
    reconstructions of the intra, inter and fused P stages hold samples at 0 and at 255 (Clip1 of prediction + residual at both ends)."""
    (cy, cuv), (ry, ruv) = X.sat_pair(w, h, blk)
    surf, imv = X.settled_field(oracle, ("sat", blk), w, h, 0)
    with X.oracle_mode(oracle, t8=t8, i8=t8):
        i_y, i_uv, _, i_lev = oracle.intra_frame(cy, cuv, 0)
        p_y, p_uv, p_mbi, p_lev, _ = oracle.pmb_frame(cy, cuv, ry, ruv, imv, surf, 0, refine=True, threads=4)
        n_y, n_uv, _, n_lev = oracle.inter_frame(cy, cuv, ry, ruv, oracle.imv_to_mbinfo(imv, 0), 0)
    n_i, n_p, n_n = (int((np.abs(l) == 2047).sum()) for l in (i_lev, p_lev, n_lev))
    print("clamped levels", (w, h, blk, t8), "intra", n_i, "fused P", n_p, "inter", n_n)
    assert n_i >= 1 and n_p >= 1 and n_n >= 1
    assert int(np.abs(i_lev).max()) == 2047 and int(np.abs(p_lev).max()) == 2047
    if t8 and blk == 8 and (w, h) == (176, 144):  # ... and in the 8x8 transform's own quantiser (luma levels of macroblocks with NZ_T8)
        is8 = ((p_mbi["nzmask"] >> 27) & 1).astype(bool)
        assert (np.abs(p_lev[is8][:, :256]) == 2047).any()
    for a in (i_y, i_uv, p_y, p_uv, n_y, n_uv):
        assert _rails(a)


def _sixtap(a, axis):
    """E - 5 F + 20 G + 20 H - 5 I + J along `axis` for the position between G and H, unrounded and unclipped (8.4.2.2.1); edges replicated"""
    a = np.asarray(a, np.int64)
    pad = [(0, 0), (0, 0)]
    pad[axis] = (2, 3)
    p = np.pad(a, pad, mode="edge")
    n = a.shape[axis]
    t = [np.take(p, range(k, k + n), axis=axis) for k in range(6)]
    return t[0] - 5 * t[1] + 20 * t[2] + 20 * t[3] - 5 * t[4] + t[5]


@pytest.mark.parametrize("w,h", BIG)
def test_stripes_clip_the_six_tap_filter_both_ways(oracle, w, h):
    """On the stripes references the half-sample planes leave 0 .. 255 before Clip1: b / h (one pass) on both sides for periods 4 and 6 (two samples
    of 255 between zeros: (20 + 20) 255 / 32 = 319; two zeros between 255s: -64) and on one side at least for periods 2 and 3; j (two passes) on both
    sides for every checkerboard of period 3 and up.  j's unrounded intermediate leaves 16 bits everywhere (on both sides for the checkerboards), and over the family it reaches
    its lower bound -(42 * 2550 + 10 * 10710) = -214 200 exactly and goes half as far again as Clip1's 255 << 10 at the top.  The refinement chooses
    fractional vectors on every pair, so those planes are read."""
    j_lo, j_hi = 0, 0
    for kind in X.STRIPE_KINDS:
        _, period, axis = kind
        (cy, _), (ry, _) = X.stripes_pair(w, h, period, axis)
        b1, h1 = _sixtap(ry, 1), _sixtap(ry, 0)
        j1 = _sixtap(b1, 0)
        one = [((p + 16) >> 5) for p, a in ((b1, "v"), (h1, "h")) if axis in (a, "both")]
        lo, hi = min(int(p.min()) for p in one), max(int(p.max()) for p in one)
        assert (lo < 0 and hi > 255) if period >= 4 else (lo < 0 or hi > 255), (kind, lo, hi)
        if axis == "both" and period >= 3 and (w, h) != (50, 34):  # (in 50 x 34 samples a checkerboard of period 3 has too few whole periods)
            jj = (j1 + 512) >> 10
            assert jj.min() < 0 and jj.max() > 255, (kind, int(jj.min()), int(jj.max()))
        assert j1.max() > 32767 and (j1.min() < -32768 or axis != "both"), (kind, int(j1.min()), int(j1.max()))
        j_lo, j_hi = min(j_lo, int(j1.min())), max(j_hi, int(j1.max()))
        if kind == ("stripes", 2, "both"):
            continue  # the current picture is flat grey: every candidate ties
        for qp in (0, 51):
            _, imv = X.settled_field(oracle, kind, w, h, qp)
            out = oracle.subpel_frame(cy, ry, oracle.imv_to_mbinfo(imv, qp), qp, threads=4)
            assert ((out["mvx"] % 4 != 0) | (out["mvy"] % 4 != 0)).any(), (kind, qp)
    print("unrounded centre half sample over the stripes", (w, h), j_lo, j_hi)
    assert j_lo == -(42 * 2550 + 10 * 10710) and j_hi > 3 * (255 << 10) // 2


@pytest.mark.parametrize("w,h", ALIGNED)
@pytest.mark.parametrize("dx,dy", X.SHIFTS)
def test_shifted_pair_puts_the_winner_in_the_corner_of_the_window(oracle, w, h, dx, dy):
    """Every interior macroblock's settled whole-sample vector is (4 dx, 4 dy) = (+-64, +-64) quarter samples; on the pair displaced half a sample further
    the refinement leaves the window: the oracle gives a fractional vector in every interior macroblock (2 of 2 at 64x48, 63 of 63 at 176x144, at QP 0 ..
    51, all four corners) -- at least half of them asserted."""
    mbw, mbh = w // 16, h // 16
    inner = lambda a: a.reshape(mbh, mbw)[1:-1, 1:-1]
    for qp in X.QPS:
        _, imv = X.settled_field(oracle, ("shift", dx, dy, False), w, h, qp)
        assert (inner(imv)["mvx"] == 4 * dx).all() and (inner(imv)["mvy"] == 4 * dy).all(), qp
        (cy, _), (ry, _) = X.shifted(w, h, dx, dy, True)
        _, imv = X.settled_field(oracle, ("shift", dx, dy, True), w, h, qp)
        assert (inner(imv)["mvx"] == 4 * dx).all() and (inner(imv)["mvy"] == 4 * dy).all(), qp
        out = inner(oracle.subpel_frame(cy, ry, oracle.imv_to_mbinfo(imv, qp), qp, threads=4))
        frac = int(((out["mvx"] % 4 != 0) | (out["mvy"] % 4 != 0)).sum())
        assert 2 * frac >= out.size, (qp, frac, out.size)
        assert (np.abs(out["mvx"]) > 64).any()  # beyond the whole-sample window


def _plane_pred_range(p, n):
    """The unclipped extremes of plane prediction (8.3.3.4 for n = 16, 8.3.4.4 for n = 8) over the interior blocks of plane p, from source neighbours"""
    p = p.astype(np.int64)
    lo, hi = 0, 255
    half, (c, sh) = n // 2, ((5, 6) if n == 16 else (34, 6))
    k = np.arange(1, half + 1)
    for y0 in range(n, p.shape[0], n):
        for x0 in range(n, p.shape[1], n):
            top, left, corner = p[y0 - 1, x0:x0 + n], p[y0:y0 + n, x0 - 1], p[y0 - 1, x0 - 1]
            tt, ll = np.concatenate([[corner], top]), np.concatenate([[corner], left])  # index i + 1 = sample i, index 0 = sample -1
            H = int((k * (tt[half + k] - tt[half - k])).sum())
            V = int((k * (ll[half + k] - ll[half - k])).sum())
            a, b, cc = 16 * (left[n - 1] + top[n - 1]), (c * H + 32) >> sh, (c * V + 32) >> sh
            for x, y in ((0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)):
                v = (a + b * (x - (half - 1)) + cc * (y - (half - 1)) + 16) >> 5
                lo, hi = min(lo, int(v)), max(hi, int(v))
    return lo, hi


@pytest.mark.parametrize("w,h", BIG)
def test_ramps_take_plane_prediction_past_both_rails(oracle, w, h):
    """near_sat_ramps: plane prediction extrapolates below 0 and above 255 for Intra_16x16 and for chroma (the analysis computes these candidates for every
    macroblock), and the reconstruction holds samples at both rails; at 176x144 the oracle also chooses the plane modes, and Intra_4x4 / Intra_8x8 occur."""
    cy, cuv = X.ramps(w, h)
    for plane, n in ((cy, 16), (cuv[:, 0::2], 8), (cuv[:, 1::2], 8)):
        lo, hi = _plane_pred_range(plane, n)
        print("plane prediction before Clip1", (w, h, n), lo, hi)
        assert (lo < 0 and hi > 255) if (w, h) == (176, 144) else (lo < 0 or hi > 255), (n, lo, hi)  # (a handful of interior macroblocks: one rail at least)
    y, uv, mbi, _ = oracle.intra_frame(cy, cuv, 30)
    assert _rails(y) and _rails(uv)
    if (w, h) == (176, 144):
        with X.oracle_mode(oracle, i4=False):
            _, _, m16, _ = oracle.intra_frame(cy, cuv, 30)
        assert (m16["i16_mode"] == 3).any() and (m16["chroma_mode"] == 3).any()
        assert (mbi["mb_type"] == 2).any()
        with X.oracle_mode(oracle, t8=True, i8=True):
            _, _, m8, _ = oracle.intra_frame(cy, cuv, 30)
        assert ((m8["mb_type"] == 2) & (((m8["nzmask"] >> 27) & 1) == 1)).any()


@pytest.mark.parametrize("qp", [(10, 51), (40, 51)])
@pytest.mark.parametrize("t8", [0.3, 0.0])
def test_deblocking_filter_lands_on_the_rails(oracle, qp, t8):
    """db_picture_sat with random_records at 11 x 9 macroblocks: at least 50 luma samples and at least 50 chroma samples are changed by the filter and end at 0
    or 255 (the oracle gives 250 .. 400 and 80 .. 100)."""
    mbw, mbh = 11, 9
    y, uv = db_picture_sat(mbw, mbh, X.SEED_DB)
    rec = random_records(mbw, mbh, X.SEED_REC, t8=t8, qp=qp)
    oy, ouv = oracle.deblock_frame(y, uv, rec)
    n_y = int(((oy != y) & ((oy == 0) | (oy == 255))).sum())
    n_uv = int(((ouv != uv) & ((ouv == 0) | (ouv == 255))).sum())
    print("deblocked onto a rail", qp, t8, "luma", n_y, "chroma", n_uv)
    assert n_y >= 50 and n_uv >= 50
    assert ((oy != y) & (oy == 0)).any() and ((oy != y) & (oy == 255)).any() and ((ouv != uv) & (ouv == 0)).any() and ((ouv != uv) & (ouv == 255)).any()


@pytest.mark.parametrize("w,h", ALIGNED)
@pytest.mark.parametrize("qp", [44, 51])
def test_deblocking_filter_saturates_on_coded_saturated_pictures(oracle, w, h, qp):
    """The oracle's own I and P picture of sat_blocks (16) at a high QP: the filter's output holds samples at both rails that it changed (at 176x144)."""
    oe = oracle.Encoder(w, h, gop=60, threads=4, scenecut=False)
    n = 0
    for y, uv in (X.sat_pair(w, h, 16)[1], X.sat_pair(w, h, 16)[0]):
        oe.encode(y[:h, :w], uv[:h // 2, :w], qp)
        n += int(((oe.recon_y != oe.prefilter_y) & ((oe.recon_y == 0) | (oe.recon_y == 255))).sum())
    print("filtered onto a rail", (w, h, qp), n)
    assert n > 0 or (w, h) != (176, 144)


@pytest.mark.parametrize("w,h", X.STREAM_GEOMS)
def test_sat_clip_spans_the_adaptive_quantiser(oracle, w, h):
    """sat_clip: the variance-0 offset (-4), the largest (+4) and at least one more occur among the macroblocks' offsets, and the oracle's encoder with
    adaptive quantisation codes macroblocks at three or more QPs in one picture."""
    mbw, mbh = w // 16, h // 16
    offs = set()
    for y, _ in X.stream_clip(w, h):
        off = np.zeros(mbw * mbh, np.int8)
        oracle.lib().orc_aq_offsets(y.ctypes.data_as(C.c_void_p), w, mbw, mbh, off.ctypes.data_as(C.c_void_p))
        offs |= set(int(o) for o in off)
    flat, noise = np.full((16, 16), 128, np.uint8), np.zeros((16, 16), np.uint8)
    noise[:, 0::2] = 255
    ends = []
    for mb in (flat, noise):
        off = np.zeros(1, np.int8)
        oracle.lib().orc_aq_offsets(mb.ctypes.data_as(C.c_void_p), 16, 1, 1, off.ctypes.data_as(C.c_void_p))
        ends.append(int(off[0]))
    print("adaptive quantisation offsets", (w, h), sorted(offs), "ends", ends)
    assert ends == [-4, 4] and len(offs) >= 3 and ends[0] in offs and ends[1] in offs and max(offs) == ends[1]
    oe = oracle.Encoder(w, h, gop=3, threads=4, aq=True, scenecut=False)
    y, uv = X.stream_clip(w, h)[0]
    oe.encode(y, uv, 26)
    assert len(set(int(q) for q in oe.mbinfo["qp"])) >= 3 and {22, 30} <= set(int(q) for q in oe.mbinfo["qp"])


@pytest.mark.parametrize("w,h", X.STREAM_GEOMS)
@pytest.mark.parametrize("cfg", ["baseline", "preset2", "partitions", "lib"])
def test_streams_decode_and_fit(oracle, w, h, cfg):
    """Every stream the GPU tests encode: the independent decoder reproduces the oracle's reconstruction, every access unit fits mi355enc_max_au_bytes,
    and the stream has what it was built for: levels at the clamp, skipped macroblocks beside saturated ones, reconstruction at both rails."""
    dec = oracle.Decoder()
    clamped = skipped = 0
    for i, (au, key, ry, ruv, mbi, lev) in enumerate(X.oracle_stream(oracle, w, h, cfg)):
        dy, duv = dec.decode(au)
        assert np.array_equal(dy, ry) and np.array_equal(duv, ruv), (cfg, i)
        assert len(au) <= X.max_au_bytes(w, h), (cfg, i, len(au))
        assert key == (i % X.STREAM_GOP == 0)
        assert _rails(ry) and _rails(ruv)
        res = lev.copy()
        if cfg == "partitions":
            res[(mbi["mb_type"] == 1) & (mbi["i16_mode"] != 0), 256:262] = 0  # (vectors of partitions 1 .. 3, not levels)
        res[mbi["mb_type"] == 2, 256:272] = 0                                 # (Intra_4x4 modes)
        clamped += int((np.abs(res) == 2047).sum())
        skipped += int(((mbi["mb_type"] == 1) & (mbi["nzmask"] == 0)).sum()) if not key else 0
    print("stream", (w, h, cfg), "levels at the clamp", clamped, "skipped", skipped, "largest access unit", max(len(s[0]) for s in X.oracle_stream(oracle, w, h, cfg)))
    assert skipped > 0 and (clamped > 0 or (w, h) == (64, 48))


def _all_2047(mbw, mbh, is_idr, rng):
    """records and levels of a picture whose 384 coefficients per macroblock are all +-2047: Intra_16x16 (16 DC + 16 x 15 AC) in an I picture, inter (16 x 16) in a P
    picture, 2 x 4 chroma DC and 8 x 15 chroma AC in both"""
    n = mbw * mbh
    mbi = np.zeros(n, E.MBINFO_DTYPE)
    lev = (rng.integers(0, 2, (n, E.LEVELS_PER_MB)) * 2 - 1).astype(np.int16) * np.int16(2047)
    lev[:, 280:408:16] = 0          # chroma AC blocks carry no coefficient 0
    if is_idr:
        lev[:, 0:256:16] = 0        # nor do Intra_16x16 AC blocks
    else:
        lev[:, 256:272] = 0         # no luma DC block in an inter macroblock
    mbi["mb_type"] = 0 if is_idr else 1
    mbi["i16_mode"] = 2 if is_idr else 0  # DC prediction needs no neighbour
    mbi["qp"] = 26
    mbi["mvx"], mbi["mvy"] = (0, 0) if is_idr else (5, -3)
    mbi["nzmask"] = 0x00FFFFFF | (1 << 25) | (1 << 26) | ((1 << 24) if is_idr else 0)
    return mbi, lev


def _write_case(path, mbw, mbh, is_idr, pic, mbi, lev):
    import struct
    with open(path, "wb") as f:  # the case file of ceracoder_amd/csrc/san_driver.c
        f.write(struct.pack("<10i", mbw, mbh, int(is_idr), pic, 0, 26, 0, 16 * mbw, 16 * mbh, 30))
        f.write(mbi.tobytes())
        f.write(np.ascontiguousarray(lev, np.int16).tobytes())


def test_host_writer_on_pictures_of_nothing_but_clamped_levels(oracle, tmp_path):
    """Every coefficient +-2047, as an I and as a P picture: 384 escape-coded levels of 28 bits are 1344 bytes per macroblock, more than the 1024 per macroblock
    (+ 1024) of the writer's RBSP buffer.  Recorded: pictures of 1 x 1 and 2 x 1 macroblocks fit and are written -- the same bytes on every
    thread count, parsed back by the independent decoder to the same records and levels; the picture of 4 x 3 macroblocks (16 128 bytes against 13 312)
    gets MI355ENC_ERR_OVERFLOW.  The quantiser cannot produce that picture: a 4x4 block's coefficients share the energy of 16 residuals of at most 255, which
    puts one or two of them at the clamp, not sixteen -- the saturated streams of this suite stay under 400 bytes per macroblock and per-sample noise at QP 0
    under 900 -- so the buffer stays as it is.  Whatever the room, nothing is written past it: the bytes behind the caller's room stay as they were, and
    the writer built with the address sanitizer (the stand-alone driver of tests/test_sanitize_cpu.py) runs all three pictures clean."""
    import os
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ceracoder_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "sanitize"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(2047)
    L = E.load()
    for mbw, mbh, fits in ((1, 1, True), (2, 1, True), (4, 3, False)):
        dec = oracle.Decoder()
        hdr = oracle.write_headers(16 * mbw, 16 * mbh, 30)
        for pic, is_idr in enumerate((True, False)):
            mbi, lev = _all_2047(mbw, mbh, is_idr, rng)
            case, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
            _write_case(case, mbw, mbh, is_idr, pic, mbi, lev)
            s = subprocess.run([os.path.join(csrc, "san", "san_asan"), "code", case, outp, "3"], capture_output=True, text=True, timeout=120,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
            assert "ERROR: AddressSanitizer" not in s.stderr and "runtime error" not in s.stderr, s.stderr[-3000:]
            assert s.returncode == (0 if fits else 3), (mbw, mbh, s.returncode, s.stderr[-500:])  # 3: the dense writer returned 0 (out of room)
            rooms = [64, mbw * mbh * 1024]
            if fits:
                au = E.host_write_slice(mbw, mbh, is_idr, pic, 0, 26, mbi, lev)
                print("all +-2047", (mbw, mbh), "I" if is_idr else "P", len(au), "bytes")
                assert mbw * mbh * 1344 <= len(au) <= X.max_au_bytes(16 * mbw, 16 * mbh)
                assert open(outp, "rb").read()[:len(hdr if is_idr else b"") + len(au)] == (E.host_write_headers(16 * mbw, 16 * mbh, 30) if is_idr else b"") + au
                for thr in (1, 2, 3):
                    assert E.host_write_slice_packed(mbw, mbh, is_idr, pic, 0, 26, mbi, lev, threads=thr) == au, thr
                cm, cl = dec.capture(mbw * mbh)
                assert dec.decode((hdr if is_idr else b"") + au) is not None
                for f in ("mb_type", "mvx", "mvy", "qp", "nzmask"):
                    assert np.array_equal(cm[f], mbi[f]), (f, pic)
                assert np.array_equal(cl, lev), (pic, np.argwhere(cl != lev)[:3])
                rooms.append(len(au) - 1)
            else:
                rooms.append(X.max_au_bytes(16 * mbw, 16 * mbh))
            for room in rooms:  # too little room (the caller's or the writer's own): the error, and nothing behind the room is touched
                out, got = np.full(room + 64, 0xA5, np.uint8), C.c_size_t(0)
                r = L.mi355enc_host_write_slice(mbw, mbh, int(is_idr), pic, 0, 26, 0, mbi.ctypes.data_as(C.c_void_p), lev.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.c_void_p), room, C.byref(got))
                assert r == -5, (mbw, mbh, room, r)  # MI355ENC_ERR_OVERFLOW
                assert (out[room:] == 0xA5).all()
