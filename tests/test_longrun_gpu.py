"""GPU: state that outlives a picture (DESIGN.md "State that outlives a picture").  The kernels that wait for each other on the device synchronise through
words that are never cleared: tagged with the handle's picture epoch, or compared with counts that only grow.  A live stream reaches the wrap of every one of
them -- the 20-bit tag of the intra rows' progress words after 4 h 51 min, the row counts' sign bit within a week -- and no other test runs more than a few
hundred pictures on a handle.  mi355enc_debug_set_counters puts a handle where such a run would have put it, tagged buffers and all: two pictures (IDR + P)
first, so that the buffers hold real stale content, then the preset, then a clip in whose middle the boundary falls.

Neither the epoch nor the counts enter the bit stream, so the reference is the oracle's encoder on the same clip: every access unit, the reconstruction and
the oracle's decoder on every access unit, all held with ==.  Besides that every stream test asserts: no recovery and a zero error word (a wrong comparison at
a boundary is a wait that runs into its bound, or a wait that passes on a stale word); that the boundary was crossed inside the clip; and that the count it is
about moved by exactly what the schedule books per picture -- a schedule that fell back to stream order (another encoder open in the process, a safe level, a
size threshold) fails the test instead of passing it idle."""
import functools
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from tests.spsref import slice_headers
from tests.util import cut_clip, first_diff, frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M32 = 0xFFFFFFFF
QP = 30
N, PRE, GOP = 12, 2, 4   # pictures per clip; those in front of the preset (IDR + P); pictures 4, 8 are IDR pictures: P, P, I, P, P, P, I, P, P, P follow the preset
CROSS = 4                # the boundary falls on / behind the fifth picture after the preset (picture 6, a P picture; picture 7 is one too, picture 8 an IDR picture)
# The scene cut of the clips that need intra macroblocks in P pictures: from picture 5 on every picture is fresh noise.  The S2 pictures in front of it carry
# intra macroblocks in most rows as well, so the P pictures before the boundary (2, 3), on it (6), behind it (7) and two pictures behind it (9) all do -- only
# the cut picture itself codes none (noise predicts noise no worse than a flat block does).  (With the cut behind the boundary the pictures AT the boundary
# would be S2's alone; with it here the words whose tags wrap are polled for both kinds of content.)
CUT = 5
EPOCHS = {"tag20": 0xFFFFF - 5, "sign": 0x7FFFFFFF - 5, "inv1": 0xFFFFFFFE - 5, "wrap": 0xFFFFFFFF - 5}
SLICINGS = {"library": dict(slices=None, slice_deblock=None), "mirror": {}, "two": dict(slices=2, slice_deblock=True)}


def _next_epoch(e, n=1):
    for _ in range(n):
        e = (e + 1) & M32 or 1   # fill_ctx: if (++h->epoch == 0) h->epoch = 1
    return e


def _crossed(kind, a, b):
    """the value went from a to b numerically past the boundary of its kind"""
    if kind == "tag20":
        return (b & 0xFFFFF) < (a & 0xFFFFF)
    if kind == "sign":
        return a < 0x80000000 <= b
    return b < a   # 2^32 (and the epoch's 0xFFFFFFFF -> 1)


@functools.lru_cache(maxsize=None)
def _clip(w, h, kind):
    if kind == "cut":
        return cut_clip(w, h, N, CUT)
    return [(y, uv) for _, _, y, uv in frames(w, h, N)]


_ORACLE = {}


def _oracle_stream(oracle, w, h, kind, slicing, gop, iip, aq, force=()):
    """the oracle's stream of a clip, computed once per configuration: access units, key flags, last reconstruction, and per picture the macroblock rows that
    hold intra macroblocks"""
    key = (w, h, kind, slicing, gop, iip, aq, force)
    if key not in _ORACLE:
        mbh = (h + 15) // 16
        kw = SLICINGS[slicing]
        if slicing == "library":
            okw = dict(p_slices=oracle.auto_slices(mbh), slice_deblock_local=True)
        else:
            okw = dict(p_slices=kw.get("slices", 1), slice_deblock_local=bool(kw.get("slice_deblock", False)))
        oracle.set_features(oracle.F_ALL | (oracle.F_I4P if iip == 2 else 0))
        try:
            oe = oracle.Encoder(w, h, gop=gop, threads=16, aq=aq, scenecut=False, **okw)
            dec = oracle.Decoder()
            aus, keys, rows = [], [], []
            for i, (y, uv) in enumerate(_clip(w, h, kind)):
                au, k = oe.encode(y, uv, QP, force_idr=i in force)
                dy, duv = dec.decode(au)
                assert np.array_equal(dy, oe.recon_y) and np.array_equal(duv, oe.recon_uv), i
                aus.append(au); keys.append(k)
                rows.append(set(np.flatnonzero((oe.mbinfo["mb_type"].reshape(oe.mbh, oe.mbw) != 1).any(axis=1)).tolist()))
            _ORACLE[key] = dict(aus=aus, keys=keys, rows=rows, rec_y=oe.recon_y, rec_uv=oe.recon_uv,
                                slice_rows=oracle.slice_rows_for(mbh, okw["p_slices"], okw["slice_deblock_local"]))
            oe.close(); dec.close()
        finally:
            oracle.set_features(oracle.F_ALL)
    return _ORACLE[key]


def _bookings(e, keys, depth, exclusive, aq, iip, fip):
    """What enc_schedule.cpp books per picture, from PRE on: (pmb_rows_total, db_started_total, ip_done_total, qpc_total).  A gated fused P stage with three
    pictures in flight counts mbw macroblocks into every row's word; every band-deblocking launch counts its workgroups (two per band, four where a P picture's
    bands are walked in two parts: mbw >= DB_CUT_MIN_MBW = 60); the intra rows riding in a deblocking launch count mbh rows; the QP_Y chain counts mbh rows."""
    nb = (e.mbh + 3) // 4
    out = []
    for k in keys[PRE:]:
        gated = (not k) and exclusive and depth >= 2 and not (aq and iip == 2)
        out.append((e.mbw if gated else 0, (2 if k or e.mbw < 60 else 4) * nb, e.mbh if gated and fip and not aq and iip else 0, e.mbh if aq else 0))
    return out


def _run(E, oracle, w, h, kind, slicing, depth, exclusive, preset, gop=GOP, iip=1, aq=False, imode=0, fip=True, force=(), trip_at=None):
    """The stream test described in the module's docstring.  preset: dict for debug_set_counters, or a function of the per-picture bookings that returns one.
    Returns (counters right behind the preset, counters at the end, bookings, oracle stream, encoder statistics)."""
    ref = _oracle_stream(oracle, w, h, kind, slicing, gop, iip, aq, tuple(force))
    clip = _clip(w, h, kind)
    e = E.Encoder(w, h, gop=gop, fixed_qp=QP, pipeline_depth=depth, exclusive=exclusive, intra_in_p=iip, aq=aq, intra_mode=imode, scenecut=False, **SLICINGS[slicing])
    try:
        assert e.p_slice_rows == ref["slice_rows"]
        book = _bookings(e, ref["keys"], depth, exclusive, aq, iip, fip)
        got = []

        def feed(lo, hi):
            for i in range(lo, hi):
                if i == trip_at:
                    e.debug_trip_wait(12)
                e.submit(*clip[i], pts=i)
                if e.pending > depth:
                    got.append(e.collect())
            while e.pending:
                got.append(e.collect())

        feed(0, PRE)
        e.debug_set_counters(**(preset(book) if callable(preset) else preset))
        c1 = e.debug_get_counters()
        feed(PRE, len(clip))
        c2 = e.debug_get_counters()
        st = e.stats()
        assert [g[2] for g in got] == list(range(len(clip)))
        assert [g[1] for g in got] == ref["keys"]
        for i, g in enumerate(got):
            assert g[0] == ref["aus"][i], ("access unit", i, len(g[0]), len(ref["aus"][i]))
        ry, ruv = e.fetch(E.FETCH_RECON_Y), e.fetch(E.FETCH_RECON_UV)
        assert np.array_equal(ry, ref["rec_y"]), first_diff(ry, ref["rec_y"])
        assert np.array_equal(ruv, ref["rec_uv"]), first_diff(ruv, ref["rec_uv"])
        if trip_at is None:
            assert st.recoveries == 0 and st.last_error_word == 0 and e.error_word() == 0, (st.recoveries, st.last_error_word, e.error_word())
        return c1, c2, book, ref, st
    finally:
        e.close()


NAMES = ("pmb_rows_total", "db_started_total", "ip_done_total", "qpc_total")


def _check_counts(c1, c2, book, in_use):
    """every count advanced by exactly what the schedule books; those the test is about must have been in use"""
    for j, name in enumerate(NAMES):
        want = sum(b[j] for b in book)
        assert (c2[name] - c1[name]) & M32 == want, "%s moved by %d, the schedule books %d" % (name, (c2[name] - c1[name]) & M32, want)
        if name in in_use:
            assert want > 0 and c2[name] != c1[name], "%s did not move: the schedule fell back to stream order (another encoder open? a safe level? a size threshold?)" % name


def _check_epoch(kind, c1, c2, n=N - PRE):
    assert c1["epoch"] == EPOCHS[kind] and c2["epoch"] == _next_epoch(EPOCHS[kind], n), (hex(c1["epoch"]), hex(c2["epoch"]))
    assert _crossed(kind, c1["epoch"], c2["epoch"]), (kind, hex(c1["epoch"]), hex(c2["epoch"]))
    # ... in the middle of the clip: the fifth picture behind the preset is stamped with the boundary value itself
    assert _next_epoch(EPOCHS[kind], CROSS + 1) in (0xFFFFF, 0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF)


def _check_intra_rows(ref, seam):
    """P pictures carry intra macroblocks before, on and behind the boundary and two pictures behind it -- with a seam, on both sides of it"""
    for i in (2, 3, 6, 7, 9):
        assert not ref["keys"][i]
        rows = ref["rows"][i]
        assert rows, i
        if seam:
            assert ref["slice_rows"] > 0 and any(r < ref["slice_rows"] for r in rows) and any(r >= ref["slice_rows"] for r in rows), (i, sorted(rows))


# ---------------------------------------------------------------- the epoch
@pytest.mark.parametrize("kind", list(EPOCHS))
@pytest.mark.parametrize("slicing", ["library", "mirror", "two"])
@pytest.mark.parametrize("fip", [True, False])
def test_epoch_three_in_flight(E, oracle, monkeypatch, kind, slicing, fip):
    """pipeline_depth 2, exclusive, 960 x 256 (bands walked in two parts; a first, inner and a last band; slicing "two": a seam with slice-local deblocking): the
    gated fused P stage on the band-done words of its reference (ref_epoch), the strips and cuts between bands, and the intra rows' 20-bit tag -- riding in the
    deblocking launch (fip), or as intra_p_kernel on its own stream with the deblocker gated on its progress words (MI355ENC_NO_FIP: the form of 1080p)."""
    if not fip:
        monkeypatch.setenv("MI355ENC_NO_FIP", "1")   # latched when the handle is opened
    c1, c2, book, ref, _ = _run(E, oracle, 960, 256, "cut", slicing, 2, True, dict(epoch=EPOCHS[kind]), fip=fip)
    _check_epoch(kind, c1, c2)
    _check_counts(c1, c2, book, ("pmb_rows_total", "db_started_total") + (("ip_done_total",) if fip else ()))
    _check_intra_rows(ref, slicing == "two")


@pytest.mark.parametrize("kind", list(EPOCHS))
@pytest.mark.parametrize("slicing", ["library", "mirror"])
@pytest.mark.parametrize("depth,exclusive,iip", [(2, True, 2), (0, False, 1), (1, True, 1)])
def test_epoch_other_schedules(E, oracle, kind, slicing, depth, exclusive, iip):
    """320 x 192 (bands walked whole): Intra_4x4 in P pictures with three pictures in flight; depth 0 without device-side waits between launches (epoch tags
    only); depth 1 exclusive (the fused stage gated, its deblocking launch behind it by event)."""
    c1, c2, book, ref, _ = _run(E, oracle, 320, 192, "cut", slicing, depth, exclusive, dict(epoch=EPOCHS[kind]), iip=iip)
    _check_epoch(kind, c1, c2)
    _check_counts(c1, c2, book, ("db_started_total",) + (("pmb_rows_total",) if depth == 2 else ()))
    _check_intra_rows(ref, False)


@pytest.mark.parametrize("kind", list(EPOCHS))
@pytest.mark.parametrize("slicing", ["library", "mirror"])
@pytest.mark.parametrize("imode,gop", [(0, GOP), (2, GOP), (0, 1)])
def test_epoch_idr_deblocker_beside_the_intra_wavefront(E, oracle, kind, slicing, imode, gop):
    """exclusive: an IDR picture's deblocker runs beside its intra wavefront, its bands waiting for the inverted epoch in d_iband_done (intra_mode 0: per row; 2: per
    band of the lock-step kernel); gop 1: an all-intra stream, in which the next picture's wavefront starts while this one is being deblocked (dbI_busy)."""
    c1, c2, book, _, _ = _run(E, oracle, 320, 192, "s2", slicing, 2, True, dict(epoch=EPOCHS[kind]), gop=gop, imode=imode)
    _check_epoch(kind, c1, c2)
    _check_counts(c1, c2, book, ("db_started_total",) + (("pmb_rows_total",) if gop > 1 else ()))


# ---------------------------------------------------------------- the four counts
def _at(boundary, j):
    """the count j starts so that the boundary falls into the middle of what the fifth picture behind the preset books (or the next one that books anything)"""
    def preset(book):
        k = CROSS
        while book[k][j] == 0:
            k += 1
        return {NAMES[j]: (boundary - sum(b[j] for b in book[:k]) - book[k][j] // 2) & M32}
    return preset


BOUNDS = {"sign": 1 << 31, "wrap": 1 << 32}


@pytest.mark.parametrize("kind", list(BOUNDS))
@pytest.mark.parametrize("slicing", ["library", "mirror"])
@pytest.mark.parametrize("name,aq", [("pmb_rows_total", False), ("db_started_total", False), ("ip_done_total", False), ("qpc_total", True)])
def test_count_through_its_boundary(E, oracle, kind, slicing, name, aq):
    """pipeline_depth 2, exclusive, 960 x 256, a cut in the clip: each count on its own through 2^31 (the sign of the kernels' wrap-safe difference) and 2^32.  The row
    counts and the started workgroups in the free-running schedule, the intra rows' count with them riding in the deblocking launch, the QP_Y chain's with adaptive
    quantisation (which keeps the intra rows out of the launch)."""
    j = NAMES.index(name)
    c1, c2, book, ref, _ = _run(E, oracle, 960, 256, "cut", slicing, 2, True, _at(BOUNDS[kind], j), aq=aq)
    _check_counts(c1, c2, book, (name, "pmb_rows_total", "db_started_total"))
    assert _crossed(kind, c1[name], c2[name]), (name, hex(c1[name]), hex(c2[name]))
    _check_intra_rows(ref, False)


@pytest.mark.parametrize("kind", list(BOUNDS))
@pytest.mark.parametrize("aq", [False, True])
def test_everything_at_its_boundary_in_one_picture(E, oracle, kind, aq):
    """All four counts and the epoch reach their boundaries in the same picture (the intra rows' count and the QP_Y chain's exclude each other in use: once
    without, once with adaptive quantisation -- the idle one is preset all the same and must stay where it was put)."""
    def preset(book):
        p = {"epoch": EPOCHS[kind]}
        for j in range(4):
            p.update(_at(BOUNDS[kind], j)(book) if any(b[j] for b in book) else {NAMES[j]: (BOUNDS[kind] - 1) & M32})
        return p
    c1, c2, book, _, _ = _run(E, oracle, 960, 256, "cut", "two", 2, True, preset, aq=aq)
    _check_epoch(kind, c1, c2)
    used = ("pmb_rows_total", "db_started_total", "qpc_total" if aq else "ip_done_total")
    _check_counts(c1, c2, book, used)
    for name in used:
        assert _crossed(kind, c1[name], c2[name]), (name, hex(c1[name]), hex(c2[name]))


# ---------------------------------------------------------------- after a recovery at a high epoch
def test_recovery_while_the_tags_wrap(E, oracle):
    """mi355enc_debug_trip_wait as tests/test_recovery_gpu.py uses it, right behind a preset of 0xFFFFF - 3: the three pictures in flight carry the last tags below
    the wrap, recover() clears the counts but neither the epoch nor the epoch-tagged buffers, and the re-encode stamps 0x100000 (tag 0) and on.  The stream
    continues from the forced IDR picture and is the oracle's told to force one there."""
    c1, c2, _, ref, st = _run(E, oracle, 320, 192, "cut", "mirror", 2, True, dict(epoch=0xFFFFF - 3), force=(PRE,), trip_at=PRE)
    assert st.recoveries == 1 and st.last_error_word == 12 and st.safe_level == 1
    assert [i for i, k in enumerate(ref["keys"]) if k] == [0, PRE, PRE + GOP, PRE + 2 * GOP]
    assert c1["epoch"] == 0xFFFFF - 3 and c2["epoch"] == 0xFFFFF - 3 + 3 + (N - PRE)   # three pictures stamped twice
    assert _crossed("tag20", c1["epoch"], c2["epoch"])
    assert all(c2[k] == 0 for k in ("pmb_rows_total", "ip_done_total"))                  # (stream order from the recovery on)


# ---------------------------------------------------------------- the stage entry points
@pytest.mark.parametrize("kind", list(EPOCHS))
@pytest.mark.parametrize("w,h", [(176, 144), (960, 256)])
@pytest.mark.parametrize("imode", [0, 2])
def test_stage_intra_at_a_high_epoch(E, oracle, kind, w, h, imode):
    """The parity suite's comparison of the intra kernels (rows: 0, lock-step bands: 2) with the inverted epoch of their granules passing each boundary: every call stamps one."""
    cy, cuv = frames(w, h, 1)[0][:2]
    o_y, o_uv, o_mbi, o_lev = oracle.intra_frame(cy, cuv, 28)
    e = E.Encoder(cy.shape[1], cy.shape[0], fixed_qp=28, intra_mode=imode)
    try:
        e.debug_set_counters(epoch=EPOCHS[kind])
        for _ in range(8):
            d_y, d_uv, d_mbi, d_lev = e.stage_intra(cy, cuv, 28)
            assert all(np.array_equal(d_mbi[f], o_mbi[f]) for f in ("mb_type", "i16_mode", "chroma_mode", "cost", "qp", "nzmask"))
            assert np.array_equal(d_lev, o_lev) and np.array_equal(d_y, o_y) and np.array_equal(d_uv, o_uv), hex(e.debug_get_counters()["epoch"])
        c = e.debug_get_counters()
        assert c["epoch"] == _next_epoch(EPOCHS[kind], 8) and _crossed(kind, EPOCHS[kind], c["epoch"]) and e.error_word() == 0
    finally:
        e.close()


@pytest.mark.parametrize("kind", list(EPOCHS))
@pytest.mark.parametrize("w,h", [(176, 144), (960, 256)])
def test_stage_deblock_at_a_high_epoch(E, oracle, kind, w, h):
    """... and of the band deblocker (mode 0) on the oracle's pre-filter pictures (an I and a P picture, four times over), the plain epoch of its strips passing each boundary."""
    oe = oracle.Encoder(w, h, gop=60, threads=8)
    pics = []
    for _, _, y, uv in frames(w, h, 2):
        oe.encode(y, uv, QP)
        pics.append((oe.prefilter_y, oe.prefilter_uv, oe.mbinfo, oe.recon_y, oe.recon_uv))
    oe.close()
    e = E.Encoder((w + 15) // 16 * 16, (h + 15) // 16 * 16, fixed_qp=QP, deblock_mode=0)
    try:
        e.debug_set_counters(epoch=EPOCHS[kind])
        c1 = e.debug_get_counters()
        for _ in range(4):
            for py, puv, mbi, ry, ruv in pics:
                d_y, d_uv = e.stage_deblock(py, puv, mbi)
                assert np.array_equal(d_y, ry), first_diff(d_y, ry)
                assert np.array_equal(d_uv, ruv), first_diff(d_uv, ruv)
        c = e.debug_get_counters()
        assert c["epoch"] == _next_epoch(EPOCHS[kind], 8) and _crossed(kind, EPOCHS[kind], c["epoch"]) and e.error_word() == 0
        assert (c["db_started_total"] - c1["db_started_total"]) & M32 == 8 * (4 if e.mbw >= 60 else 2) * ((e.mbh + 3) // 4)   # (the stage launches a picture of either type like a P picture: in two parts from 60 macroblocks per row)
    finally:
        e.close()


# ---------------------------------------------------------------- the adversarial libraries
CHILD = textwrap.dedent("""
    import hashlib, json, sys
    sys.path.insert(0, %r)
    from ceracoder_amd import enc as E, synth
    import numpy as np
    w, h, n, depth, exclusive, presets = 1920, 1080, 14, int(sys.argv[1]), bool(int(sys.argv[2])), json.loads(sys.argv[3])
    # the clip of tests/test_adversarial_gpu.py: a window sliding 8 lines per picture down and back over a taller S2 clip
    big = list(synth.s2_frames(w, h + 64, n))
    offs = [8 * (i if i < 8 else 14 - i) for i in range(n)]
    clip = [(np.ascontiguousarray(y[o:o + h]), np.ascontiguousarray(uv[o // 2:o // 2 + h // 2])) for (y, uv), o in zip(big, offs)]
    e = E.Encoder(w, h, gop=30, fixed_qp=30, pipeline_depth=depth, exclusive=exclusive, scenecut=False)
    m, out, seen = hashlib.sha256(), [], []
    for i, (y, uv) in enumerate(clip):
        if str(i) in presets:  # drain, then put the handle where a long run would have put it
            while e.pending:
                out.append(e.collect()[0])
            e.debug_set_counters(**presets[str(i)])
        e.submit(y, uv, pts=i)
        seen.append(e.debug_get_counters())
        if e.pending > depth:
            out.append(e.collect()[0])
    while e.pending:
        out.append(e.collect()[0])
    for au in out:
        m.update(au)
    st = e.stats()
    print(json.dumps({"digest": m.hexdigest(), "recoveries": int(st.recoveries), "error_word": e.error_word(), "seen": seen}))
    e.close()
""") % ROOT


def _child(tmp_path, lib, depth, exclusive, presets):
    script = tmp_path / "longrun_adv.py"
    script.write_text(CHILD)
    env = dict(os.environ)
    env.pop("MI355ENC_LIB", None)
    if lib:
        path = os.path.join(ROOT, "ceracoder_amd", "variants", "libmi355enc_%s.so" % lib)
        if not os.path.exists(path):
            pytest.fail("%s not built: run __graft_entry__.build()" % path)
        env["MI355ENC_LIB"] = path
    r = subprocess.run([sys.executable, str(script), str(depth), str(int(exclusive)), json.dumps(presets)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


_IN_ORDER = {}


def _in_order(tmp_path):
    if not _IN_ORDER:
        _IN_ORDER.update(_child(tmp_path, None, 0, False, {}))   # the shipped library, every kernel in stream order, nothing preset
    return _IN_ORDER


def test_delayed_progress_words_at_a_stale_tag_and_through_tag_zero(tmp_path):
    """ADVIP (every progress word of the intra rows ~20 us late: the deblocker catches up with them at every intra macroblock), three pictures in flight, one run:
    picture 1 (a P picture) leaves its words behind with tag 2; the preset makes picture 2 epoch 2 + 2^20 -- the same 20 bits, 2^20 - 1 epochs without a launch
    of the rows in between, what a run of IDR pictures of 4 h 51 min leaves -- so every word the deblocker finds says "row final" under its own picture's
    tag until that picture's rows have rewritten it: the words are cleared in front of such a launch (ip_rows_stamp).  A second preset takes the tag through
    0xFFFFF -> 0 at pictures 9 / 10.  The digest is the in-order run's."""
    presets = {"2": {"epoch": 2 + (1 << 20) - 1}, "6": {"epoch": 0x2FFFFF - 4}}
    adv = _child(tmp_path, "ADVIP", 2, True, presets)
    ep = [s["epoch"] for s in adv["seen"]]
    assert ep[1] == 2 and ep[2] == 2 + (1 << 20) and (ep[9] & 0xFFFFF, ep[10] & 0xFFFFF) == (0xFFFFF, 0), [hex(x) for x in ep]
    mbw = 120
    assert adv["seen"][-1]["pmb_rows_total"] == 13 * mbw, "the fused P stage did not run gated: the schedule fell back to stream order"
    assert adv["recoveries"] == 0 and adv["error_word"] == 0
    assert adv["digest"] == _in_order(tmp_path)["digest"]


def test_delayed_band_with_the_gate_epoch_through_the_wrap(tmp_path):
    """ADVBAND (one deblocking band's last lines reach memory ~0.3 ms late), three pictures in flight: the band-done words pmb_kernel's gate compares with its
    reference's epoch go 0xFFFFFFFE, 0xFFFFFFFF, 1, 2 at pictures 5 .. 8 of the clip."""
    adv = _child(tmp_path, "ADVBAND", 2, True, {"2": {"epoch": 0xFFFFFFFF - 5}})
    ep = [s["epoch"] for s in adv["seen"]]
    assert ep[5:9] == [0xFFFFFFFE, 0xFFFFFFFF, 1, 2], [hex(x) for x in ep]
    assert adv["seen"][-1]["pmb_rows_total"] == 13 * 120, "the fused P stage did not run gated: the schedule fell back to stream order"
    assert adv["recoveries"] == 0 and adv["error_word"] == 0
    assert adv["digest"] == _in_order(tmp_path)["digest"]


# ---------------------------------------------------------------- host-side wraps that need the device only as a source of pictures
@pytest.mark.parametrize("w,h", [(16, 16), (64, 48)])
@pytest.mark.parametrize("depth", [0, 2])
def test_frame_num_wraps_in_an_ordinary_stream(E, oracle, w, h, depth):
    """520 P pictures behind one IDR picture (gop 600, no intra refresh): frame_num, 8 bits in the slice header, is the picture's distance from the IDR picture
    modulo 256; the access units are the oracle's, and the independent decoder reproduces the reconstruction."""
    n = 521
    fr = [(y, uv) for _, _, y, uv in frames(w, h, 12)]
    pic = lambda i: fr[i % 22 if i % 22 < 12 else 22 - i % 22]
    e = E.Encoder(w, h, gop=600, fixed_qp=QP, pipeline_depth=depth, exclusive=depth == 2, scenecut=False)
    oe, dec = oracle.Encoder(w, h, gop=600, threads=4, scenecut=False), oracle.Decoder()
    try:
        got = []
        for i in range(n):
            e.submit(*pic(i), pts=i)
            if e.pending > depth:
                got.append(e.collect()[0])
        while e.pending:
            got.append(e.collect()[0])
        fns = []
        for i, au in enumerate(got):
            assert au == oe.encode(*pic(i), QP)[0], i
            dy, duv = dec.decode(au)
            hdr = slice_headers(au)
            assert hdr and len({s[2] for s in hdr}) == 1
            fns.append(hdr[0][2])
        assert fns == [i % 256 for i in range(n)]
        assert np.array_equal(dy, e.fetch(E.FETCH_RECON_Y)) and np.array_equal(duv, e.fetch(E.FETCH_RECON_UV))
        assert np.array_equal(dy, oe.recon_y) and e.stats().recoveries == 0
    finally:
        e.close(); oe.close(); dec.close()


def test_idr_pic_id_wraps_after_65536_idr_pictures(E, oracle):
    """idr_count preset to 65534 in an all-intra stream: idr_pic_id (ue(v) behind frame_num) runs 65534, 65535, 0, 1, ...; two consecutive IDR pictures never
    share a value (7.4.3), and every access unit decodes to the device's reconstruction."""
    w, h = 64, 48
    e = E.Encoder(w, h, gop=1, fixed_qp=QP, scenecut=False)
    dec = oracle.Decoder()
    try:
        e.debug_set_counters(idr_count=65534)
        ids = []
        for i, (_, _, y, uv) in enumerate(frames(w, h, 6)):
            au, key = e.encode(y, uv, pts=i)
            hdr = slice_headers(au)
            assert key and hdr and all(s[0] == 5 and s[2] == 0 for s in hdr) and len({s[3] for s in hdr}) == 1
            ids.append(hdr[0][3])
            dy, duv = dec.decode(au)
            assert np.array_equal(dy, e.fetch(E.FETCH_RECON_Y)) and np.array_equal(duv, e.fetch(E.FETCH_RECON_UV)), i
        assert ids == [65534, 65535, 0, 1, 2, 3]
        assert all(a != b for a, b in zip(ids, ids[1:]))
        assert e.debug_get_counters()["idr_count"] == 65540
    finally:
        e.close(); dec.close()


# ---------------------------------------------------------------- the hook's own rules
def test_set_counters_needs_an_idle_handle_and_keeps_what_it_is_not_given(E):
    """MI355ENC_ERR_STATE with a picture pending (the handle stays as it was); a field that is not named is not touched; host-side value and device-side word move
    together (the next pictures run without a wait running out)."""
    w, h = 320, 192
    fr = [(y, uv) for _, _, y, uv in frames(w, h, 4)]
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, exclusive=True, scenecut=False)
    try:
        e.submit(*fr[0], pts=0)
        before = e.debug_get_counters()
        with pytest.raises(E.EncoderError) as err:
            e.debug_set_counters(epoch=77)
        assert "(%d)" % E.ERR_STATE in str(err.value) and e.debug_get_counters() == before
        e.collect()
        e.debug_set_counters(db_started_total=M32 - 1)
        after = e.debug_get_counters()
        assert after == dict(before, db_started_total=M32 - 1)
        e.debug_set_counters()   # nothing named: nothing moves
        assert e.debug_get_counters() == after
        for i in (1, 2, 3):
            e.submit(*fr[i], pts=i)
        while e.pending:
            e.collect()
        assert e.stats().recoveries == 0 and e.error_word() == 0
        assert e.debug_get_counters()["db_started_total"] == (M32 - 1 + 3 * 2 * ((e.mbh + 3) // 4)) & M32
    finally:
        e.close()
