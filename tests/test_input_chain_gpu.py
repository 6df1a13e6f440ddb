"""GPU: the whole input chain at once, on pictures with coded margins ("The chain").  Handles with one step and with every step of
ingest_end on are held to tests/chainref.py, the composition of the steps' own references: the slot's source surfaces at every collect with ==, the access
units against a plain encoder fed the composition's visible pictures, and every record a last_* call reports.  The pictures are the smallest at which the
named thing can go wrong (chainref.PICTURES); tests/test_input_chain_cpu.py checks that every step does something on every picture of them."""
import ctypes as C_

import numpy as np
import pytest

from oracle import csc as OC
from tests import adjustref as A
from tests import chainref as C
from tests import geomref as G
from tests import jpegref as J
from tests import qualityref as Q
from tests import rateref
from tests import snapref
from tests.inputref import device_planes
from tests.test_geometry_gpu import plain_stream, same
from tests.test_stabilize_gpu import planes_in

pytestmark = pytest.mark.gpu

GOP, QP, NPIC, DEPTH, NS = 30, 28, 6, 2, 10 ** 9
OFF = dict()  # a picture's settings with every step off


def encoder(E, name, rate=None, fps=60, stabilise=None, yuv=True, **kw):
    p = C.PICTURES[name]
    if p["geom"]:
        crop, dst, _ = p["geom"]
        kw["geometry"] = E.geometry(C.IN, crop=crop, dst=dst, border=C.BORDER, keep_sar=True)  # (the headers of an unscaled stream: the plain encoder's)
        if crop and (stabilise is None or stabilise):
            kw["stabilize"] = dict(range=C.STAB[0], leak=C.STAB[1], margin=(C.STAB[2], C.STAB[3]))
    if p["method"]:
        kw["orientation"] = p["method"]
    if yuv:
        kw["input_colorimetry"] = C.INPUT_COLORIMETRY
    return E.Encoder(p["size"][0], p["size"][1], fps=fps, gop=GOP, fixed_qp=QP, pipeline_depth=DEPTH, colorimetry=C.COLORIMETRY, rate=rate, **kw)


class Setter:
    """hands a picture's settings to the handle, only what changed against the picture before (a set counts: generations), and keeps what each submit latched"""

    def __init__(self, E, e):
        self.E, self.e, self.cur, self.lut_gen, self.warp_gen, self.latched = E, e, {}, 0, 0, []

    def __call__(self, s):
        e, cur = self.e, self.cur
        for k in C.ORDER:
            new = s.get(k)
            if k == "yuv" or new is cur.get(k):
                continue
            if k == "warp":
                if new is None:
                    e.set_warp(None)
                else:
                    e.set_warp(dict(kind=new["kind"], fill=new["fill"]), **new["params"])
                    self.warp_gen += 1
            elif k == "dspatial":
                e.set_denoise_spatial(new)
            elif k == "denoise":
                e.set_denoise_motion(new[2] if new else 0)
                e.set_denoise(luma=new[0], chroma=new[1]) if new else e.set_denoise()
            elif k == "lut":
                if new is None:
                    e.set_lut3d(None)
                else:
                    e.set_lut3d(new[0], new[2])
                    self.lut_gen += 1
            elif k == "autolevel":
                e.set_autolevel(new)
            elif k == "adjust":
                e.set_adjust(new)
            elif k == "layers":
                if new:
                    ly = new[0]
                    e.set_image(0, ly["pixels"], ly["x"], ly["y"], ly["opacity"], self.E.FMT_RGBX)
                else:
                    e.set_image(0, None)
            elif k == "text":
                if new:
                    e.set_overlay_style(**new[1])
                e.set_overlay_text(new[0] if new else None)
            cur[k] = new
        self.latched.append(dict(lut=self.lut_gen if s.get("lut") else 0, warp=self.warp_gen if s.get("warp") else 0))


def drive(E, e, sets, feed, pts=None, mode=rateref.OFF, records=True):
    """every submit with its settings set in front of it, the pipeline kept full -> (per collected picture a dict: au, y, uv and the last_* records; what each
    submit returned; the Setter; the reconstruction of the last picture)"""
    setter, out, counts = Setter(E, e), [], []

    def take():
        d = dict(au=e.collect(), y=e.fetch(E.FETCH_SOURCE_Y), uv=e.fetch(E.FETCH_SOURCE_UV))
        if records:
            d.update(lut=e.last_lut3d(), warp=e.last_warp(), autolevel=e.last_autolevel(), dspatial=e.last_denoise_spatial(), stab=e.last_stabilize()[1],
                     adjust=e.last_adjust(), denoise=(e.last_denoise(), e.last_denoise_motion()), text=e.last_overlay())
        out.append(d)

    for i, s in enumerate(sets):
        setter(s)
        need = 1 if mode == rateref.OFF else max(e.rate_peek(pts[i]), 1 if mode == rateref.BLEND else 0)
        while DEPTH + 1 - e.pending < need:
            take()
        counts.append(feed(i))
    while e.pending:
        take()
    return out, counts, setter, (e.fetch(0), e.fetch(1))


def check_surfaces(got, want, w, h, replicas=True):
    assert len(got) == len(want)
    for i, (g, r) in enumerate(zip(got, want)):
        assert np.array_equal(g["y"], r["y"]), (i, np.argwhere(g["y"] != r["y"])[:4])
        assert np.array_equal(g["uv"], r["uv"]), (i, np.argwhere(g["uv"] != r["uv"])[:4])
        if replicas:
            assert C.margins_are_replicas(g["y"], g["uv"], w, h), i


def check_records(got, want, sets, setter, stab=None):
    """every picture carries the settings of its own submit, and reports what the composition computed for it"""
    for i, (g, r) in enumerate(zip(got, want)):
        s, lat = sets[r["input"]], setter.latched[r["input"]]
        lut = s.get("lut")
        assert g["lut"] == ((dict(size=lut[1], strength=lut[2]), lat["lut"]) if lut else (dict(size=0, strength=0), 0)), i
        assert g["warp"] == lat["warp"], i
        rec, table = r["records"]["autolevel"]
        assert g["autolevel"][1] == rec and np.array_equal(g["autolevel"][2], table), (i, g["autolevel"][1], rec)
        assert g["dspatial"][1] == r["records"]["dspatial"], (i, g["dspatial"][1], r["records"]["dspatial"])
        assert g["adjust"] == (A.params(**s["adjust"]) if s.get("adjust") else A.NEUTRAL), i
        dn = s.get("denoise") or (0, 0, 0)
        assert g["denoise"] == (dict(luma=dn[0], chroma=dn[1]), dn[2]), i
        assert g["text"] == (s["text"][0].encode() if s.get("text") else b""), i
        if stab is not None:
            assert g["stab"] == stab[r["input"]], (i, g["stab"], stab[r["input"]])


def plain(E, name, want, **kw):
    w, h = C.PICTURES[name]["size"]
    return plain_stream(E, w, h, [o["visible"] for o in want], colorimetry=C.COLORIMETRY, **kw)


def plain_groups(E, name, want, counts, fps=30):
    """the plain encoder at the output rate, fed the composition's outputs in the groups the converting encoder's submits yielded, with the ticks' pts"""
    w, h = C.PICTURES[name]["size"]
    p = E.Encoder(w, h, fps=fps, gop=GOP, fixed_qp=QP, pipeline_depth=DEPTH, colorimetry=C.COLORIMETRY)
    ref, k = [], 0
    for c in counts:
        while DEPTH + 1 - p.pending < c:
            ref.append(p.collect())
        for o in want[k:k + c]:
            p.submit(*o["visible"], pts=o["pts"])
        k += c
    while p.pending:
        ref.append(p.collect())
    out = ref, (p.fetch(0), p.fetch(1))
    p.close()
    return out


def stream_of(got, recon):
    return [g["au"] for g in got], recon


# ---- 1. one step on: the margins stay replicas
ONE = {
    "warp": lambda on: dict(warp=on["warp"]), "colour-step": lambda on: dict(), "spatial-filter": lambda on: dict(dspatial=on["dspatial"]),
    "temporal-filter": lambda on: dict(denoise=on["denoise"]), "motion-compensated-filter": lambda on: dict(denoise=(8, 8, 4)), "lut": lambda on: dict(lut=on["lut"]),
    "autolevel": lambda on: dict(autolevel=on["autolevel"]), "controls-table": lambda on: dict(adjust=dict(brightness=40, contrast=1200, saturation=1250)),
    "controls-sharpen": lambda on: dict(adjust=on["adjust"]), "layer": lambda on: dict(layers=on["layers"]), "text": lambda on: dict(text=on["text"]),
}


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("step", list(ONE))
def test_one_step_on_the_margins_stay_replicas_and_the_stream_is_the_plain_encoders(E, step, name):
    """(the motion-compensated filter on the still clip only: DESIGN.md section 25)"""
    n, yuv = 3, step == "colour-step"
    w, h = C.PICTURES[name]["size"]
    src = C.sources(name, n)
    sets = [ONE[step](C.all_on(name))] * n
    want = C.compose(C.handle(name, yuv=yuv), src, sets)
    assert all(not np.array_equal(o["visible"][0], s[0]) or not np.array_equal(o["visible"][1], s[1]) for o, s in list(zip(want, src))[1:])
    e = encoder(E, name, yuv=yuv)
    got, _, setter, recon = drive(E, e, sets, lambda i: e.submit(*src[i], pts=i))
    e.close()
    check_surfaces(got, want, w, h)
    check_records(got, want, sets, setter)
    same(stream_of(got, recon), plain(E, name, want))


@pytest.mark.parametrize("name", ["A", "B"])
def test_the_mix_alone_keeps_the_margins_replicas_and_the_stream_is_the_plain_encoders(E, name):
    """test 1's case of the mix: it has no setting of its own but the handle's rate conversion, five inputs at 50 a second give three pictures at 30"""
    w, h = C.PICTURES[name]["size"]
    src, pts = C.sources(name, 5), [i * NS // 50 for i in range(5)]
    want = C.compose(C.handle(name, yuv=False, rate=(rateref.BLEND, NS, 30, 2)), src, [OFF] * 5, pts=pts)
    assert any(not any(np.array_equal(o["visible"][0], s[0]) for s in src) for o in want)  # (a picture that is a mix)
    e = encoder(E, name, rate=(rateref.BLEND, NS, 2), fps=30, yuv=False)
    got, counts, _, recon = drive(E, e, [OFF] * 5, lambda i: e.submit(*src[i], pts=pts[i]), pts, rateref.BLEND, records=False)
    e.close()
    check_surfaces(got, want, w, h)
    assert sum(counts) == len(want) == 3 and [g["au"][2] for g in got] == [o["pts"] for o in want]
    same(stream_of(got, recon), plain_groups(E, name, want, counts))


# ---- 2. every step at once
def _submit(E, e, name, src, pts=None):
    return lambda i: e.submit(*src[i], pts=pts[i] if pts else i), src, None


def _submit_yuy2(E, e, name, src):
    w, h = C.PICTURES[name]["size"]
    planes = [planes_in(G.FMT_YUY2, s) for s in src]
    vis = [C.visible_part(*OC.to_nv12(OC.FMT_YUY2, p, w, h), w, h) for p in planes]
    return lambda i: e.submit_fmt(E.FMT_YUY2, planes[i], pts=i), vis, None


def _submit_jpeg(E, e, name, src):
    w, h = C.PICTURES[name]["size"]
    data = [J.write_jpeg([s[0], np.ascontiguousarray(s[1][:, 0::2]), np.ascontiguousarray(s[1][:, 1::2])], "420")[0] for s in src]
    vis = [C.visible_part(*J.surfaces(*J.decode(d), w, h), w, h) for d in data]
    return lambda i: e.submit_jpeg(data[i], pts=i), vis, None


def _submit_device(E, e, name, src, stride=None, offset=1, pts=None):
    """planes at an odd address and a stride of width + 5, unless the test names others (pts: the submits' time stamps; their indices otherwise)"""
    w, h = C.PICTURES[name]["size"]
    stride = stride or w + 5
    dev = [device_planes(E, [y, uv], [h, h // 2], [w, w], stride, offset) for y, uv in src]

    def after():
        for (hip, buf, ptrs), (y, uv) in zip(dev, src):  # the caller's planes are unchanged
            for ptr, p in zip(ptrs, (y, uv)):
                back = np.empty(p.shape, np.uint8)
                assert hip.hipMemcpy2D(back.ctypes.data_as(C_.c_void_p), C_.c_size_t(w), C_.c_void_p(ptr), C_.c_size_t(stride), C_.c_size_t(w), C_.c_size_t(p.shape[0]), 2) == 0
                assert np.array_equal(back, p)
            assert hip.hipFree(buf) == 0
    return lambda i: e.submit_device(dev[i][2][0], stride, dev[i][2][1], stride, pts=pts[i] if pts else i), src, after


ENTRY = {"submit": _submit, "submit_fmt-yuy2": _submit_yuy2, "submit_device": _submit_device, "submit_jpeg": _submit_jpeg}
_WANT = {}


def all_steps(name, n=NPIC, auto=False):
    """the composition of picture `name` with every step on, made once: (sources, settings, the composition, the stabiliser's records)"""
    if (name, n, auto) not in _WANT:
        src = C.sources(name, n)
        ins, stab = C.inputs(name, src)
        sets = [C.all_on(name, auto=auto)] * n
        _WANT[name, n, auto] = (src, sets, C.compose(C.handle(name), ins, sets), stab)
    return _WANT[name, n, auto]


@pytest.mark.parametrize("name,entry", [("A", k) for k in ENTRY] + [(k, "submit") for k in "BCD"] + [("D", "submit-spatial-filter-automatic")])
def test_every_step_at_once(E, name, entry):
    """(D once more with the spatial filter's automatic strength: its measure launch under the transposed rectangle, the record compared)"""
    w, h = C.PICTURES[name]["size"]
    src, sets, want, stab = all_steps(name, auto=entry.endswith("automatic"))
    e = encoder(E, name)
    feed, vis, after = ENTRY[entry.split("-spatial")[0]](E, e, name, src)
    if vis is not src:  # (another fill: the composition of the pictures that fill makes)
        want = C.compose(C.handle(name), vis, sets)
    got, _, setter, recon = drive(E, e, sets, feed)
    e.close()
    if after:
        after()
    check_surfaces(got, want, w, h)
    check_records(got, want, sets, setter, stab)
    same(stream_of(got, recon), plain(E, name, want))


# ---- 3. the same with the motion-compensated filter
def test_every_step_at_once_with_the_motion_compensated_filter(E):
    """surfaces and records only: a moving scene's margins behind the filter are no replicas by rule, and though the LUT writes them afresh nothing is claimed
    of the stream"""
    w, h = C.PICTURES["A"]["size"]
    src = C.sources("A", 4, still=False)
    sets = [dict(C.all_on("A"), denoise=(8, 8, 8))] * 4
    want = C.compose(C.handle("A"), src, sets)
    e = encoder(E, "A")
    got, _, setter, _ = drive(E, e, sets, lambda i: e.submit(*src[i], pts=i))
    e.close()
    check_surfaces(got, want, w, h, replicas=False)
    check_records(got, want, sets, setter)


# ---- 4. settings changed while three pictures are in flight
def test_settings_changed_with_three_pictures_in_flight_each_picture_carries_its_own(E):
    """eight pictures and chainref.changing's settings: warp at picture 1, spatial filter 2, temporal filter off 3, LUT 4, automatic levels 5, temporal filter
    on again with other strengths (it primes again) and the layer 6, controls and text 7 -- eight steps and one that comes back are nine changes for seven
    pictures, so two pictures carry two, each a once-per-input step beside a drawn one"""
    w, h, n = 70, 50, 8
    sets = C.changing("A", n)
    src = C.sources("A", n)
    want = C.compose(C.handle("A"), src, sets)
    e = encoder(E, "A")
    got, _, setter, recon = drive(E, e, sets, lambda i: e.submit(*src[i], pts=i))
    e.close()
    assert [lat["lut"] for lat in setter.latched] == [1, 1, 1, 1, 2, 2, 2, 2] and [lat["warp"] for lat in setter.latched] == [1] + [2] * 7
    check_surfaces(got, want, w, h)
    check_records(got, want, sets, setter)
    same(stream_of(got, recon), plain(E, "A", want))


# ---- 5. under the frame-rate mix
def test_under_the_mix_every_step_runs_once_per_input_and_layers_and_text_per_output(E):
    w, h, n = 70, 50, 10
    src, sets, _, _ = all_steps("A", n)
    pts = [i * NS // 50 for i in range(n)]
    want = C.compose(C.handle("A", rate=(rateref.BLEND, NS, 30, 2)), src, sets, pts=pts)
    steps = rateref.run(rateref.BLEND, NS, 30, 1, 2, pts)
    e = encoder(E, "A", rate=(rateref.BLEND, NS, 2), fps=30)
    got, counts, _, recon = drive(E, e, sets, lambda i: e.submit(*src[i], pts=pts[i]), pts, rateref.BLEND, records=False)
    e.close()
    assert counts == [len(s[0]) for s in steps] and 0 in counts and sum(counts) == len(want) == len(got)
    check_surfaces(got, want, w, h)
    assert [g["au"][2] for g in got] == [o["pts"] for o in want]
    same(stream_of(got, recon), plain_groups(E, "A", want, counts))


def test_a_held_picture_is_the_finished_picture_again(E):
    """hold, max_fill 2, inputs at 20 a second for 30: a repeated picture is not filtered, graded or measured twice; layers and text are drawn into it afresh"""
    w, h, n = 70, 50, 4
    src, sets, _, _ = all_steps("A", n)
    pts = [i * NS // 20 for i in range(n)]
    want = C.compose(C.handle("A", rate=(rateref.HOLD, NS, 30, 2)), src, sets, pts=pts)
    e = encoder(E, "A", rate=(rateref.HOLD, NS, 2), fps=30)
    got, counts, _, _ = drive(E, e, sets, lambda i: e.submit(*src[i], pts=pts[i]), pts, rateref.HOLD, records=False)
    e.close()
    assert max(counts) == 2 and sum(counts) == len(want) == len(got)
    check_surfaces(got, want, w, h)


# ---- 6. the readers see the finished picture
def test_the_quality_metrics_and_the_still_read_the_finished_picture(E):
    w, h = C.PICTURES["A"]["size"]
    src, sets, want, _ = all_steps("A")
    # the reconstructions: the plain encoder's, picture by picture
    p = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=0, colorimetry=C.COLORIMETRY)
    recs, ref = [], []
    for i, o in enumerate(want):
        p.submit(*o["visible"], pts=i)
        ref.append(p.collect())
        recs.append((p.fetch(E.FETCH_RECON_Y), p.fetch(E.FETCH_RECON_UV)))
    p.close()
    e = encoder(E, "A")
    e.set_quality_metrics(True)
    setter, aus, quality, stills = Setter(E, e), [], [], {}

    def take():
        aus.append(e.collect())
        quality.append(e.last_quality().ints())
        if len(aus) - 1 == 2:
            stills[2] = e.take_snapshot()
    for i in range(NPIC):
        setter(sets[i])
        if i == 2:
            e.request_snapshot(E.SNAP_SOURCE, 1, 75)
        e.submit(*src[i], pts=i)
        if e.pending > DEPTH:
            take()
    while e.pending:
        take()
    e.close()
    assert [a[:2] for a in aus] == [r[:2] for r in ref]  # the access units are those of the chain without either reader
    for i, o in enumerate(want):
        assert quality[i] == Q.quality(o["y"], o["uv"], recs[i][0], recs[i][1], w, h), i
    assert stills[2] is not None and stills[2][0] == snapref.still(*want[2]["visible"], 1, 75)


# ---- 7. everything off after everything on
def test_everything_off_after_everything_on_and_on_again(E):
    """from picture 3 on the bytes are the plain encoder's; on again at picture 5 every stateful step primes as its own reference says"""
    w, h, n = 70, 50, 7
    on = C.all_on("A")
    sets = [on] * 3 + [OFF] * 2 + [on] * 2
    src = C.sources("A", n)
    want = C.compose(C.handle("A", yuv=False), src, sets)
    for i in (3, 4):
        assert np.array_equal(want[i]["visible"][0], src[i][0]) and np.array_equal(want[i]["visible"][1], src[i][1])
    e = encoder(E, "A", yuv=False)
    got, _, setter, recon = drive(E, e, sets, lambda i: e.submit(*src[i], pts=i))
    e.close()
    check_surfaces(got, want, w, h)
    check_records(got, want, sets, setter)
    same(stream_of(got, recon), plain(E, "A", want))
