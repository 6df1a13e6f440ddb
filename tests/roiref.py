"""Region-of-interest quantisation, the references of its tests: the map's rule in numpy (roi_map), the sanitiser driver's sequence
of configurations and its checksum (driver_checksum: the same xorshift32 and FNV-1a as san_roi_driver.c), and the oracle composed under a map -- one IDR
picture and one P picture behind it through the oracle's stage functions with orc_set_aq_map, written, decoded and checked (compose_idr / compose_p), which
the CPU tests hold against the oracle's own decoder and the GPU tests against the device."""
import ctypes as C

import numpy as np

D, F, B = 12, 8, 12  # |delta|, feather, balance at most


def roi_map(cfg, user, mbw, mbh):
    """cfg: dict(rects=[(x, y, w, h, delta, feather), ...], balance=) or None; user: int8 (mbh, mbw) or None -> (t int8 (mbh, mbw), active, background)"""
    rects = [] if cfg is None else [tuple(r) + ((0,) if len(r) == 5 else ()) for r in cfg.get("rects", ())]
    balance = 0 if cfg is None else int(cfg.get("balance", 0))
    my, mx = np.mgrid[0:mbh, 0:mbw].astype(np.int64)
    e, p = np.zeros((mbh, mbw), np.int64), np.zeros((mbh, mbw), np.int64)
    for x, y, w, h, delta, feather in rects:
        if x >= 16 * mbw or y >= 16 * mbh or x + w <= 0 or y + h <= 0:
            continue  # wholly outside: nothing, feather included
        mx0, mx1, my0, my1 = x >> 4, (x + w - 1) >> 4, y >> 4, (y + h - 1) >> 4  # (Python's >> is a floor)
        d = np.maximum.reduce([mx0 - mx, mx - mx1, my0 - my, my - my1, np.zeros_like(mx)])
        ramp = abs(delta) * np.clip(feather + 1 - d, 0, None) // (feather + 1)
        c = np.where(d == 0, abs(delta), np.where(d <= feather, ramp, 0))
        if delta < 0:
            e = np.minimum(e, -c)
        else:
            p = np.maximum(p, c)
    t = np.where(e < 0, e, p)
    if user is not None:
        t = t + np.asarray(user, np.int64).reshape(mbh, mbw)
    t = np.clip(t, -D, D)
    active = bool((t != 0).any())
    S, N0, b = int(t.sum()), int((t == 0).sum()), 0
    if balance > 0 and S < 0 and N0 > 0:
        b = min(balance, (-S + N0 // 2) // N0)
        t = np.where(t == 0, b, t)
    return t.astype(np.int8), active, b


# ---- the sanitiser driver's sequence (ceracoder_amd/csrc/san_roi_driver.c), reproduced
class Rng:
    def __init__(self, s=0x9E3779B9):
        self.s = s

    def next(self):
        s = self.s
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        self.s = s
        return s

    def between(self, lo, hi):
        return lo + self.next() % (hi - lo + 1)


BASE = dict(rects=[(16, 16, 40, 20, -6, 2)], balance=6)
FIELDS = [("n_rects", 0, 8), ("x", -65536, 65536), ("y", -65536, 65536), ("w", 1, 65536), ("h", 1, 65536), ("delta", -12, 12), ("feather", 0, 8), ("balance", 0, 12)]
BEYOND = [(-40, 40, 60, 60), (-100, 40, 100, 60), (-100, 40, 99, 60), (300, 40, 100, 60), (336, 40, 100, 60), (335, 40, 1, 60),
          (40, -30, 60, 50), (40, -50, 60, 50), (40, 170, 60, 50), (40, 192, 60, 50), (-65536, -65536, 65536, 65536), (-65535, -65535, 65536, 65536)]
SIZES = [(1, 1), (4, 3), (5, 3), (21, 12), (45, 25)]
BIG = dict(rects=[(1000, 2000, 3000, 1500, -12, 8), (8000, 8100, 65536, 65536, 7, 3)], balance=12)


def with_field(name, v):
    """BASE with one field at v (n_rects 8: the seven further rectangles of the driver)"""
    x, y, w, h, delta, feather = BASE["rects"][0]
    r = dict(x=x, y=y, w=w, h=h, delta=delta, feather=feather)
    cfg = dict(rects=[tuple(r.values())], balance=BASE["balance"])
    if name == "n_rects":
        cfg["rects"] = [(x + 16 * j, y, w, h, delta if j == 0 else (5 if j & 1 else -5), feather) for j in range(max(v, 0))]
    elif name == "balance":
        cfg["balance"] = v
    else:
        r[name] = v
        cfg["rects"] = [tuple(r.values())]
    return cfg


def random_cfg(g, mbw, mbh):
    n, balance, rects = g.between(0, 8), g.between(0, 12), []
    for _ in range(n):
        x, y = g.between(-64, 16 * mbw + 32), g.between(-64, 16 * mbh + 32)
        w, h = g.between(1, 16 * mbw + 64), g.between(1, 16 * mbh + 64)
        delta = g.between(1, 12)
        if g.next() & 1:
            delta = -delta
        rects.append((x, y, w, h, delta, g.between(0, 8)))
    return dict(rects=rects, balance=balance)


def driver_cases():
    """(cfg, mbw, mbh, user) in the driver's order, the caller's maps drawn from its generator"""
    g = Rng()

    def case(cfg, mbw, mbh, with_user):
        user = np.array([g.between(-12, 12) for _ in range(mbw * mbh)], np.int8).reshape(mbh, mbw) if with_user else None
        return cfg, mbw, mbh, user

    for name, lo, hi in FIELDS:
        for v in (lo, hi):
            yield case(with_field(name, v), 5, 3, False)
            yield case(with_field(name, v), 21, 12, True)
    for i, (x, y, w, h) in enumerate(BEYOND):
        for fe in (0, 4, 8):
            yield case(dict(rects=[(x, y, w, h, 12 if i & 1 else -12, fe)], balance=6), 21, 12, False)
    yield case(BASE, 1, 1, False)
    yield case(BASE, 1, 1, True)
    yield case(None, 1, 1, True)
    yield case(BIG, 512, 512, False)
    yield case(BIG, 512, 512, True)
    yield case(None, 512, 512, False)
    for i in range(200):
        mbw, mbh = SIZES[i % 5]
        cfg = random_cfg(g, mbw, mbh)
        yield case(cfg, mbw, mbh, bool(g.next() & 1))


def driver_checksum(map_fn=roi_map):
    """FNV-1a over every map of driver_cases (bytes, then active and background) -> (checksum, maps)"""
    h, n = np.uint64(2166136261), 0
    for cfg, mbw, mbh, user in driver_cases():
        t, active, bg = map_fn(cfg, user, mbw, mbh)
        data = np.concatenate([np.asarray(t, np.int8).reshape(-1).view(np.uint8), np.array([int(active), bg], np.uint8)])
        hv = int(h)
        for b in data.tolist():  # (262 144 bytes at 512 x 512: a second of Python)
            hv = ((hv ^ b) * 16777619) & 0xFFFFFFFF
        h = np.uint64(hv)
        n += 1
    return int(h), n


# ---- the oracle composed under a map
_keep = None


def set_aq_map(oracle, t):
    """orc_set_aq_map: the offsets of the picture the oracle's stage functions code next (None: none); the array is kept alive until the next call"""
    global _keep
    L = oracle.lib()
    L.orc_set_aq_map.argtypes, L.orc_set_aq_map.restype = [C.c_void_p], None
    _keep = None if t is None else np.ascontiguousarray(t, np.int8).reshape(-1)
    L.orc_set_aq_map(None if t is None else _keep.ctypes.data_as(C.c_void_p))


def sends_delta(mbi):
    """7.3.5: mb_qp_delta is there for an Intra_16x16 macroblock and for one with a coded block"""
    return (mbi["mb_type"] == 0) | ((mbi["nzmask"] & 0x07FFFFFF) != 0)


def check_qp(mbi, qp_y, qp, t, mbw, slice_rows):
    """mbi: the picture's records (which macroblocks send a delta); qp_y: QP_Y of every macroblock as a decoder derived it; t: the offsets the picture was
    coded with.  QP_Y of every macroblock that sends a delta is clamp(qp + t), and every delta sent lies in -26 .. +25 (7.4.5).  Returns the deltas sent."""
    want = np.clip(qp + np.asarray(t, np.int64).reshape(-1), 0, 51)
    sent = sends_delta(mbi)
    qp_y = np.asarray(qp_y, np.int64).reshape(-1)
    assert np.array_equal(qp_y[sent], want[sent]), "QP_Y of a macroblock that sends mb_qp_delta is not clamp(qp + t)"
    prev = np.concatenate([[qp], qp_y[:-1]])
    if slice_rows:
        prev[::slice_rows * mbw] = qp  # QP_Y,PRED at a slice's first macroblock: the slice's QP
    assert np.array_equal(qp_y[~sent], prev[~sent]), "QP_Y of a macroblock without mb_qp_delta is not its predecessor's"
    deltas = (qp_y - prev)[sent]
    assert deltas.size == 0 or (-26 <= deltas.min() and deltas.max() <= 25), (int(deltas.min()), int(deltas.max()))
    return deltas


def _finish(oracle, dec, w, h, is_idr, frame_num, qp, t, rows, rec_y, rec_uv, mbi, lev, headers, idr_pic_id=0):
    """QP_Y chain, deblocking, slice writing (all under the map), then the oracle's decoder on the access unit and the checks of the module's docstring"""
    mbh, mbw = rec_y.shape[0] // 16, rec_y.shape[1] // 16
    mbi = np.ascontiguousarray(mbi)
    oracle.lib().orc_qp_chain_slices(mbi.ctypes.data_as(C.c_void_p), mbi.size, qp, rows * mbw)
    rec_y, rec_uv = oracle.deblock_frame(rec_y, rec_uv, mbi)
    au = (oracle.write_headers(w, h, 60) if headers else b"") + oracle.write_slice(mbw, mbh, is_idr, frame_num, idr_pic_id, qp, mbi, lev)
    cap_mbi, _ = dec.capture(mbw * mbh)
    dy, duv = dec.decode(au)
    assert np.array_equal(dy, rec_y) and np.array_equal(duv, rec_uv), "the access unit does not decode to the composed reconstruction"
    deltas = check_qp(mbi, cap_mbi["qp"], qp, t, mbw, rows)
    return dict(au=au, rec_y=rec_y, rec_uv=rec_uv, mbi=mbi, lev=lev, deltas=deltas)


def compose_idr(oracle, dec, w, h, yp, uvp, qp, t, rows=0, dbf=0, idr_pic_id=0):
    """One IDR picture of the padded planes yp / uvp under the map t (int8, one offset per macroblock) with slices of `rows` macroblock rows (0: one) and
    disable_deblocking_filter_idc dbf: orc_intra_frame (analysis, decisions, reconstruction) -> orc_qp_chain_slices -> orc_deblock_frame ->
    orc_write_slice behind orc_write_headers, decoded by dec"""
    oracle.set_slice_rows(rows)
    oracle.set_slice_deblock(dbf)
    set_aq_map(oracle, t)
    try:
        rec_y, rec_uv, mbi, lev = oracle.intra_frame(yp, uvp, qp)
        pre = (rec_y.copy(), rec_uv.copy(), mbi.copy())
        out = _finish(oracle, dec, w, h, True, 0, qp, t, rows, rec_y, rec_uv, mbi, lev, True, idr_pic_id)
        out["pre"] = pre
        return out
    finally:
        set_aq_map(oracle, None)
        oracle.set_slice_rows(0)
        oracle.set_slice_deblock(0)


def field(oracle, cy, ry, qp, iters=3):
    """the whole-sample search of the oracle's encoder: source against source, then the selection's iterations (tests/test_t8_adaptive_gpu.py::_field)"""
    surf, imv = oracle.me_frame(cy, ry, 16, qp, threads=8)
    for _ in range(iters):
        imv = oracle.me_select(surf, imv, cy.shape[1] // 16, cy.shape[0] // 16, 16, qp, threads=8)
    return surf, imv


def compose_p(oracle, dec, w, h, yp, uvp, prev_yp, ref_y, ref_uv, qp, t, rows=0, dbf=0, frame_num=1):
    """One P picture behind a picture dec has decoded: the search against the previous padded source, orc_pmb_frame and orc_intra_p_frame from the
    reference (ref_y, ref_uv) under the map t, then as compose_idr"""
    mbh, mbw = yp.shape[0] // 16, yp.shape[1] // 16
    oracle.set_slice_rows(rows)
    oracle.set_slice_deblock(dbf)
    try:
        surf, imv = field(oracle, yp, prev_yp, qp)
        idec = oracle.intra_decide(oracle.intra_analyse(yp, uvp), mbw, mbh, qp, False)
        set_aq_map(oracle, t)
        rec_y, rec_uv, mbi, lev, pre = oracle.pmb_frame(yp, uvp, ref_y, ref_uv, imv, surf, qp, idec=idec, threads=8)
        before = (rec_y.copy(), rec_uv.copy(), mbi.copy())  # (in front of the chain and the filter: what mi355enc_stage_pmb with run_intra_p gives)
        out = _finish(oracle, dec, w, h, False, frame_num, qp, t, rows, rec_y, rec_uv, mbi, lev, False)
        out.update(pre=before, imv=imv, surf=surf, idec=idec, pmb_pre=pre)
        return out
    finally:
        set_aq_map(oracle, None)
        oracle.set_slice_rows(0)
        oracle.set_slice_deblock(0)


# ---- the composed pictures the CPU and the GPU tests share: computed once per (size, slices, QP)
SIZES_COMPOSED, QPS_COMPOSED = ((176, 144), (322, 182)), (6, 30, 45)  # (QP 6 and 45 with -12 and +12: both clamps of QP_Y are reached)
_COMPOSED = {}


def picture_map(w, h, seed=7):
    """the map the composed pictures are coded under: -12 in the centre with a feather, +12 in a corner, the caller's noise of -2 .. +2 and a balance"""
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    cfg = dict(rects=[(w // 2, h // 2, w // 4, h // 4, -12, 1), (0, 0, 32, 32, 12, 0)], balance=6)
    user = np.random.default_rng(seed).integers(-2, 3, (mbh, mbw)).astype(np.int8)
    return cfg, user, roi_map(cfg, user, mbw, mbh)[0]


def composed(w, h, slices, qp):
    """IDR + P of the S2 clip at w x h under picture_map, slices 1 (the filter across nothing) or 2 (slice-local deblocking): dict(clip=, t=, rows=, dbf=, idr=, p=)"""
    key = (w, h, slices, qp)
    if key not in _COMPOSED:
        from oracle import oracle as O
        from tests.util import frames
        O.lib()
        clip = frames(w, h, 2)
        t = picture_map(w, h)[2]
        rows = O.slice_rows_for((h + 15) // 16, slices, slices > 1) if slices > 1 else 0
        dbf = 2 if slices > 1 else 0
        dec = O.Decoder()
        (y0, uv0), (y1, uv1) = clip[0][:2], clip[1][:2]
        idr = compose_idr(O, dec, w, h, y0, uv0, qp, t, rows, dbf)
        p = compose_p(O, dec, w, h, y1, uv1, y0, idr["rec_y"], idr["rec_uv"], qp, t, rows, dbf)
        dec.close()
        _COMPOSED[key] = dict(clip=clip, t=t, rows=rows, dbf=dbf, idr=idr, p=p)
    return _COMPOSED[key]


def aq_offsets(oracle, yp):
    """orc_aq_offsets of a padded luma plane -> int8 (mbh, mbw)"""
    yp = np.ascontiguousarray(yp, np.uint8)
    mbh, mbw = yp.shape[0] // 16, yp.shape[1] // 16
    out = np.zeros((mbh, mbw), np.int8)
    oracle.lib().orc_aq_offsets(yp.ctypes.data_as(C.c_void_p), yp.shape[1], mbw, mbh, out.ctypes.data_as(C.c_void_p))
    return out


def offsets(oracle, yp, t, aq):
    """rule 6: what the device quantises a picture with -- clamp(aq + t, -12, 12), aq = 0 without adaptive quantisation"""
    a = aq_offsets(oracle, yp).astype(np.int64) if aq else 0
    return np.clip(a + np.asarray(t, np.int64).reshape(yp.shape[0] // 16, yp.shape[1] // 16), -D, D).astype(np.int8)
