"""Plain numpy reference of the band deblocker's cut (k_deblock.hip, "the cut"; DESIGN sections 4-5) -- test infrastructure.

Written from H.264 8.7.2.1 (boundary strength) and the rule as DESIGN and the kernel's comments state it, not from the kernel's code:

  * A P picture's deblocking bands (DB_ROWS macroblock rows; the last one may be shorter) are walked by two workgroups each, split at
    a vertical macroblock edge whose bS is 0 in every row and segment of the band: the two parts then share no filtered sample.
  * The column is chosen inside a window of 2 * cut_w + 1 columns around the middle (cut_w = min(mbw / 4, 31)), nearest to a target
    a little left of the middle, right before left at equal distance.
  * It never lies left of the band above's cut when the band has a top edge in its slice and the band above had work and a cut inside
    the row; otherwise there is nothing to keep to.
  * A band without any edge to filter leaves 0; a band without a free column in the window leaves mbw (the left part walks it whole).

Records are enc.MBINFO_DTYPE arrays (raster order).  Partitions (bs_of_q) are out of scope: one vector per macroblock.
"""
import numpy as np

DB_ROWS = 4            # MI355_BAND_ROWS: macroblock rows per band
DB_CUT_MIN_MBW = 60    # k_deblock.hip: rows at least this long are walked in two parts
NZ_T8 = 1 << 27        # transform_size_8x8_flag of a P macroblock


def n_bands(mbh):
    return (mbh + DB_ROWS - 1) // DB_ROWS


def has_top(my, slice_rows, idc):
    """8.7: the top macroblock edge of row `my` is filtered -- not the picture's first row, and with disable_deblocking_filter_idc 2
    not a slice's first row."""
    return my > 0 and not (idc == 2 and slice_rows > 0 and my % slice_rows == 0)


def _grid(records, mbw, mbh):
    r = np.asarray(records).reshape(mbh, mbw)
    return r["mb_type"] != 1, r["nzmask"].astype(np.int64), r["mvx"].astype(np.int64), r["mvy"].astype(np.int64)


def _coded(nz, bx, by):
    """6.4.3: the luma 4x4 block at raster position (bx, by) carries coefficients; with the 8x8 transform the 8x8 block containing it
    (8.7.2.1: "the 8x8 luma block containing the sample ... contains non-zero transform coefficient levels")."""
    b8 = (by >> 1) * 2 + (bx >> 1)
    blk = 4 * b8 + (by & 1) * 2 + (bx & 1)
    t8 = (nz & NZ_T8) != 0
    return np.where(t8, ((nz >> (4 * b8)) & 15) != 0, ((nz >> blk) & 1) != 0)


def _bs(p, q, pb, qb, mb_edge):
    """8.7.2.1 for frame macroblocks with one reference picture, elementwise: p, q = (intra, nzmask, mvx, mvy) arrays,
    pb, qb = the (bx, by) of the 4x4 block on either side."""
    pi, pn, px, py = p
    qi, qn, qx, qy = q
    intra = pi | qi
    coded = _coded(pn, *pb) | _coded(qn, *qb)
    mv = (np.abs(px - qx) >= 4) | (np.abs(py - qy) >= 4)
    return np.where(intra, 4 if mb_edge else 3, np.where(coded, 2, np.where(mv, 1, 0)))


def vertical_mb_edge_bs(records, mbw, mbh):
    """bS of every macroblock's LEFT edge: (mbh, mbw, 4) by row, column and 4-sample segment; column 0 (the picture's edge) has none."""
    g = _grid(records, mbw, mbh)
    out = np.zeros((mbh, mbw, 4), np.int64)
    if mbw > 1:
        p = tuple(a[:, :-1] for a in g)
        q = tuple(a[:, 1:] for a in g)
        for sg in range(4):
            out[:, 1:, sg] = _bs(p, q, (3, sg), (0, sg), True)
    return out


def top_mb_edge_bs(records, mbw, mbh, slice_rows=0, idc=0):
    """bS of every macroblock's TOP edge where it is filtered (0 where not): (mbh, mbw, 4) by row, column and segment."""
    g = _grid(records, mbw, mbh)
    out = np.zeros((mbh, mbw, 4), np.int64)
    for my in range(1, mbh):
        if not has_top(my, slice_rows, idc):
            continue
        p = tuple(a[my - 1] for a in g)
        q = tuple(a[my] for a in g)
        for sg in range(4):
            out[my, :, sg] = _bs(p, q, (sg, 3), (sg, 0), True)
    return out


def inner_edge_work(records, mbw, mbh):
    """(mbh, mbw): some inner luma edge of the macroblock (vertical or horizontal edge 1..3; 1 and 3 are no transform edges with the
    8x8 transform) has bS > 0.  One vector per macroblock: an inner edge is never 1."""
    g = _grid(records, mbw, mbh)
    t8 = (g[1] & NZ_T8) != 0
    work = np.zeros((mbh, mbw), bool)
    for e in (1, 2, 3):
        skip = t8 if e & 1 else np.zeros_like(t8)
        for k in range(4):
            v = _bs(g, g, (e - 1, k), (e, k), False)
            h = _bs(g, g, (k, e - 1), (k, e), False)
            work |= ~skip & ((v > 0) | (h > 0))
    return work


def band_rows(band, mbh):
    return range(band * DB_ROWS, min(mbh, (band + 1) * DB_ROWS))


def band_work(records, mbw, mbh, slice_rows=0, idc=0):
    """(n_bands,) bool: some edge of the band -- vertical or horizontal, macroblock or inner, the top macroblock edge only where it is
    filtered -- has bS > 0.  (One flag for both planes: a chroma edge takes the bS of its luma edge, so a band with luma work only on
    luma edges 1 and 3 is walked in chroma too and filters nothing there.)"""
    row = (vertical_mb_edge_bs(records, mbw, mbh) > 0).any(axis=(1, 2))
    row |= (top_mb_edge_bs(records, mbw, mbh, slice_rows, idc) > 0).any(axis=(1, 2))
    row |= inner_edge_work(records, mbw, mbh).any(axis=1)
    return np.array([row[list(band_rows(b, mbh))].any() for b in range(n_bands(mbh))])


def window(mbw):
    """(first, last, target) columns of the cut's window: 2 * cut_w + 1 columns centred on mbw / 2, the target a little left of the middle."""
    mid, w = mbw // 2, min(mbw // 4, 31)
    return mid - w, mid + w, mid - w // 8


def _band_edge_bs(records, mbw, mbh, band):
    """vertical_mb_edge_bs of the band's rows alone (a vertical edge's bS takes nothing from another row): what a picture of 128 bands can afford per band"""
    rows = band_rows(band, mbh)
    return vertical_mb_edge_bs(np.asarray(records).reshape(mbh, mbw)[rows.start:rows.stop], mbw, len(rows))


def busy_columns(records, mbw, mbh, band):
    """Per plane, (2, mbw) bool: the left macroblock edge of the column has bS > 0 in some row of the band -- luma by its 16 lines' segments,
    chroma by its 8 lines (chroma line k lies in luma segment k // 2)."""
    bs = _band_edge_bs(records, mbw, mbh, band)
    luma = (bs[:, :, [k // 4 for k in range(16)]] > 0).any(axis=(0, 2))
    chroma = (bs[:, :, [k // 2 for k in range(8)]] > 0).any(axis=(0, 2))
    return np.stack([luma, chroma])


def expected_cuts(records, mbw, mbh, slice_rows=0, idc=0, trace=False):
    """(n_bands, 2) int: the column the rule chooses per band, luma and chroma.  With trace=True also a list of per-band dicts saying
    which branch chose it (tests use them to check that a fixture reaches what it means to reach)."""
    nb = n_bands(mbh)
    work = band_work(records, mbw, mbh, slice_rows, idc)
    first, last, target = window(mbw)
    cuts = np.zeros((nb, 2), np.int64)
    why = []
    for b in range(nb):
        t = dict(band=b, work=bool(work[b]), bound=None, above=None, free=0)
        if not work[b]:
            t["branch"] = "idle"
            why.append(t)
            continue
        busy = busy_columns(records, mbw, mbh, b)
        # 8.7.2.1: chroma edge bS is the corresponding luma edge's, so both planes see the same free columns -- a statement, checked
        assert np.array_equal(busy[0], busy[1]), ("luma and chroma disagree on the free columns", b)
        for plane in range(2):
            lo = first
            if b > 0 and has_top(b * DB_ROWS, slice_rows, idc):
                up = int(cuts[b - 1, plane])
                t["above"] = "idle" if not work[b - 1] else "whole" if up == mbw else "cut"
                if work[b - 1] and 0 < up < mbw:
                    lo = up
                    t["bound"] = up
            free = [c for c in range(max(lo, first), last + 1) if not busy[plane, c]]
            tgt = max(target, lo)
            cuts[b, plane] = min(free, key=lambda c: (abs(c - tgt), c < tgt)) if free else mbw
            t["free"] = len(free)
            t["free_in_window"] = int((~busy[plane, first:last + 1]).sum())
        c = int(cuts[b, 0])
        t["branch"] = "none" if c == mbw else "edge_left" if c == first else "edge_right" if c == last else "inner"
        t["forced_right"] = t["bound"] is not None and t["bound"] > target
        t["forced_none"] = c == mbw and t["free_in_window"] > 0
        why.append(t)
    assert np.array_equal(cuts[:, 0], cuts[:, 1])
    return (cuts, why) if trace else cuts


def cut_is_safe(records, mbw, mbh, band, col):
    """The property the cut rests on, independent of how the column was chosen: no split (col == mbw), or bS = 0 in every row and
    segment of the band on the left edge of column col (0: the picture's edge)."""
    if col == mbw:
        return True
    if not 0 <= col < mbw:
        return False
    return not (_band_edge_bs(records, mbw, mbh, band)[:, col] > 0).any()


def never_steps_left(cuts, mbw, mbh, slice_rows=0, idc=0):
    """Bands whose top edge is filtered and whose band above has a cut inside the row: their own cut, if inside the row, is not left of it.
    Returns the first offending band or None."""
    for b in range(1, len(cuts)):
        if has_top(b * DB_ROWS, slice_rows, idc) and 0 < cuts[b - 1] < mbw and 0 < cuts[b] < mbw and cuts[b] < cuts[b - 1]:
            return b
    return None
