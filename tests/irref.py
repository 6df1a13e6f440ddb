"""Plain numpy reference of periodic intra refresh (mi355enc_set_intra_refresh) -- test infrastructure.

Written from the rule as the issue and DESIGN state it, not from the encoder's code:

  * P picture number p >= 1 after the last IDR picture is picture j = (p - 1) mod N of a refresh cycle (N = cfg.gop); a(j) = floor(j * mbw / N).
  * A coded picture forces the macroblock columns [max(R - 1, 0), a(j + 1)) intra, R the first column the cycle has not refreshed yet (R = a(j)
    unless an all-skip picture of this cycle refreshed nothing), and then R = a(j + 1).  The cycle's first picture starts with R = 0.
  * An all-skip picture refreshes nothing.  The last picture of a cycle is never one: an all-skip picture wanted there moves to the next picture.
  * Left of the forced columns (mx < max(R - 1, 0)) an inter macroblock reads only luma columns <= 16 R - 4 (counting the six-tap support of a
    fractional position) and chroma columns <= 8 R - 2 (counting the bilinear neighbour): deblocking of the reference's edge at 16 R put dirt on
    its last 3 luma and last chroma column of column R - 1.
  * In the refresh column next to the unrefreshed side (column a(j + 1) - 1, when a(j + 1) < mbw) Intra_4x4 block 5 may not use modes 3
    (diagonal down-left) and 7 (vertical-left): they read the macroblock above-right.
  * A decoder that starts at a cycle's first picture with any reference has exact luma columns < 16 a(j + 1) - 3 and chroma columns
    < 8 a(j + 1) - 1 in picture j, i.e. the whole picture from j = N - 1 on.
"""
DROP_SKIP = 255
DROP_MAX = 12


def a_col(j, mbw, n):
    return j * mbw // n


def luma_max_col(mx, mvx):
    """rightmost luma column a 16x16 partition of column mx reads with horizontal vector mvx (quarter samples): 8.4.2.2.1, six taps"""
    return 16 * mx + 15 + (mvx >> 2) + (3 if mvx & 3 else 0)


def chroma_max_col(mx, mvx):
    """... and chroma column (4:2:0, eighth samples): 8.4.2.2.2, two taps"""
    return 8 * mx + 7 + (mvx >> 3) + (1 if mvx & 7 else 0)


def luma_ok(mx, mvx, clean):
    return luma_max_col(mx, mvx) <= clean


def chroma_ok(mx, mvx, clean):
    return chroma_max_col(mx, mvx) <= clean // 2


def vector_ok(mx, mvx, pic):
    """an inter macroblock of column mx in picture `pic` (an entry of schedule()) may use horizontal vector mvx"""
    if pic is None or pic["kind"] != "p" or mx >= pic["c0"]:
        return True
    return luma_ok(mx, mvx, pic["clean"]) and chroma_ok(mx, mvx, pic["clean"])


def i4_mode_ok(pic, mx, mbw, blk, mode):
    """Intra_4x4 mode of block blk (blkIdx) in column mx: not 3 / 7 in block 5 of the refresh column next to the unrefreshed side"""
    if pic is None or pic["kind"] != "p" or blk != 5 or mode not in (3, 7):
        return True
    return not (mx == pic["c1"] - 1 and pic["c1"] < mbw)


def schedule(mbw, n, wants):
    """wants: per picture 'idr' (an IDR picture: the first one, a forced key unit, a scene cut), 'p', or 'skip' (rate control or the caller wants
    an all-skip picture).  Returns one dict per picture: kind ('idr' / 'p' / 'skip'), j (-1 for IDR), start (a cycle's first picture), c0, c1
    (forced columns), clean (luma bound of the inter macroblocks left of c0, -1: none), R (first column not refreshed after the picture)."""
    out, p, R, owed = [], 0, 0, False
    for want in wants:
        if want == "idr":
            p, R, owed = 0, 0, False
            out.append(dict(kind="idr", j=-1, start=False, c0=0, c1=0, clean=-1, R=0))
            p += 1
            continue
        j = (p - 1) % n
        if j == 0:
            R = 0
        last = j == n - 1
        skip = want == "skip"
        if skip and last:
            skip, owed = False, True
        elif owed and not last:
            skip, owed = True, False
        if skip:
            out.append(dict(kind="skip", j=j, start=j == 0, c0=0, c1=0, clean=-1, R=R))
        else:
            c0, c1 = max(R - 1, 0), a_col(j + 1, mbw, n)
            out.append(dict(kind="p", j=j, start=j == 0, c0=c0, c1=c1, clean=16 * R - 4 if R > 0 else -1, R=c1))
            R = c1
        p += 1
    return out


def exact_cols(pic, mbw):
    """a decoder that joined at the cycle's first picture: (luma, chroma) columns below which picture `pic` is exact"""
    R = pic["R"]
    if R >= mbw:
        return 16 * mbw, 8 * mbw
    return max(16 * R - 3, 0), max(8 * R - 1, 0)
