"""GPU: the privacy masks (mi355enc_set_mask, k_mask.hip) -- the launches on noise, bit for bit against tests/maskref.py with the coded
margins as replicas, and streams: the access units of an encoder with masks on equal, byte for byte, those of a plain encoder fed maskref's pictures."""
import numpy as np
import pytest

from tests import chainref
from tests import imageref
from tests import maskref as R
from tests import overlayref
from tests import rateref
from tests import snapref
from tests.inputref import device_free
from tests.test_geometry_gpu import GOP, QP, nv12_clip, same
from tests.test_input_chain_gpu import ENTRY
from tests.test_yuv_convert_gpu import dev_get, dev_put

pytestmark = pytest.mark.gpu

FILL, PIX, BLUR = R.FILL, R.PIXELATE, R.BLUR
SURFACES = [(42, 26), (70, 50), (322, 182), (8192, 32)]  # coded 48 x 32, 80 x 64, 336 x 192 (regions span several workgroup tiles) and a strip without margins
MODES = [(FILL, 0), (PIX, 6), (BLUR, 3)]
_PROBE = {}


def probe(E, w, h):
    """an encoder of that size and a noise picture with replica margins, made once"""
    if (w, h) not in _PROBE:
        e = E.Encoder(w, h, fixed_qp=QP)
        rng = np.random.default_rng(w + h)
        vis = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
        _PROBE[w, h] = (e, vis, R.with_margins(*vis, 16 * e.mbw, 16 * e.mbh))
    return _PROBE[w, h]


def check(E, w, h, regs, changes=True):
    e, vis, (y, uv) = probe(E, w, h)
    gy, guv = e.mask_probe(regs, y, uv)
    wy, wuv = R.coded(*vis, regs, *y.shape[::-1], coef=E.csc_coefficients(1 if w > 1024 or h > 576 else 6, 0))  # (an unspecified matrix: by the picture's size)
    assert np.array_equal(gy, wy) and np.array_equal(guv, wuv), (regs, np.argwhere(gy != wy)[:4].tolist(), np.argwhere(guv != wuv)[:4].tolist())
    assert chainref.margins_are_replicas(gy, guv, w, h)
    assert changes != (np.array_equal(gy, y) and np.array_equal(guv, uv)), regs
    return gy, guv


@pytest.mark.parametrize("w,h", SURFACES[:3], ids=lambda v: str(v))
def test_probe_small_odd_outside_and_larger_regions(E, w, h):
    for mode, param in MODES + [(PIX, 4), (BLUR, 1), (BLUR, 32)]:
        check(E, w, h, [(10, 6, 2, 2, mode, param, 0, 0xC02040)])                      # a 2 x 2 region
        check(E, w, h, [(11, 7, 1, 1, mode, param, 1, 0xC02040)])                      # ... and the odd sample that rounds outward to one, as an ellipse
        check(E, w, h, [(-10, -12, w + 20, h + 30, mode, param, 0, 0x10F0A0)])         # larger than the picture
        check(E, w, h, [(3, 5, 17, 11, mode, param, 0, 0x808080)])                     # odd x, y, w, h
        check(E, w, h, [(w - 11, h - 9, 40, 40, mode, param, 0, 0x3060C0)])            # over the bottom-right visible corner: the margins are replicas
        for outside in ((w, 2, 10, 10), (w + 5, 2, 10, 10), (-10, 2, 10, 10), (2, h, 10, 10), (2, -10, 10, 10), (-16384, -16384, 16384, 16384)):
            check(E, w, h, [outside + (mode, param, 0, 0)], changes=False)             # wholly outside: nothing, and no error
    e = probe(E, w, h)[0]
    assert e.get_mask() is None  # (the probe is no part of the handle's own setting)


@pytest.mark.parametrize("w,h", SURFACES[:3], ids=lambda v: str(v))
def test_probe_pixelate_cells(E, w, h):
    for c in (4, 64, 8, 34):
        check(E, w, h, [(2, 2, 66, 20, PIX, c)])               # a 66-wide region: with c = 4 and 64 a two-column edge cell (at 42 wide the picture cuts it first)
        check(E, w, h, [(w - 13, h - 9, 30, 30, PIX, c)])      # a cell cut by the picture's edge
        check(E, w, h, [(-7, -5, 31, 23, PIX, c)])             # ... and by its top-left edge: the grid starts outside
        check(E, w, h, [(-7, -5, w + 20, h + 20, PIX, c, 1)])  # means over the rectangle's cell under an ellipse


@pytest.mark.parametrize("w,h", SURFACES[:3], ids=lambda v: str(v))
def test_probe_blur(E, w, h):
    check(E, w, h, [(5, 3, 30, 20, BLUR, 1)])
    check(E, w, h, [(8, 2, 6, 20, BLUR, 32)])                  # clamping dominates: the window is eleven times the region
    check(E, w, h, [(8, 2, 20, 6, BLUR, 32)])
    check(E, w, h, [(10, 10, 300, 70, BLUR, 32)])              # (322 x 182: several tiles each way; the smaller pictures clip it)
    check(E, w, h, [(0, 0, w, h, BLUR, 17)])
    for r in (2, 5, 16, 31):
        check(E, w, h, [(w // 2 - 9, 1, 19 + r, h - 3, BLUR, r)])


@pytest.mark.parametrize("w,h", SURFACES[:3], ids=lambda v: str(v))
def test_probe_ellipses(E, w, h):
    for mode, param in MODES + [(BLUR, 32), (PIX, 64)]:
        check(E, w, h, [(4, 2, 30, 18, mode, param, 1, 0xFFFFFF)])             # w != h
        check(E, w, h, [(-15, 4, 30, 18, mode, param, 1, 0xFF00FF)])           # half off the left edge: still that ellipse
        check(E, w, h, [(w - 12, h - 14, 40, 22, mode, param, 1, 0x00FF00)])   # off the bottom-right corner
        check(E, w, h, [(6, -30, 18, 60, mode, param, 1, 0x0000FF)])           # tall, off the top


@pytest.mark.parametrize("w,h", SURFACES[:3], ids=lambda v: str(v))
def test_probe_eight_overlapping_regions_the_lowest_index_wins(E, w, h):
    regs = [(6, 4, 24, 16, BLUR, 4, 1), (2, 2, 20, 14, PIX, 6), (14, 8, 22, 14, FILL, 0, 0, 0xE01010), (0, 0, w, h, BLUR, 9, 1), (10, 0, 12, h, PIX, 4, 1),
            (w - 20, h - 16, 30, 30, FILL, 0, 1, 0x1010E0), (-4, h - 12, w + 8, 20, BLUR, 32), (0, 0, w, h, PIX, 64)]
    gy, guv = check(E, w, h, regs)
    e, vis, (y, uv) = probe(E, w, h)
    # region 0's quads are region 0's result alone, whatever lies behind it; and the order matters
    ay, auv = R.apply(*vis, regs[:1])
    m = R.membership(R.region(regs[0]), w, h)
    assert np.array_equal(gy[:h, :w][np.repeat(np.repeat(m, 2, 0), 2, 1)], ay[np.repeat(np.repeat(m, 2, 0), 2, 1)])
    ry, _ = check(E, w, h, regs[::-1])
    assert not np.array_equal(ry, gy)
    # eight blurs of the whole picture overlap and do not fit the ping-pong planes together: batches, the same bytes as the first alone
    by, buv = check(E, w, h, [(0, 0, w, h, BLUR, 3 + k) for k in range(8)])
    oy, ouv = check(E, w, h, [(0, 0, w, h, BLUR, 3)])
    assert np.array_equal(by, oy) and np.array_equal(buv, ouv)


def test_probe_on_the_8192_strip_a_region_across_the_full_width(E):
    w, h = SURFACES[3]
    check(E, w, h, [(0, 0, w, h, BLUR, 32)])
    check(E, w, h, [(-3, 1, w + 6, h - 3, PIX, 64, 1)])
    check(E, w, h, [(1, 3, w - 2, 9, FILL, 0, 0, 0x204060), (0, 0, w, h, BLUR, 5, 1), (4000, 0, 300, 32, PIX, 10)])


def test_probe_refusals_and_colours(E):
    e, vis, (y, uv) = probe(E, 70, 50)
    for bad in ([(0, 0, 4, 4, BLUR, 33)], [(0, 0, 4, 4, PIX, 5)], [(0, 0, 0, 4, FILL, 0)], [(0, 0, 4, 4, 4, 0)]):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.mask_probe(bad, y, uv)
    for full, matrix in ((1, 1), (0, 9)):  # the fill colour follows the output's matrix and range
        f = E.Encoder(70, 50, fixed_qp=QP, colorimetry=(full, 2, 2, matrix))
        regs = [(3, 5, 17, 11, FILL, 0, 0, 0xC04020)]
        gy, guv = f.mask_probe(regs, y, uv)
        wy, wuv = R.coded(*vis, regs, 80, 64, coef=E.csc_coefficients(matrix, full))
        assert np.array_equal(gy, wy) and np.array_equal(guv, wuv)
        f.close()


def test_close_the_probes(E):
    for e, _, _ in _PROBE.values():
        e.close()
    _PROBE.clear()


# ---- streams
W, H, NPIC = 70, 50, 8
SETS = [[(3, 5, 17, 11, BLUR, 4)], [(20, 10, 30, 30, PIX, 8, 1)], [(w0, 4, 20, 20, FILL, 0, 0, 0x4080C0) for w0 in (2, 40)], [],
        [(W - 11, H - 9, 40, 40, BLUR, 32, 1), (0, 0, W, H, PIX, 64)], [(100, 100, 10, 10, BLUR, 3)], [(0, 0, W, H, BLUR, 2)], [(1, 1, 9, 9, PIX, 4), (5, 5, 40, 30, FILL, 0, 1, 0xFFFFFF)]]


def masked(pics, sets):
    return [R.apply(y, uv, regs) if regs else (y, uv) for (y, uv), regs in zip(pics, sets)]


def plain(E, pictures, depth=2, w=W, h=H, setup=None, **kw):
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, **kw)
    if setup:
        setup(e)
    res = stream(e, lambda i: e.submit(*pictures[i], pts=i), len(pictures), depth)[0]
    e.close()
    return res


def stream(e, feed, n, depth=2, before=None):
    """-> ((access units, reconstruction), the pictures' last_mask)"""
    out, last = [], []
    for i in range(n):
        if before:
            before(i)  # (with the pipeline full: depth + 1 pictures in flight)
        if e.pending > depth:
            out.append(e.collect())
            last.append(e.last_mask())
        feed(i)
    while e.pending:
        out.append(e.collect())
        last.append(e.last_mask())
    return (out, (e.fetch(0), e.fetch(1))), last


@pytest.mark.parametrize("depth", [0, 2])
def test_stream_with_the_mask_changing_on_every_picture(E, depth):
    pics = nv12_clip(W, H, NPIC, 900)
    want = masked(pics, SETS)
    assert sum(not np.array_equal(a[0], b[0]) for a, b in zip(want, pics)) == 6  # (none, and one wholly outside)
    ref = plain(E, want, depth)
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=depth)
    assert e.get_mask() is None and e.debug_mask_bytes() == 0  # off by default
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.last_mask()

    def before(i):
        assert e.pending == min(i, depth + 1)  # earlier pictures are in flight with their own masks
        e.set_mask(SETS[i])
        assert e.get_mask() == ([R.region(r) for r in SETS[i]] or None)
        if i == 0:
            assert e.debug_mask_bytes() == 0  # nothing is allocated before the first masked picture

    got, last = stream(e, lambda i: e.submit(*pics[i], pts=i), NPIC, depth, before)
    assert e.debug_mask_bytes() == 3 * 80 * 64 * 3 // 2
    assert [r for r, _ in last] == [[R.region(r) for r in s] for s in SETS] and [g for _, g in last] == [1, 2, 3, 0, 4, 5, 6, 7]
    # the last picture's coded surfaces: the reference's picture and its replicas
    wy, wuv = R.with_margins(*want[-1], 80, 64)
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), wy) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), wuv)
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        e.set_mask([(0, 0, 4, 4, BLUR, 33)])  # refused: the configuration stays
    assert e.get_mask() == [R.region(r) for r in SETS[-1]]
    e.close()
    same(got, ref)


@pytest.mark.parametrize("entry", list(ENTRY))
def test_through_every_submit_entry_point(E, entry):
    n = 3
    src = chainref.sources("A", n)
    sets = [SETS[4], SETS[0] + SETS[1], SETS[7]]
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    feed, vis, after = ENTRY[entry](E, e, "A", src)
    got, _ = stream(e, feed, n, 2, lambda i: e.set_mask(sets[i]))
    e.close()
    if after:
        after()  # (submit_device: the caller's planes are unchanged)
    same(got, plain(E, masked(vis, sets)))


def test_submit_device_on_aligned_surfaces_is_still_masked_and_the_callers_surface_is_unchanged(E):
    """64 x 48 on 16-byte-aligned planes would take the in-place exit, which codes from the caller's memory: with a mask it must not"""
    w, h = 64, 48
    pics = nv12_clip(w, h, 3, 905)
    sets = [[(10, 6, 30, 20, BLUR, 6, 1)], [(40, 30, 40, 40, PIX, 8)], []]
    ref = plain(E, masked(pics, sets), w=w, h=h)
    dev = [(dev_put(y), dev_put(uv)) for y, uv in pics]
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    got, _ = stream(e, lambda i: e.submit_device(dev[i][0], w, dev[i][1], w, pts=i), 3, 2, lambda i: e.set_mask(sets[i]))
    e.close()
    for (dy, duv), (y, uv) in zip(dev, pics):
        assert np.array_equal(dev_get(dy, y.shape), y) and np.array_equal(dev_get(duv, uv.shape), uv)
        device_free(dy); device_free(duv)
    same(got, ref)


def test_an_image_layer_and_a_text_are_drawn_on_top_of_the_mask(E):
    """order: mask, layer, text -- a layer and a text over a blurred region stay sharp"""
    pics = nv12_clip(W, H, 4, 906)
    regs = [(0, H - 30, W, 30, BLUR, 8), (W - 30, 0, 30, H, PIX, 10, 1)]
    img = imageref.random_image(np.random.default_rng(41), 24, 16)
    layer = imageref.layer(img, W - 20, H - 12, 200)
    text = ("M1", dict(halign=overlayref.LEFT, valign=overlayref.BOTTOM, xpad=2, ypad=0, scale=1, shaded_background=1))
    coef = imageref.coefficients(6, 0, 80, 64)
    want, other = [], []
    for y, uv in pics:
        my, muv = R.apply(y, uv, regs)
        want.append(overlayref.draw(*imageref.blend(my, muv, [layer], coef), text[0], **text[1]))
        other.append(R.apply(*overlayref.draw(*imageref.blend(y, uv, [layer], coef), text[0], **text[1]), regs))
    assert all(not np.array_equal(a[0], b[0]) for a, b in zip(want, other))  # (the other order is another picture)
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    e.set_mask(regs)
    e.set_image(0, layer["pixels"], layer["x"], layer["y"], layer["opacity"], E.FMT_RGBX)
    e.set_overlay_style(**text[1])
    e.set_overlay_text(text[0])
    got, _ = stream(e, lambda i: e.submit(*pics[i], pts=i), 4)
    wy, wuv = R.with_margins(*want[-1], 80, 64)
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), wy) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), wuv)
    e.close()
    same(got, plain(E, want))


def test_under_a_rate_conversion_hold_the_repeated_picture_carries_its_own_latchs_mask(E):
    ns = 10 ** 9
    pics = nv12_clip(W, H, 3, 907)
    a, b = [(4, 4, 30, 20, BLUR, 5)], [(30, 20, 30, 20, PIX, 6, 1)]
    e = E.Encoder(W, H, fps=60, gop=GOP, fixed_qp=QP, pipeline_depth=2, rate=(rateref.HOLD, ns, 2))
    e.set_mask(a)
    assert e.submit(*pics[0], pts=0) == 1
    e.collect()
    first = R.with_margins(*R.apply(*pics[0], a), 80, 64)
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), first[0]) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), first[1]) and e.last_mask() == ([R.region(a[0])], 1)
    e.set_mask(b)
    assert e.submit(*pics[1], pts=ns // 30) == 2  # the tick in between repeats picture 0 -- unmasked on the device -- under the mask set now, not blurred twice
    e.collect()
    held = R.with_margins(*R.apply(*pics[0], b), 80, 64)
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), held[0]) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), held[1]) and e.last_mask() == ([R.region(b[0])], 2)
    e.collect()
    own = R.with_margins(*R.apply(*pics[1], b), 80, 64)
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), own[0]) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), own[1])
    e.set_mask(None)
    assert e.submit(*pics[2], pts=2 * ns // 30) == 2  # ... and off: the held picture is picture 1 as it came in
    e.collect()
    bare = R.with_margins(*pics[1], 80, 64)
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), bare[0]) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), bare[1]) and e.last_mask() == ([], 0)
    e.collect()
    e.close()


def test_a_coded_picture_still_and_the_quality_metrics_see_the_mask(E):
    from tests import qualityref as Q
    pics = nv12_clip(W, H, 3, 908)
    regs = [(10, 6, 40, 30, BLUR, 7, 1), (0, 0, 20, 20, FILL, 0, 0, 0x20C040)]
    want = masked(pics, [regs] * 3)
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=0)
    e.set_quality_metrics(True)
    e.set_mask(regs)
    for i in range(3):
        if i == 1:
            e.request_snapshot(E.SNAP_SOURCE, 1, 75)
        e.submit(*pics[i], pts=i)
        e.collect()
        wy, wuv = R.with_margins(*want[i], 80, 64)
        assert e.last_quality().ints() == Q.quality(wy, wuv, e.fetch(E.FETCH_RECON_Y), e.fetch(E.FETCH_RECON_UV), W, H), i
        if i == 1:
            still = e.take_snapshot()
            assert still is not None and still[0] == snapref.still(*want[1], 1, 75)
    e.close()


def test_off_after_on_is_never_on_and_a_never_masked_handle_allocates_nothing(E):
    pics = nv12_clip(W, H, 6, 909)
    sets = [SETS[0], SETS[4], [], [], [], []]
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    got, last = stream(e, lambda i: e.submit(*pics[i], pts=i), 6, 2, lambda i: e.set_mask(sets[i] or None))
    assert e.get_mask() is None and [g for _, g in last] == [1, 2, 0, 0, 0, 0]
    py, puv = R.with_margins(*pics[-1], 80, 64)  # (off, the coded surfaces are the input path's: the picture and its replicas)
    assert np.array_equal(e.fetch(E.FETCH_SOURCE_Y), py) and np.array_equal(e.fetch(E.FETCH_SOURCE_UV), puv)
    e.close()
    same(got, plain(E, masked(pics, sets)))
    # on and off again before the first picture, and a region that never reaches the picture: the plain stream, and nothing was allocated
    ref = plain(E, pics)
    for regs in (None, [(200, 200, 10, 10, BLUR, 4)]):
        e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=2)
        e.set_mask(SETS[0])
        e.set_mask(regs)
        got, _ = stream(e, lambda i: e.submit(*pics[i], pts=i), 6)
        assert e.debug_mask_bytes() == 0
        for stage in (E.STAGE_MASK_CELLS, E.STAGE_MASK_BLUR):
            if regs is None:
                with pytest.raises(E.EncoderError, match=r"\(-6\)"):
                    e.time_stage(stage, 2)
        e.close()
        same(got, ref)


def test_the_timed_stages_run_and_the_handle_encodes_correctly_after_them(E):
    pics = nv12_clip(W, H, 4, 910)
    regs = [(4, 4, 40, 30, BLUR, 6), (30, 10, 30, 30, PIX, 8, 1), (0, 30, 20, 20, FILL, 0, 0, 0x808080)]
    ref = plain(E, masked(pics, [regs] * 4))
    e = E.Encoder(W, H, gop=GOP, fixed_qp=QP, pipeline_depth=2)
    e.set_mask(regs[:1])
    assert e.time_stage(E.STAGE_MASK_BLUR, 2) > 0
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.time_stage(E.STAGE_MASK_CELLS, 2)  # (no fill or pixelate region in the value set last)
    e.set_mask(regs)
    assert e.time_stage(E.STAGE_MASK_CELLS, 2) > 0 and e.time_stage(E.STAGE_MASK_BLUR, 2) > 0
    got, _ = stream(e, lambda i: e.submit(*pics[i], pts=i), 4)
    e.close()
    same(got, ref)
