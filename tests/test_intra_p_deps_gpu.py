"""Intra macroblocks of P pictures reconstructed by dependency (intra_p_row: runs of adjacent intra macroblocks spread over wave pairs, the row
below waiting for the epoch-tagged bottom lines of exactly the macroblocks it predicts from): whole streams against the oracle, picture by
picture, on clips whose P pictures are dense in intra macroblocks -- runs of many and isolated ones, at the picture's edges and across slice
seams -- at 1080p (intra_p_kernel) and 720p (the intra rows riding in the deblocking launch), with Intra_4x4 in P pictures and the 8x8
transform on and off, one and three pictures in flight."""
import numpy as np
import pytest

from ceracoder_amd import synth
from tests.util import first_diff

pytestmark = pytest.mark.gpu


def _mask(mbw, mbh):
    """Macroblocks (True) that get a new, unpredictable content at the cut: a block of long runs at the left edge, isolated macroblocks on a
    checkerboard (diagonal neighbours only: top-left / top-right dependencies without a left one), a column band at the right edge through
    every row (every slice seam), and whole rows around the first slice seam."""
    m = np.zeros((mbh, mbw), bool)
    m[2:6, 0:mbw // 3] = True
    for y in range(mbh // 2, min(mbh, mbh // 2 + 6)):
        m[y, (y % 2)::3] = True
    m[:, mbw - 3:] = True
    s = max(1, mbh // 4)
    m[s - 1:s + 1, mbw // 2:] = True
    return m


def partial_cut_clip(w, h, n, cut):
    """S2 clip where, from picture `cut` on, the macroblocks of _mask come from the S3 (noise) generator: a partial scene cut."""
    a = list(synth.s2_frames(w, h, n))
    b = list(synth.s3_frames(w, h, n))
    m = _mask((w + 15) // 16, (h + 15) // 16)
    my = np.kron(m, np.ones((16, 16), bool))[:h, :w]
    muv = np.kron(m, np.ones((8, 16), bool))[:h // 2, :w]
    out = []
    for i in range(n):
        y, uv = a[i][0].copy(), a[i][1].copy()
        if i >= cut:
            y[my] = b[i][0][my]
            uv[muv] = b[i][1][muv]
        out.append((np.ascontiguousarray(y), np.ascontiguousarray(uv)))
    return out


def _run(E, oracle, w, h, n, ip, t8, depth, slices=4):
    qps = [30, 26, 34, 31, 24]
    oracle.set_features(oracle.F_ALL | (oracle.F_I4P if ip == 2 else 0))
    oracle.set_transform8x8(t8)
    try:
        e = E.Encoder(w, h, gop=60, fixed_qp=30, pipeline_depth=depth, exclusive=depth > 0, slices=slices, slice_deblock=True, intra_in_p=ip,
                      transform8x8=t8, scenecut=False)
        oe = oracle.Encoder(w, h, gop=60, threads=16, p_slices=slices, slice_deblock_local=True, scenecut=False)
        clip = partial_cut_clip(w, h, n, 2)
        got = []
        for i, (y, uv) in enumerate(clip):
            e.set_fixed_qp(qps[i % len(qps)])
            e.submit(y, uv, pts=i)
            if e.pending > depth:
                got.append(e.collect()[0])
        while e.pending:
            got.append(e.collect()[0])
        intra = []
        for i, (y, uv) in enumerate(clip):
            ref_au, key = oe.encode(y, uv, qps[i % len(qps)])
            assert got[i] == ref_au, ("bitstream", i, len(got[i]), len(ref_au))
            if not key:
                intra.append(int((oe.mbinfo["mb_type"] != 1).sum()))
        assert np.array_equal(e.fetch(E.FETCH_RECON_Y), oe.recon_y), first_diff(e.fetch(E.FETCH_RECON_Y), oe.recon_y)
        assert np.array_equal(e.fetch(E.FETCH_RECON_UV), oe.recon_uv)
        assert e.stats().recoveries == 0
        e.close()
        return intra
    finally:
        oracle.set_features(oracle.F_ALL)
        oracle.set_transform8x8(False)


@pytest.mark.parametrize("w,h", [(1920, 1080), (1280, 720)])
@pytest.mark.parametrize("ip", [1, 2])
@pytest.mark.parametrize("t8", [False, True])
@pytest.mark.parametrize("depth", [0, 2])
def test_partial_cut_equals_oracle(E, oracle, w, h, ip, t8, depth):
    """Every picture of a clip with a partial scene cut, bit for bit; the P pictures after the cut hold many intra macroblocks in runs and alone."""
    intra = _run(E, oracle, w, h, 5, ip, t8, depth)
    m = _mask((w + 15) // 16, (h + 15) // 16)
    assert max(intra) >= int(m.sum()) // 10, intra  # (noise is not always coded intra: about a fifth of it at QP 26..34)


@pytest.mark.parametrize("w,h,slices", [(1920, 1080, 1), (1280, 720, 3), (176, 144, 2)])
def test_partial_cut_other_slicings_equal_oracle(E, oracle, w, h, slices):
    """The same with one slice (every row predicts from the row above) and with other seams, and a picture narrower than a row of runs."""
    intra = _run(E, oracle, w, h, 4, 1, False, 2, slices=slices)
    assert max(intra) > 0, intra
