"""Picture controls without a device: mi355enc_adjust_tables against the restatement in tests/adjustref.py -- exactly where the rule is
integers (gamma 1000), within one code of the double model elsewhere -- the literal cases of the rule, the argument ranges at each edge, and the identity of
sharpen -16 with the rounded binomial blur, which adjustref's step must satisfy."""
import numpy as np
import pytest

from ceracoder_amd import enc as E
from tests import adjustref as A


def sweep(seed, n, gamma_1000):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        a = {k: int(rng.integers(lo, hi + 1)) if rng.integers(8) else int((lo, hi)[int(rng.integers(2))]) for k, (lo, hi) in A.RANGES.items()}
        if gamma_1000:
            a["gamma"] = 1000
        yield a, int(rng.integers(2))


def test_neutral_is_the_identity_and_no_rotation():
    for full in (0, 1):
        luma, chroma = E.adjust_tables(A.params(), full)
        assert np.array_equal(luma, np.arange(256)) and tuple(chroma) == (4096, 0)
    assert E.adjust(None).as_dict() == A.NEUTRAL and E.adjust_check() == 0


def test_literal_cases():
    for s in (1, -1):
        assert tuple(E.adjust_tables(A.params(hue=s * 500))[1]) == (0, s * 4096)
        assert tuple(E.adjust_tables(A.params(hue=s * 1000))[1]) == (-4096, 0)
    assert tuple(E.adjust_tables(A.params(saturation=0))[1]) == (0, 0)
    assert tuple(E.adjust_tables(A.params(saturation=0, hue=333))[1]) == (0, 0)
    luma = E.adjust_tables(A.params(contrast=2000), 0)[0]
    assert (luma[16], luma[126], luma[136]) == (16, 236, 255)


def test_integer_table_equals_the_restatement_and_rotation_is_within_one():
    n = 0
    for a, full in sweep(2301, 3000, True):
        luma, chroma = E.adjust_tables(a, full)
        assert np.array_equal(luma, A.luma_table_int(a, full)), (a, full)
        cu, su = A.chroma_model(a)
        assert abs(int(chroma[0]) - np.round(cu)) <= 1 and abs(int(chroma[1]) - np.round(su)) <= 1, (a, tuple(chroma), cu, su)
        n += 1
    assert n == 3000


def test_gamma_table_is_within_one_code_of_the_model_and_non_decreasing():
    for a, full in sweep(2302, 2000, False):
        luma = E.adjust_tables(a, full)[0].astype(np.int64)
        model = np.clip(A.luma_model(a, full), 0.0, 255.0)
        assert np.max(np.abs(luma - model)) <= 1.0, (a, full)
        assert np.all(np.diff(luma) >= 0), (a, full)
    for a, full in sweep(2303, 500, True):  # ... the integer path too
        assert np.all(np.diff(E.adjust_tables(a, full)[0].astype(np.int64)) >= 0), (a, full)


@pytest.mark.parametrize("name", sorted(A.RANGES))
def test_ranges_are_refused_one_past_each_edge(name):
    lo, hi = A.RANGES[name]
    for v, ok in ((lo - 1, False), (lo, True), (lo + 1, True), (hi - 1, True), (hi, True), (hi + 1, False)):
        assert (E.adjust_check(**{name: v}) == 0) == ok, (name, v)
        if ok:
            E.adjust_tables(A.params(**{name: v}), 0)
        else:
            with pytest.raises(E.EncoderError):
                E.adjust_tables(A.params(**{name: v}), 0)
    with pytest.raises(E.EncoderError):
        E.adjust_tables(A.params(), 2)


def test_sharpen_minus_16_is_the_rounded_binomial_blur():
    rng = np.random.default_rng(2304)
    for shape in ((16, 16), (37, 53)):
        for y in (rng.integers(0, 256, shape, dtype=np.uint8), rng.choice(np.array([0, 255], np.uint8), shape)):
            blur = ((A.binomial_sum(y) + 8) >> 4).astype(np.uint8)
            assert np.array_equal(A.sharpen(y, -16, 0), blur)
            assert np.array_equal(A.sharpen(y, -16, 32), blur)  # (the threshold is used for sharpen > 0 only)
    flat = np.full((8, 8), 77, np.uint8)
    assert np.array_equal(A.sharpen(flat, 64, 0), flat)
