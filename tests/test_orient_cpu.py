"""CPU: the host's statement of the orientation rule (mi355enc_orient_size / mi355enc_orient_source, enc_orient.cpp) against tests/orientref.py,
and the group laws both must obey."""
import numpy as np
import pytest

from tests import orientref as R

SIZES = [(6, 4), (4, 6)]


def through_host(E, a, method):
    """`a` oriented sample by sample through the host mapping"""
    h, w = a.shape
    ow, oh = E.orient_size(method, w, h)
    out = np.empty((oh, ow), a.dtype)
    for y in range(oh):
        for x in range(ow):
            sx, sy = E.orient_source(method, ow, oh, x, y)
            out[y, x] = a[sy, sx]
    return out


@pytest.mark.parametrize("method", range(8), ids=R.NAMES)
@pytest.mark.parametrize("wh", SIZES, ids=lambda s: "%dx%d" % s)
def test_host_mapping_equals_the_reference(E, wh, method):
    w, h = wh
    a = np.arange(w * h, dtype=np.int32).reshape(h, w)
    assert E.orient_size(method, w, h) == R.size(method, w, h)
    ref = R.plane(a, method)
    assert ref.shape == R.size(method, w, h)[::-1]
    assert np.array_equal(through_host(E, a, method), ref)
    assert E.orient_size(R.NAMES[method], w, h) == R.size(method, w, h)  # (the mirror takes names as well)


@pytest.mark.parametrize("wh", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("method,times", [(1, 4), (4, 2), (6, 2), (3, 4), (2, 2), (5, 2), (7, 2)], ids=lambda v: str(v))
def test_repeated_methods_give_the_identity(E, wh, method, times):
    w, h = wh
    a = np.arange(w * h, dtype=np.int32).reshape(h, w)
    r, g = a, a
    for k in range(times):
        r, g = R.plane(r, method), through_host(E, g, method)
        if k < times - 1:
            assert not np.array_equal(r, a) or method == 0
    assert np.array_equal(r, a) and np.array_equal(g, a)


def test_the_pairs_of_an_nv12_picture_stay_whole(E):
    """the reference's NV12 form against the host mapping applied to the plane of pairs: a pair moves as one unit"""
    y, uv = R.noise(6, 4, 1)
    pairs = uv.reshape(2, 3, 2).astype(np.uint16)
    packed = pairs[:, :, 0] | (pairs[:, :, 1] << 8)
    for m in range(8):
        oy, ouv = R.orient(y, uv, m)
        assert np.array_equal(oy, through_host(E, y, m))
        op = through_host(E, packed, m)
        assert np.array_equal(ouv[:, 0::2], op & 255) and np.array_equal(ouv[:, 1::2], op >> 8)
        assert oy.shape == R.size(m, 6, 4)[::-1] and ouv.shape == (oy.shape[0] // 2, oy.shape[1])
        assert (ouv[:, 0::2] < 128).all() and (ouv[:, 1::2] >= 128).all()
        assert sorted(oy.ravel()) == sorted(y.ravel())
    assert np.array_equal(R.orient(y, uv, 1)[0], np.rot90(y, -1)) and np.array_equal(R.orient(y, uv, 7)[0], y[::-1, ::-1].T)


def test_bad_arguments(E):
    L = E.load()
    import ctypes as C
    a, b = C.c_int(0), C.c_int(0)
    for m in (-1, 8):
        assert L.mi355enc_orient_size(m, 6, 4, C.byref(a), C.byref(b)) == E.ERR_ARG
        assert L.mi355enc_orient_source(m, 6, 4, 0, 0, C.byref(a), C.byref(b)) == E.ERR_ARG
    assert L.mi355enc_orient_size(1, 0, 4, C.byref(a), C.byref(b)) == E.ERR_ARG
    assert L.mi355enc_orient_size(1, 6, -2, C.byref(a), C.byref(b)) == E.ERR_ARG
    assert L.mi355enc_orient_size(1, 6, 4, None, C.byref(b)) == E.ERR_ARG
    for x, y in ((-1, 0), (0, -1), (4, 0), (0, 6)):  # 90r of 6 x 4 is 4 x 6
        assert L.mi355enc_orient_source(1, 4, 6, x, y, C.byref(a), C.byref(b)) == E.ERR_ARG
    assert L.mi355enc_orient_source(1, 4, 6, 3, 5, None, C.byref(b)) == E.ERR_ARG
    assert L.mi355enc_orient_source(1, 4, 6, 3, 5, C.byref(a), C.byref(b)) == 0
    assert L.mi355enc_get_orientation(None) == E.ERR_ARG and L.mi355enc_set_orientation(None, 1) == E.ERR_ARG
    with pytest.raises(ValueError):
        E.orient_method("sideways")
