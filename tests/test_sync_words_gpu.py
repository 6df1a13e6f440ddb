"""The words kernels wait on against the host's account of them (csrc/enc_sync.hpp): after a short stream the device's counting words equal the totals the
host booked from plan_launches(), at the smallest size of each launch shape -- the intra rows inside the deblocking launch, the gated fused stage without row
counts, the QP_Y chain leading the launch, bands walked in two parts -- and no bounded wait ran out on the way."""
import numpy as np
import pytest

from ceracoder_amd import enc as E
from ceracoder_amd import synth

pytestmark = pytest.mark.gpu

N, GOP, QP = 12, 4, 30


def _stream(w, h, depth, **kw):
    """12 pictures through an exclusive encoder; (host totals, device words, key frames, error word, recoveries) after the last collect"""
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, exclusive=True, scenecut=False, intra_in_p=1, **kw)
    try:
        keys = []
        for i, (y, uv) in enumerate(synth.s2_frames(w, h, N)):
            e.submit(y, uv, pts=i)
            if e.pending > depth:
                keys.append(e.collect()[1])
        while e.pending:
            keys.append(e.collect()[1])
        return e.debug_get_counters(), e.sync_words(), sum(bool(k) for k in keys), e.error_word(), int(e.stats().recoveries), e.mbw, e.mbh
    finally:
        e.close()


def _check(host, dev, err, recoveries):
    print("host", {k: host[k] for k in ("pmb_rows_total", "db_started_total", "ip_done_total", "qpc_total")}, "device", dev, "error word", err, "recoveries", recoveries)
    assert err == 0 and recoveries == 0
    for k in ("db_started_total", "ip_done_total", "qpc_total"):
        assert dev[k] == host[k], k
    assert np.array_equal(dev["row_done"], np.full(len(dev["row_done"]), host["pmb_rows_total"], np.uint32))


def test_rows_inside_the_deblocking_launch():
    """320x144, three pictures in flight: 20 x 9 macroblocks, three bands walked whole; every P picture's fused stage counts its rows and its intra rows ride in
    the deblocking launch"""
    host, dev, n_idr, err, rec, mbw, mbh = _stream(320, 144, 2)
    _check(host, dev, err, rec)
    assert n_idr == N // GOP
    assert host["pmb_rows_total"] == (N - n_idr) * mbw and host["ip_done_total"] == (N - n_idr) * mbh and host["qpc_total"] == 0


def test_gated_without_row_counts():
    """the same with two pictures in flight: the fused stage is gated, the deblocking launch follows it by event"""
    host, dev, n_idr, err, rec, mbw, mbh = _stream(320, 144, 1)
    _check(host, dev, err, rec)
    assert host["pmb_rows_total"] == 0 and host["ip_done_total"] == 0 and host["db_started_total"] == N * 2 * ((mbh + 3) // 4)


def test_qp_chain_leads_the_launch():
    """adaptive quantisation at depth 2: the chain's workgroup leads every deblocking launch and counts the picture's rows; the intra rows stay a kernel of their own"""
    host, dev, n_idr, err, rec, mbw, mbh = _stream(320, 144, 2, aq=True)
    _check(host, dev, err, rec)
    assert host["qpc_total"] == N * mbh and host["ip_done_total"] == 0 and host["pmb_rows_total"] == (N - n_idr) * mbw


def test_bands_in_two_parts_count_four_workgroups():
    """960x144: 60 macroblocks per row, the cut is on -- a P picture's launch counts four workgroups per band, an IDR picture's two"""
    host, dev, n_idr, err, rec, mbw, mbh = _stream(960, 144, 2)
    _check(host, dev, err, rec)
    nb = (mbh + 3) // 4
    assert (mbw, nb, n_idr) == (60, 3, N // GOP)
    assert host["db_started_total"] == (N - n_idr) * 4 * nb + n_idr * 2 * nb == 126
