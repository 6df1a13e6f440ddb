"""State that outlives a picture, host side (DESIGN.md "State that outlives a picture"): the 33-bit time stamps of the transport stream across their
wrap after 26.5 h.  Host only; the device-side tags and counts are in tests/test_longrun_gpu.py (with the state rule of the hook that presets them: it
needs an open handle)."""
import numpy as np

from tests.test_tsmux_cpu import AUD, Mux, fake_au
from tests.tsdemux import demux

M33 = (1 << 33) - 1


def _t90(pts_ns):
    """the muxer's 90 kHz time of a nanosecond time stamp (include/mi355ts.h: rounded down), not wrapped"""
    return pts_ns * 9 // 100000


def test_pts_and_pcr_across_two_to_the_33():
    """Access units at 60 Hz from 0.5 s before the stream time at which PTS (= time + 1 s) reaches 2^33 to 0.5 s after it: PTS and PCR are the 33-bit values
    of the unwrapped time (PTS wraps 7.5 pictures before PCR does: PCR trails by 125 ms), their distance is 11250 modulo 2^33 on every access unit,
    continuity counters and PSI CRCs hold (the demultiplexer asserts them), PAT / PMT keep their 100 ms cadence, and the payload is the input."""
    rng = np.random.default_rng(33)
    wrap = (1 << 33) - 90000  # the stream time, in 90 kHz ticks, at which PTS = 2^33
    ticks = [wrap - 45000 + 1500 * i for i in range(61)]  # 60 Hz: 1500 ticks per picture, 0.5 s either side; picture 30 is the first with a wrapped PTS
    times = [-(-k * 100000 // 9) for k in ticks]           # the first nanosecond of each tick
    assert [_t90(t) for t in times] == ticks and ticks[0] < wrap < ticks[-1]
    m = Mux()
    ts, aus = b"", []
    for i, t in enumerate(times):
        au = fake_au(rng, 300 + 7 * i, False)  # no key frames: PAT / PMT come from the 100 ms rule alone
        rc, out = m.mux(au, t, False)
        assert rc == 0
        ts += out
        aus.append(au)
    m.close()
    d = demux(ts)  # sync bytes, continuity counters per PID, PSI CRCs, PCR on every access unit start
    assert len(d["pes"]) == len(aus)
    wrapped_pts = wrapped_pcr = 0
    for p, au, t in zip(d["pes"], aus, times):
        want_pts, want_pcr = _t90(t) + 90000, _t90(t) + 90000 - 11250
        assert p["pts"] == want_pts & M33, (t, p["pts"], want_pts)
        assert p["pcr"] % 300 == 0 and p["pcr"] // 300 == want_pcr & M33, (t, p["pcr"], want_pcr)
        assert (p["pts"] - p["pcr"] // 300) & M33 == 11250
        wrapped_pts += want_pts > M33
        wrapped_pcr += want_pcr > M33
        assert bytes(p["data"]) == AUD + au
    assert 0 < wrapped_pcr < wrapped_pts < len(aus)  # both wrapped inside the clip, and on some access units only the PTS had
    # PAT + PMT in front of the first access unit and then whenever 100 ms (9000 ticks) of unwrapped stream time have passed since the last pair: at 60 Hz
    # every sixth access unit, across the wrap as before it
    pos = {idx: k for k, (kind, idx) in enumerate(d["order"]) if kind == "pes"}
    with_psi = [i for i in range(len(aus)) if pos[i] >= 2 and d["order"][pos[i] - 2][0] == "pat" and d["order"][pos[i] - 1][0] == "pmt"]
    want = list(range(0, len(aus), 6))
    assert with_psi == want and len(d["pat"]) == len(d["pmt"]) == len(want), (with_psi, want)
