"""GPU: every input step keeps an aligned device input out of the in-place exit, and runs ("The input path").  mi355enc_submit_device
codes 16-byte-aligned planes of a picture without margins where they lie -- unless a step changes the samples, which the table of steps answers
(steps_active) -- or the frame rate is converted.  A step missing there would be skipped for such input without a word: tests/test_input_chain_gpu.py submits
device planes at an odd address, tests/test_input_paths_gpu.py takes the exit with every step off.  Here each step is on alone, on the smallest picture
at which the exit can be taken at all (chainref.PICTURES["E"]: 64 x 48, no margins, planes at a 256-byte-aligned address with a stride of 64), and held
to a second handle with the same settings that is fed the same pictures from host memory, a path the other tests hold to tests/chainref.py."""
import numpy as np
import pytest

from tests import chainref as C
from tests import maskref
from tests import rateref
from tests.test_input_chain_gpu import NS, ONE, _submit, _submit_device, drive, encoder

pytestmark = pytest.mark.gpu

NAME, N = "E", 3
MASK = [(16, 8, 32, 24, maskref.PIXELATE, 8)]  # one pixelate region inside the picture
CASES = list(ONE) + ["mask", "rate-hold"]


def case_of(case):
    """-> (the settings of every submit, encoder keywords, the pts, the rate mode, what the steps' references make of the sources or None)"""
    src = C.sources(NAME, N)
    if case == "rate-hold":  # inputs at 20 a second for 30: pictures are kept and repeated, and that never in the caller's planes
        return [{}] * N, dict(rate=(rateref.HOLD, NS, 2), fps=30, yuv=False), [i * NS // 20 for i in range(N)], rateref.HOLD, None
    if case == "mask":
        return [{}] * N, dict(yuv=False), None, rateref.OFF, [maskref.apply(y, uv, MASK) for y, uv in src]
    yuv = case == "colour-step"
    sets = [ONE[case](C.all_on(NAME))] * N
    return sets, dict(yuv=yuv), None, rateref.OFF, [o["visible"] for o in C.compose(C.handle(NAME, yuv=yuv), src, sets)]


def differs(a, b):
    return not np.array_equal(a[0], b[0]) or not np.array_equal(a[1], b[1])


@pytest.mark.parametrize("case", CASES)
def test_a_step_that_is_on_keeps_an_aligned_device_input_out_of_the_in_place_exit_and_runs(E, case):
    w, h = C.PICTURES[NAME]["size"]
    assert C.coded(w, h) == (w, h)  # (no margins: the exit's first condition)
    src = C.sources(NAME, N)
    sets, kw, pts, mode, ref = case_of(case)
    if ref is not None:  # by the steps' own references the step changes at least one of the pictures: a surface that differs from its source shows it ran
        assert any(differs(r, s) for r, s in zip(ref, src))
    out = {}
    for entry in ("device", "host"):
        e = encoder(E, NAME, **kw)
        if case == "mask":
            e.set_mask(MASK)
        feed, _, after = _submit_device(E, e, NAME, src, stride=w, offset=0, pts=pts) if entry == "device" else _submit(E, e, NAME, src, pts=pts)
        got, counts, _, _ = drive(E, e, sets, feed, pts, mode, records=False)
        e.close()
        if after:
            after()  # the caller's device planes are byte for byte what was submitted
        out[entry] = (got, counts)
    (dev, dev_counts), (host, host_counts) = out["device"], out["host"]
    assert dev_counts == host_counts and len(dev) == len(host) >= N
    for i, (g, r) in enumerate(zip(dev, host)):
        assert np.array_equal(g["y"], r["y"]) and np.array_equal(g["uv"], r["uv"]), i  # FETCH_SOURCE_Y / _UV at every collect
        assert g["au"] == r["au"], i
    if case != "rate-hold":
        assert any(differs((g["y"], g["uv"]), s) for g, s in zip(dev, src))
