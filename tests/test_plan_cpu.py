"""The stream schedule of one picture (ceracoder_amd/csrc/enc_plan.hpp: plan_picture) on every input: a stand-alone program, csrc/plan_driver.cpp, built with
g++ under ASan + UBSan, walks the full product of the inputs -- fifteen two-valued ones x intra_mode, intra_in_p, pipeline_depth in {0, 1, 2}: 884 736
cases -- and prints the plan of each.  Held (1) exactly against the restatement of the rule in tests/planref.py, and (2) against the invariants the
device-side waits rely on, stated here on their own.  Host code only."""
import os
import subprocess

import numpy as np
import pytest

from tests import planref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")
N_CASES = 2 ** len(planref.IN_BITS) * 3 ** len(planref.IN_INTS)
N_IN, N_OUT = len(planref.IN_BITS) + len(planref.IN_INTS), len(planref.OUT)


@pytest.fixture(scope="module")
def table():
    """one row of digits per input: the inputs (planref.IN_BITS, IN_INTS), then the plan (planref.OUT)"""
    r = subprocess.run(["make", "-C", CSRC, "san/plan_driver"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "plan_driver")], env=env, capture_output=True, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-3000:]
    width = N_IN + 1 + N_OUT + 1
    assert len(r.stdout) == N_CASES * width
    raw = np.frombuffer(r.stdout, np.uint8).reshape(N_CASES, width)
    assert (raw[:, N_IN] == ord(" ")).all() and (raw[:, -1] == ord("\n")).all()
    t = np.concatenate([raw[:, :N_IN], raw[:, N_IN + 1:-1]], axis=1).astype(np.int16) - ord("0")
    assert t.min() == 0 and t[:, :len(planref.IN_BITS)].max() == 1 and t[:, len(planref.IN_BITS):N_IN].max() == 2
    number = t[:, :N_IN].astype(np.int64) @ np.array([3 ** len(planref.IN_INTS) << k for k in range(len(planref.IN_BITS))] + [1, 3, 9])
    assert np.array_equal(np.sort(number), np.arange(N_CASES))  # every input, once
    t.setflags(write=False)
    return t


def test_plan_equals_the_restated_rule_on_every_input(table):
    want = np.array([planref.plan(*row) for row in table[:, :N_IN].tolist()], np.int16)
    bad = np.nonzero((want != table[:, N_IN:]).any(axis=1))[0]
    assert bad.size == 0, "%d of %d inputs differ; the first: in %s -> %s, the rule says %s" % (
        bad.size, N_CASES, dict(zip(planref.IN_BITS + planref.IN_INTS, table[bad[0], :N_IN].tolist())), table[bad[0], N_IN:].tolist(), want[bad[0]].tolist())


def test_plan_invariants_on_every_input(table):
    col = dict(zip(planref.IN_BITS + planref.IN_INTS, table[:, :N_IN].T))
    i = {k: v.astype(bool) for k, v in col.items() if k in planref.IN_BITS}
    intra_mode, intra_in_p, depth = col["intra_mode"], col["intra_in_p"], col["pipeline_depth"]
    o = dict(zip(planref.OUT, table[:, N_IN:].T))
    may_wait, split, pgate, prows, isplit, fip = (o[k].astype(bool) for k in planref.OUT[:6])
    idr, coded = i["idr"], ~i["all_skip"]  # (an all-skip picture comes first in every rule: the host writes it, nothing of it is scheduled)

    def implies(a, b):
        return (~a | b).all()

    # an all-skip picture has every flag false -- and, nothing of it being enqueued, no stream but the main one and no upload
    assert not table[i["all_skip"], N_IN:].any()
    # the chain of the P picture's overlaps, and what each flag needs
    assert implies(fip, prows) and implies(prows, pgate) and implies(pgate, may_wait)
    assert implies(split, may_wait & ~idr & (intra_in_p > 0))  # (c->intra_p is non-zero exactly when cfg.intra_in_p is)
    assert implies(isplit, idr & may_wait & (intra_mode != 1))
    assert implies(idr, ~(split | pgate | prows | fip))
    assert implies(prows, depth >= 2)
    assert implies(fip, ~i["prof"] & ~i["aq_mode"])
    # where no kernel may wait on the device for another one
    room = np.where(idr, i["wait_room1"], i["wait_room0"])
    for never in (~i["overlap_allowed"], ~i["exclusive_device"], i["deblock_mode"], i["keep_prefilter"], ~room, i["prof"] & idr, i["prof"] & ~idr & ~i["profile_overlap"]):
        assert never.any() and not may_wait[never].any()
    # ... and what follows from the flags
    assert ((o["gpu_done"] == planref.INTRA) == (split | pgate)).all() and np.isin(o["gpu_done"], (planref.MAIN, planref.INTRA)).all()
    # the device copy of the context is uploaded exactly when a kernel replayed from a graph reads it (of a coded picture: an all-skip picture has no context)
    assert (o["upload_ctx"].astype(bool) == (coded & ((idr & (intra_mode == 1)) | i["deblock_mode"]))).all()
    # the flags are not vacuous: each one is set somewhere
    assert all(f.any() for f in (may_wait, split, pgate, prows, isplit, fip))
