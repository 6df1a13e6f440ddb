"""The stream schedule of one picture (ceracoder_amd/csrc/enc_plan.hpp: plan_picture) on every input: a stand-alone program, csrc/plan_driver.cpp, built with
g++ under ASan + UBSan, walks the full product of the inputs -- fifteen two-valued ones x intra_mode, intra_in_p, pipeline_depth in {0, 1, 2}: 884 736
cases -- and prints the plan of each.  Held (1) exactly against the restatement of the rule in tests/planref.py, and (2) against the invariants the
device-side waits rely on, stated here on their own.  The same driver then walks plan_launches() -- which kernel the two launches that wait on the device run,
their workgroups, what they add to the counts device and host keep in step -- over every (plan, IDR, qp_off) the first walk produced, with and without the
parts' words, at every size of planref.SIZES_*: held exactly against planref.launches(), the rule the launchers decoded from their pointer arguments before, and
against its own invariants; open()'s wait_room rule against the workgroup count it used to call; and the booking of the uint32 totals past their wrap.
Host code only."""
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


# ---- the launches that follow from a plan (plan_launches), open()'s wait_room rule, the booking of the host's totals
def _run_driver(*args):
    r = subprocess.run(["make", "-C", CSRC, "san/plan_driver"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "plan_driver")] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def launch_table():
    """(rows of planref.LAUNCH_IN + planref.LAUNCH_OUT, one per distinct (plan, idr, qp_off) of the walk x part_words x size; the "room" lines)"""
    lines = _run_driver("launches")
    rows = np.array([l.split() for l in lines if not l.startswith("room")], np.int64)
    rooms = np.array([l.split()[1:] for l in lines if l.startswith("room")], np.int64)
    assert rows.shape[1] == len(planref.LAUNCH_IN) + len(planref.LAUNCH_OUT) and 0 < len(rows) < 300000
    rows.setflags(write=False)
    return rows, rooms


def test_launches_walk_every_plan_the_schedule_produces(table, launch_table):
    rows, _ = launch_table
    n_plan = len(planref.OUT)
    idr, aq = planref.IN_BITS.index("idr"), planref.IN_BITS.index("aq_mode")
    want = {tuple(r) for r in np.unique(np.concatenate([table[:, N_IN:], table[:, [idr, aq]]], axis=1), axis=0).tolist()}  # every (plan, idr, qp_off) of the walk
    got = {tuple(r) for r in np.unique(rows[:, :n_plan + 2], axis=0).tolist()}
    assert got == want
    per = 2 * len(planref.SIZES_MBW) * len(planref.SIZES_MBH)
    assert len(rows) == per * len(want)  # each with and without the parts' words, at every size
    sizes = {tuple(r) for r in rows[:, n_plan + 3:n_plan + 5].tolist()}
    assert sizes == {(w, h) for w in planref.SIZES_MBW for h in planref.SIZES_MBH}


def test_launches_equal_the_rule_the_launchers_decoded(launch_table):
    rows, _ = launch_table
    n_in, n_plan = len(planref.LAUNCH_IN), len(planref.OUT)
    want = np.array([planref.launches(dict(zip(planref.OUT, r[:n_plan])), *r[n_plan:n_in]) for r in rows.tolist()], np.int64)
    bad = np.nonzero((want != rows[:, n_in:]).any(axis=1))[0]
    assert bad.size == 0, "%d of %d differ; the first: %s -> %s, the rule says %s" % (
        bad.size, len(rows), dict(zip(planref.LAUNCH_IN, rows[bad[0], :n_in].tolist())), rows[bad[0], n_in:].tolist(), want[bad[0]].tolist())


def test_launch_invariants(launch_table):
    rows, _ = launch_table
    c = dict(zip(planref.LAUNCH_IN + planref.LAUNCH_OUT, rows.T))
    b = {k: c[k].astype(bool) for k in ("fip", "db_rows", "db_follows_ip", "prows", "pgate", "idr", "qp_off", "part_words", "parts", "qpc")}
    variant, gate, mbw, mbh = c["variant"], c["gate"], c["mbw"], c["mbh"]

    def implies(a, x):
        return (~a | x).all()

    fused = variant == planref.DB_P_FUSED_IP
    assert implies(b["fip"], fused & b["db_rows"] & b["db_follows_ip"]) and implies(fused, b["fip"])
    assert implies(b["idr"], (variant == planref.DB_ALL_INTRA) & ~b["parts"] & (gate == planref.PMB_IN_ORDER)) and implies(variant == planref.DB_ALL_INTRA, b["idr"])
    assert implies(b["parts"], (mbw >= 60) & ~b["idr"] & b["part_words"])
    assert implies(b["qpc"], b["qp_off"])
    counted = np.where(b["parts"], 4, 2) * ((mbh + 3) // 4)
    assert (c["inc_started"] == counted).all() and (c["grid"] == counted + np.where(fused, mbh, np.where(b["qpc"], 1, 0))).all()
    assert ((gate == planref.PMB_GATED_ROWS) == b["prows"]).all() and implies(gate == planref.PMB_GATED, b["pgate"] & ~b["prows"])
    # device and host count the same: rows with the gated rows, the intra rows with the fused variant, the chain's rows with the chain
    assert (c["inc_rows"] == np.where(gate == planref.PMB_GATED_ROWS, mbw, 0)).all() and (c["inc_ip_done"] == np.where(fused, mbh, 0)).all()
    assert (c["inc_qpc"] == np.where(b["qpc"], mbh, 0)).all()
    # every variant and every gate occurs, and so do parts and the chain
    assert set(variant.tolist()) == {0, 1, 2, 3} and set(gate.tolist()) == {0, 1, 2} and b["parts"].any() and b["qpc"].any()


def test_wait_room_rule_is_the_workgroup_count_open_used(launch_table):
    _, rooms = launch_table
    assert len(rooms) == 4 * len(planref.SIZES_MBW) * len(planref.SIZES_MBH)
    for mbw, mbh, idr, fip_rows, wgs in rooms.tolist():
        assert wgs == planref.wait_wgs(mbw, mbh, idr, fip_rows), (mbw, mbh, idr, fip_rows)


@pytest.mark.parametrize("mbw,mbh", [(59, 9), (120, 68)])
def test_booked_totals_wrap_like_the_device_words(mbw, mbh):
    """uint32 totals over 2^32 / mbw + 3 pictures of each kind: the row total passes 2^32, and all four equal arithmetic modulo 2^32"""
    (line,) = _run_driver("book", mbw, mbh)
    v = [int(x) for x in line.split()]
    n, a, b, tot = v[0], v[1:5], v[5:9], v[9:13]
    assert n == 2 ** 32 // mbw + 3
    fused = dict(zip(planref.OUT, (1, 0, 1, 1, 0, 1, planref.INTRA, planref.MAIN, planref.INTRA, 0, 1, 1)))
    chain = dict(fused, fip=0, db_follows_ip=0)
    order = [5, 6, 7, 8]  # LAUNCH_OUT's inc_rows, inc_started, inc_ip_done, inc_qpc
    assert a == [planref.launches(fused, 0, 0, 1, mbw, mbh)[i] for i in order] and b == [planref.launches(chain, 0, 1, 1, mbw, mbh)[i] for i in order]
    assert a[0] == mbw and n * (a[0] + b[0]) >= 2 ** 32
    assert tot == [(n * (x + y)) % 2 ** 32 for x, y in zip(a, b)]
