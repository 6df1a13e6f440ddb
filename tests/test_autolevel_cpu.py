"""Automatic levels and white balance without a device: the C statement (ceracoder_amd/csrc/autolevel_host.c, mi355enc_autolevel_decide)
against tests/autolevelref.py bit for bit -- seeded measurements and settings, the hand-made corners -- the setting's ranges, and the properties the rule
promises, on the restatement."""
import ctypes as C

import numpy as np
import pytest

from tests import autolevelref as R

CASES = R.decide_cases()


def both(E, m, a, full, state):
    """the reference's answer, after the C function has given the same one"""
    want = R.decide(m, a, full, state, prime=state is None)
    got = E.autolevel_decide(m, a, full, state, prime=state is None)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2], (got[0], want[0], got[2], want[2])
    return want


def test_exports_are_present(E):
    L = E.load()
    names = [n for n in E.EXPORTS if "autolevel" in n]
    assert len(names) == 10
    for n in names:
        getattr(L, n)
    assert L.mi355enc_abi_version() == 4
    assert (E.STAGE_AUTOLEVEL_MEASURE, E.STAGE_AUTOLEVEL_DECIDE, E.STAGE_AUTOLEVEL_APPLY) == (32, 33, 34)


def test_the_device_entry_points_refuse_a_null_handle_in_front_of_any_hip_call(E, capfd):
    L = E.load()
    buf = np.zeros(64 * 48 * 2, np.uint8)
    p = buf.ctypes.data
    a, info, m, st = E.autolevel(levels=1000), E.AutolevelInfo(), E.autolevel_meas(np.ones(256), 0, 0, 0, 1), (C.c_int32 * 4)()
    rect = (C.c_int * 4)(0, 64, 0, 48)
    assert L.mi355enc_autolevel_probe_stage(None, C.byref(a), p, p, C.byref(info), p) == E.ERR_ARG
    assert L.mi355enc_autolevel_probe_measure(None, p, p, 64, 48, C.byref(rect), 64, 48, 0, 48, C.byref(m)) == E.ERR_ARG
    assert L.mi355enc_autolevel_probe_decide(None, C.byref(m), C.byref(a), 0, 1, C.byref(st), C.byref(info), p) == E.ERR_ARG
    assert L.mi355enc_set_autolevel(None, C.byref(a)) == E.ERR_ARG and L.mi355enc_get_autolevel(None, C.byref(a)) == E.ERR_ARG
    assert L.mi355enc_last_autolevel(None, None, None, None) == E.ERR_ARG and L.mi355enc_debug_autolevel_bytes(None) == 0
    ms = C.c_double(0)
    for stage in (32, 33, 34, 35):
        assert L.mi355enc_time_stage(None, stage, 1, C.byref(ms)) == E.ERR_ARG
    assert "mi355enc:" not in capfd.readouterr().err  # (what HIPCHK prints for a HIP call that failed)


def test_default_is_off_and_check_at_every_edge(E):
    d = E.Autolevel()
    E.load().mi355enc_autolevel_default(C.byref(d))
    assert d.as_dict() == R.DEFAULT == E.autolevel().as_dict() and not R.active(d.as_dict())
    assert E.autolevel(levels=500, clip=7).as_dict() == dict(R.DEFAULT, levels=500, clip_low=7, clip_high=7)
    assert E.autolevel_check() == 0
    for field, (lo, hi) in R.RANGES.items():
        for edge in (lo, hi):
            for v in range(edge - 2, edge + 3):
                assert (E.autolevel_check(**{field: v}) == 0) == (lo <= v <= hi), (field, v)
    assert E.load().mi355enc_autolevel_check(None) == E.ERR_ARG
    with pytest.raises(TypeError):
        E.autolevel(gain=3)


def test_decide_refuses_what_the_rule_does_not_cover(E):
    m = dict(hist=np.full(256, 10), voters=10, su=1000, sv=1000, chroma=100)
    on = dict(levels=1000, balance=1000)
    E.autolevel_decide(m, on, 0, None, prime=True)
    for bad in (dict(m, voters=101), dict(m, su=2551), dict(m, sv=2551), dict(m, chroma=(1 << 24) + 1), dict(m, hist=np.full(256, 1 << 19))):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            E.autolevel_decide(bad, on, 0, None, prime=True)
    for state in ((-1, 0, 0, 0), (0, 65281, 0, 0), (0, 0, -32769, 0), (0, 0, 0, 32768)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            E.autolevel_decide(m, on, 0, state)
        E.autolevel_decide(m, on, 0, state, prime=True)  # (priming does not read it)
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        E.autolevel_decide(m, dict(on, speed=0), 0, None, prime=True)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_made_cases(E, case):
    name, m, a, full, state = case
    rec, table, st = both(E, m, a, full, state)
    B, S = R.black_scale(full)
    assert B <= rec["lo"] <= B + S and B <= rec["hi"] <= B + S
    if name.startswith("flat"):  # a pure offset with gain max_gain: the table's slope through the picture's code
        assert rec["lo"] == rec["hi"]
        v = rec["lo"]
        L, span = _interval(a, full, st)
        assert span == -((-256000 * S) // 2000) and L <= 256 * v <= L + span
    if name.startswith("clips0"):
        assert (rec["lo"], rec["hi"]) == (max(3, B), min(250, B + S))
    if name.startswith("clips-"):
        assert (rec["lo"], rec["hi"]) == (60, 180)
    if name == "below-limited":  # (the full range has nothing below its black level)
        assert rec["lo"] == rec["hi"] == B
    if name.startswith("voters-at"):
        assert rec["valid"] == 1 and (rec["du"], rec["dv"]) == (256 * 12, -256 * 8) and (rec["off_u"], rec["off_v"]) == (12, -8)
    if name.startswith(("voters-under", "no-voters")):
        assert rec["valid"] == 0 and (rec["s_du"], rec["s_dv"]) == (500, -700)
    if name.startswith("speed256"):
        assert (rec["s_lo"], rec["s_hi"], rec["s_du"], rec["s_dv"]) == (256 * rec["lo"], 256 * rec["hi"], rec["du"], rec["dv"])
    if name.startswith("speed1-"):
        assert rec["s_lo"] == 256 * 100 + ((256 * rec["lo"] - 256 * 100) >> 8) and rec["s_du"] == -3000 + ((rec["du"] + 3000) >> 8)
    if name.startswith("gain1000"):
        assert np.array_equal(table[B:B + S + 1], np.arange(B, B + S + 1))
    if name.startswith("negative-du"):
        bal = R.params(a)["balance"]
        assert rec["s_du"] < 0 and rec["s_dv"] < 0
        assert rec["off_u"] == int(np.floor((rec["s_du"] * bal + 128000) / 256000)) and rec["off_v"] == int(np.floor((rec["s_dv"] * bal + 128000) / 256000))
    if name.startswith("levels0"):
        assert np.array_equal(table[B:B + S + 1], np.arange(B, B + S + 1))
    if name.startswith("balance0"):
        assert (rec["off_u"], rec["off_v"]) == (0, 0) and rec["valid"] == 1


def _interval(a, full, st):
    """(L, span) of a state, as the rule makes them"""
    a = R.params(a)
    B, S = R.black_scale(full)
    L = 256 * B + ((st[0] - 256 * B) * a["levels"]) // 1000
    T = 256 * (B + S) - ((256 * (B + S) - st[1]) * a["levels"]) // 1000
    smin = -((-256000 * S) // a["max_gain"])
    if T - L >= smin:
        return L, T - L
    L = ((L + T) >> 1) - (smin >> 1)
    L = min(max(L, 256 * B), 256 * (B + S) - smin)
    return L, smin


def test_seeded_measurements_and_settings(E):
    rng = np.random.default_rng(2028)
    seen = dict(prime=0, invalid=0, limited=0, negative=0)
    for _ in range(3000):
        m, a, full, state = R.random_case(rng)
        rec, table, st = both(E, m, a, full, state)
        B, S = R.black_scale(full)
        # the table is non-decreasing and inside [B, B + S]
        assert np.all(np.diff(table.astype(int)) >= 0) and table[0] >= B and table[255] <= B + S
        seen["prime"] += state is None
        seen["invalid"] += not rec["valid"]
        seen["limited"] += _interval(a, full, st)[1] == -((-256000 * S) // a["max_gain"])
        seen["negative"] += rec["off_u"] < 0
    assert min(seen.values()) > 100, seen


def test_primed_at_full_strength_the_points_map_to_the_ends_of_the_range(E):
    rng = np.random.default_rng(5)
    n = 0
    for _ in range(400):
        m, a, full, _ = R.random_case(rng)
        a = dict(a, levels=1000)
        rec, table, st = both(E, m, a, full, None)
        B, S = R.black_scale(full)
        if 256 * (rec["hi"] - rec["lo"]) >= -((-256000 * S) // a["max_gain"]):
            assert table[rec["lo"]] == B and table[rec["hi"]] == B + S
            n += 1
    assert n > 50


@pytest.mark.parametrize("full", [0, 1])
def test_speed_16_on_a_constant_input_settles_within_a_sixteenth(E, full):
    B, S = R.black_scale(full)
    hist = np.zeros(256, np.int64)
    hist[B + 30], hist[B + 150] = 500, 500
    m = dict(hist=hist, voters=600, su=600 * 141, sv=600 * 117 + 300, chroma=1000)
    a = dict(levels=800, balance=900, speed=16)
    for state in ((256 * B, 256 * (B + S), -30000, 30000), (256 * (B + S), 256 * B, 32767, -32768)):
        inside = 0
        for _ in range(200):
            rec, _, state = both(E, m, a, full, state)
            err = [abs(256 * rec["lo"] - state[0]), abs(256 * rec["hi"] - state[1]), abs(rec["du"] - state[2]), abs(rec["dv"] - state[3])]
            if max(err) < 16:
                inside += 1
            else:
                assert inside == 0, err  # once inside it stays
        assert inside > 50


def test_off_then_on_primes_and_the_c_chain_equals_the_references(E):
    """the clip of the stream tests, off at 6 and 7: the record of picture 8 is that of a primed picture, and a chain kept with the C function gives the reference's"""
    w, h = 64, 48
    pics = R.clip(w, h)
    on = dict(levels=900, balance=800, speed=64)
    settings = [None if i in (6, 7) else on for i in range(len(pics))]
    ref = R.chain(pics, settings)
    assert ref[6][2] == R.ZERO and ref[8][2]["s_lo"] == 256 * ref[8][2]["lo"] and ref[8][2]["s_du"] == ref[8][2]["du"]
    assert ref[5][2]["s_lo"] != 256 * ref[5][2]["lo"] and not np.array_equal(ref[5][0], pics[5][0])
    assert ref[4][2]["off_u"] == 0 and ref[9][2]["off_u"] > 0 and ref[9][2]["off_v"] < 0  # the cast appears at picture 5 and is followed
    state, primed = None, False
    for (y, uv), a, want in zip(pics, settings, ref):
        if a is None:
            primed = False
            continue
        rec, table, state = E.autolevel_decide(R.measure(y, uv, reach=R.params(a)["reach"]), a, 0, state, prime=not primed)
        primed = True
        assert rec == want[2] and np.array_equal(table, want[3])
