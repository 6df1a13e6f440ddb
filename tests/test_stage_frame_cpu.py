"""The single-stage entry points without a device ("The stage entry points"): a call without a handle is refused by the entry point's own
argument check, in front of the frame and of any HIP call -- on a machine without a GPU a HIP call would fail and answer MI355ENC_ERR_HIP with a line on
stderr, on one with a GPU the null handle would be read."""
import ctypes as C

import numpy as np
import pytest

from tests import stageframe as SF


@pytest.fixture(scope="module")
def table(E):
    buf = np.zeros(SF.BUF_BYTES, np.uint8)
    return SF.entries(E, buf, buf.ctypes.data), buf


def test_the_table_names_every_stage_entry_point(E, table):
    assert sorted(name for name, _, _ in table[0]) == sorted(n for n in E.EXPORTS if n.startswith("mi355enc_stage_"))


def test_every_stage_entry_point_refuses_a_null_handle(E, table, capfd):
    L = E.load()
    for name, args, _ in table[0]:
        assert getattr(L, name)(None, *args) == E.ERR_ARG, name
    assert "mi355enc:" not in capfd.readouterr().err  # (what HIPCHK prints for a HIP call that failed)


@pytest.mark.parametrize("stage", range(-1, 30))
def test_time_stage_refuses_a_null_handle_at_every_stage(E, stage, capfd):
    ms = C.c_double(0)
    assert E.load().mi355enc_time_stage(None, stage, 1, C.byref(ms)) == E.ERR_ARG
    assert "mi355enc:" not in capfd.readouterr().err
