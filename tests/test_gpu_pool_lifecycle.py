"""-m gpu: three pools created, played and destroyed in one process, each with everything a pool can own -- the small-pool
schedule's second stream, its two events and its pinned word besides the buffers and the step's events.  The owners of
mortal_amd/csrc/mj_host.h must release them in an order the real runtime accepts, and a pool must not depend on what the one
before it left behind.  Allocation failures themselves are tested on the emulator only (tests/test_emu_alloc_failures.py)."""
import pytest

import parity_util

pytestmark = pytest.mark.gpu


def test_three_pools_in_a_row_with_the_small_pool_schedule(oracle, monkeypatch):
    monkeypatch.setenv("MJ_SP_WIDE", "1")
    monkeypatch.setenv("MJ_SP_GRID", "8")
    runs = [parity_util.run_lockstep(oracle, 16, version=4, max_cycles=40, policy="greedy", sp_rows_checked=True, verbose=False)
            for _ in range(3)]  # (each compares every obs, mask and row list with the oracle, and closes its pool)
    assert runs[0]["obs_checked"] > 0 and runs[0]["sp_schedule"]["hybrid_launches"] > 0, runs[0]
    assert runs[1] == runs[0] and runs[2] == runs[0]
