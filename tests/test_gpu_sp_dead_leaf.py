"""-m gpu: tests/test_sp_dead_leaf.py on hardware, at 256 tables.  Rows with as many draws left as their shanten number skip their
tenpai level (mj_sp.hip: leaf_dead, sp_expand_dead_chunk); a staggered, refilling pool is pre-rolled in obs v3 for 800 cycles and then
compared with the oracle for 20 cycles of obs v4, every row's SP block f32 bit for bit (tests/sp_dead_leaf_cases.py).  The oracle
alone gives this window 226 such rows (56 / 114 / 56 at 1 / 2 / 3 shanten, 29 without a discard), 219 rows with one draw more and
181 with one draw less; the conditions are those of the 64-table emulator test times four, the kernel's count of the rows that took
the path must equal the oracle's, and nothing may overflow.  Once through mj_k_sp alone (the headline kernel, MJ_SP_WIDE=0) and once
through the small-pool schedule (mj_k_sp_promo parks large rows, mj_k_sp_wide finishes them -- the dead level included -- and takes
rows from the queue itself)."""
import pytest

import sp_dead_leaf_cases as cases

pytestmark = pytest.mark.gpu

N_TABLES, PRE, WINDOW = 256, 800, 20


def _pool_cls():
    from mortal_amd.pool import TablePool

    return TablePool


def test_dead_leaf_rows_mj_k_sp_alone(oracle, monkeypatch):
    monkeypatch.setenv("MJ_SP_WIDE", "0")
    st, c, ticks = cases.run(oracle, _pool_cls(), N_TABLES, PRE, WINDOW, threads=8)
    cases.check(st, c, ticks, 4)
    assert st["sp_schedule"]["hybrid_launches"] == 0, st["sp_schedule"]


def test_dead_leaf_rows_small_pool_schedule(oracle, monkeypatch):
    monkeypatch.setenv("MJ_SP_WIDE", "1")
    monkeypatch.setenv("MJ_SP_PROMO_MIN1", "24")
    monkeypatch.setenv("MJ_SP_PROMO_MIN2", "6")
    st, c, ticks = cases.run(oracle, _pool_cls(), N_TABLES, PRE, WINDOW, threads=8)
    cases.check(st, c, ticks, 4)
    sc = st["sp_schedule"]
    assert sc["hybrid_launches"] == WINDOW and sc["rows_promoted"] + sc["rows_swept"] > 100, sc
