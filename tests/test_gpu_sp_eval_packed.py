"""-m gpu: the evaluation's triangular sums on pairs of terms (mj_sp.hip: sp_eval_wave0 / sp_eval_wave, mj_algo.h: sp_div_domain2)
against the oracle.  64 tables under the greedy policy, first starts staggered over 160 cycles, then 48 cycles in which every row's
whole obs (SP rows 889..1011 included) is compared f32 bit for bit; the compared rows hold every T from 17 down to 1 and every
(instantiation, off) -- counted on the oracle alone, tests/sp_eval_packed_cases.py.  Once through mj_k_sp alone (the headline kernel) and
once through the small-pool schedule with every eligible row parked (mj_k_sp_promo / mj_k_sp_wide share the evaluation functions)."""
import pytest

import sp_eval_packed_cases as cases

pytestmark = pytest.mark.gpu


def _pool_cls():
    from mortal_amd.pool import TablePool

    return TablePool


def test_packed_sums_mj_k_sp_alone(oracle, monkeypatch):
    monkeypatch.setenv("MJ_SP_WIDE", "0")
    st, c = cases.run(oracle, _pool_cls(), threads=8)
    cases.check(st, c)
    assert st["sp_schedule"]["hybrid_launches"] == 0, st["sp_schedule"]


def test_packed_sums_small_pool_schedule_every_row_parked(oracle, monkeypatch):
    monkeypatch.setenv("MJ_SP_WIDE", "1")
    monkeypatch.setenv("MJ_SP_PROMO_MIN1", "1")
    monkeypatch.setenv("MJ_SP_PROMO_MIN2", "1")
    st, c = cases.run(oracle, _pool_cls(), threads=8)
    cases.check(st, c)
    sc = st["sp_schedule"]
    assert sc["hybrid_launches"] > 0 and sc["rows_promoted"] + sc["rows_swept"] > 100, sc
