"""-m gpu: the staged insert pass of the expansion (mj_sp.hip: sp_expand_chunk, P4 -- decode, look, claim loop, HBM table, new states,
child-list entry) against the oracle on hardware, where the claims race between real wavefronts.
64 tables under the greedy policy, first starts staggered over 160 cycles, then 48 cycles in which every row's whole obs (SP rows
included) is compared f32 bit for bit (tests/sp_eval_packed_cases.py: rows of every shanten 0..3 and every T from 17 down to 1):
once through mj_k_sp alone (the LDS hash set), once through the small-pool schedule with every eligible row parked (mj_k_sp_promo /
mj_k_sp_wide: the child-cache form of the pass).  The heavy directed hands (tests/golden/sp_directed_hands.json) on a one-table pool
add the rounds bit parity does not reach in small rows -- thousands of states, the set's 2,048 ways full and the rest handed over to
the HBM table -- and what parity cannot see: a state placed twice would only grow the row's state count, which must be the fixture's."""
import pytest

import sp_eval_packed_cases as cases

pytestmark = pytest.mark.gpu


def _pool_cls():
    from mortal_amd.pool import TablePool

    return TablePool


def test_insert_stages_mj_k_sp_alone(oracle, monkeypatch):
    monkeypatch.setenv("MJ_SP_WIDE", "0")
    st, c = cases.run(oracle, _pool_cls(), threads=8)
    cases.check(st, c)
    assert st["sp_schedule"]["hybrid_launches"] == 0, st["sp_schedule"]


def test_insert_stages_small_pool_schedule_every_row_parked(oracle, monkeypatch):
    monkeypatch.setenv("MJ_SP_WIDE", "1")
    monkeypatch.setenv("MJ_SP_PROMO_MIN1", "1")
    monkeypatch.setenv("MJ_SP_PROMO_MIN2", "1")
    st, c = cases.run(oracle, _pool_cls(), threads=8)
    cases.check(st, c)
    sc = st["sp_schedule"]
    assert sc["hybrid_launches"] > 0 and sc["rows_promoted"] + sc["rows_swept"] > 100, sc


def test_heavy_directed_hands_keep_their_state_counts(oracle, monkeypatch):
    import test_sp_contention as D

    from libriichi.state import PlayerState

    monkeypatch.setenv("MJ_SP_WIDE", "0")
    heavy = [h for h in D.directed_hands() if h["kind"] == "heavy"]
    assert len(heavy) >= 3 and all(h["hbm"] > 0 for h in heavy)
    for h in heavy:
        n = D.check_directed_hand(oracle, PlayerState, h)  # whole v4 obs, no overflow, mj_k_sp alone, the fixture's state count
        print(f"{h['name']}: {n} states")
