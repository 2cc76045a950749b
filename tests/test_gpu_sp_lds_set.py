"""-m gpu: mj_k_sp ITSELF against the oracle on hardware.  Every launch of at most 20 k rows runs the small-pool schedule unless told
otherwise (mj_capi.hip: sp_launch -- mj_k_sp_promo + mj_k_sp_wide, which keep the child cache), so the lock-steps of
tests/test_gpu_parity.py below 65,536 tables, the directed hands of tests/test_gpu_state.py and the reference's bench kyoku never reach
the headline kernel and its two-choice hash set in LDS (sp_set_find_or_claim: ways claimed by ds_cmpst between real wavefronts, the
loser of a claim re-reading what won, the hand-over to the HBM tag table).  Every test here switches the schedule off before its pool
exists (MJ_SP_WIDE=0) and asserts that no launch used it, so none can silently test the other kernels.

The directed hands (tests/golden/sp_directed_hands.json, tools/gen_sp_directed_hands.py) add what bit parity cannot see: a race that
placed one state in two slots would leave every obs value right and only grow the row's number of states, so the device's count must
equal the one the emulator recorded with its uniqueness check on."""
import pytest

import parity_util

pytestmark = pytest.mark.gpu


def _only_mj_k_sp(st):
    assert st["counters"]["sp_overflow"] == 0
    assert st["sp_schedule"]["hybrid_launches"] == 0, st["sp_schedule"]


def test_mj_k_sp_greedy_64_tables_whole_hanchan(oracle, monkeypatch):
    """Greedy policy (hands at 0..3 shanten, riichi, calls, late-game rows), v4, 64 tables, whole hanchan: SP rows f32 bit for bit on
    EVERY cycle of the first 200 (the first kyoku: at most 70 draws, each with at most one round of calls behind it), every 4th cycle afterwards."""
    monkeypatch.setenv("MJ_SP_WIDE", "0")
    cycles = set(range(200)) | set(range(200, 3000, 4))
    st = parity_util.run_lockstep(oracle, 64, version=4, max_cycles=3000, obs_cycles=cycles, policy="greedy", sp_rows_checked=True)
    assert st["scores_checked"] == 64 and st["obs_checked"] > 20000
    _only_mj_k_sp(st)


def test_mj_k_sp_two_workgroups_chain_every_row(oracle, monkeypatch):
    """The same at 32 tables with MJ_SP_GRID=2: two workgroups take every row of every launch one after the other -- tag epochs, the
    stale ways of earlier rows in the set, four real wavefronts racing on each set."""
    monkeypatch.setenv("MJ_SP_WIDE", "0")
    monkeypatch.setenv("MJ_SP_GRID", "2")
    cycles = set(range(200)) | set(range(200, 3000, 4))
    st = parity_util.run_lockstep(oracle, 32, version=4, max_cycles=3000, obs_cycles=cycles, policy="greedy", sp_rows_checked=True)
    assert st["scores_checked"] == 32 and st["obs_checked"] > 10000
    _only_mj_k_sp(st)


def test_mj_k_sp_4096_tables_v4_obs(oracle, monkeypatch):
    """tests/test_gpu_parity.py::test_lockstep_4096_tables_v4_obs_with_sp on the other kernel: every workgroup chains many rows of the
    SP-heavy first turns."""
    monkeypatch.setenv("MJ_SP_WIDE", "0")
    st = parity_util.run_lockstep(oracle, 4096, version=4, max_cycles=223, obs_cycles={2, 37, 111, 222}, sp_rows_checked=True,
                                  deal_algo=1, threads=16)
    assert st["obs_checked"] > 10000
    _only_mj_k_sp(st)


def test_mj_k_sp_refill_and_stagger_512_tables(oracle, monkeypatch):
    """Refill + staggered starts at 512 tables, greedy: the row queue mixes every phase of a hanchan, at least two played generations
    per slot."""
    monkeypatch.setenv("MJ_SP_WIDE", "0")
    st = parity_util.run_lockstep(oracle, 512, version=4, max_cycles=20000, obs_every=29, sp_rows_checked=True, refill=128, stagger=300,
                                  min_games=2, deal_algo=1, policy="greedy", threads=16)
    assert st["generations"][0] >= 3 and st["games_checked"] >= 1024 and st["obs_checked"] > 10000  # (generation 1 = the staggered start)
    _only_mj_k_sp(st)


def test_mj_k_sp_directed_rows_and_their_state_counts(oracle, monkeypatch):
    """Every fixture hand on a one-table pool with the schedule off: the whole v4 obs equals the oracle's and the row's state count
    (mj_sp_phase_ticks word 7) equals the fixture's -- no state was placed twice, under real races, at the set's real capacity (the heavy
    rows fill its 2,048 ways and hand up to 4,174 states over to the HBM table)."""
    import test_sp_contention as D

    from libriichi.state import PlayerState

    monkeypatch.setenv("MJ_SP_WIDE", "0")
    hands = D.directed_hands()
    assert sum(h["kind"] == "heavy" and h["hbm"] > 0 for h in hands) >= 3
    for h in hands:
        n = D.check_directed_hand(oracle, PlayerState, h)
        print(f"{h['name']}: {n} states")
