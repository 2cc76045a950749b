"""-m gpu: the SP kernels' level-0 scoring pass with its inputs in registers (mj_sp.hip: sp_l0_score_all / sp_get_score, the inlined agari
code of mj_algo.h) against the oracle.  What a register-passed AgariIn can get wrong shows on tenpai rows with open melds (pons, chis and
kans in the decomposition, fu of open sets, the non-menzen yaku values), on yakuman shapes, and on riichi rows with more than one dora
indicator (the uradora table instead of the closed form) -- the greedy policy reaches all of them inside the first kyoku: the default
seeds at 64 tables give, in 200 cycles, 12,557 decision rows of which 5,264 belong to an open hand at three shanten or less, 1,739 see a
kan on the board (two or more dora indicators) and 549 of those are concealed hands (counted on the oracle alone)."""
import re

import pytest

import parity_util

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("schedule", ["mj_k_sp", "small_pool"])
def test_l0_scoring_greedy_64_tables_sp_block_bit_exact(oracle, monkeypatch, capfd, schedule):
    """64 tables, obs v4, greedy policy, 200 cycles, every cycle's whole obs (SP block included) f32 bit for bit; once through mj_k_sp
    alone (the headline kernel; a pool this small would otherwise never launch it) and once through the small-pool schedule
    (mj_k_sp_promo + mj_k_sp_wide), which share the scoring function.  The phase counters must show that level-0 items were scored."""
    if schedule == "mj_k_sp":
        monkeypatch.setenv("MJ_SP_WIDE", "0")
    monkeypatch.setenv("MJ_SP_PROF", "1")  # mj_counters prints the phase counters, the level-0 item count among them
    st = parity_util.run_lockstep(oracle, 64, version=4, max_cycles=200, obs_every=1, policy="greedy", sp_rows_checked=True)
    assert st["cycles"] == 200 and st["obs_checked"] > 10000
    assert st["counters"]["sp_overflow"] == 0
    assert (st["sp_schedule"]["hybrid_launches"] == 0) == (schedule == "mj_k_sp"), st["sp_schedule"]
    err = capfd.readouterr().err
    items = [int(x) for x in re.findall(r"\[sp prof\].*? l0-entries (\d+)", err)]
    assert items, err[-500:]
    print(f"{schedule}: level-0 items scored {items[-1]}")
    assert items[-1] > 10000  # (every tenpai state of every row brings a few)
