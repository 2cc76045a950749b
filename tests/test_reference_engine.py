"""BASELINE configs[0]: the reference's own `mortal/engine.py` (MortalEngine) over `mortal/model.py` (Brain, DQN), random-init
tiny models, playing `libriichi.arena.OneVsThree.py_vs_py` — the call `mortal/one_vs_three.py:77-97` makes — and checked against
the reference-shaped oracle loop driven by the same two engines through the reference's list-of-ndarray contract.  The engines
are recorded (tests/golden/record_reference_engines.py -> tests/golden/reference_*) and replayed by
tests/recorded_engine.RecordedEngine: a decision whose obs or mask differs bit for bit from what the reference engine saw fails.

Runs on CPU: the arena's device kernels execute on the host SIMT emulator (tests/host/emu)."""
import os
import sys

import numpy as np
import pytest

REAL = os.environ.get("MORTAL_AMD_CFG0_REAL") == "1"  # on an MI355X (profiles/r06_cfg0_real_library.log): the real libmortal_amd.so and the networks on cuda:0
KEY = 0xD5DFAA4CEF265CD7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
if HOST not in sys.path:
    sys.path.insert(0, HOST)


def _oracle_rankings(oracle, chal, cham, seed_start, seed_count, version, deal_algo):
    """BatchGame::run (arena/game.rs:286-304) on the oracle; engines get the reference's contract: lists of per-row arrays."""
    n = seed_count * 4
    seeds = [(seed_start[0] + g // 4, seed_start[1]) for g in range(n)]
    arena = oracle.Arena(seeds, deal_algo=deal_algo, enable_quick_eval=True, version=version, keep_log=False)
    while arena.n_live > 0:
        rows = arena.poll()
        k = len(rows)
        obs, masks = arena.encode(0, k, want_obs=True)
        act = np.full(k, 45, dtype=np.int32)
        if k:
            is_chal = rows[:, 1] == rows[:, 0] % 4
            for eng, sel in ((chal, is_chal), (cham, ~is_chal)):
                idx = np.flatnonzero(sel)
                if len(idx):
                    a, _q, _m, _g = eng.react_batch([obs[i] for i in idx], [masks[i].astype(bool) for i in idx], None)
                    act[idx] = a
        arena.commit(act)
    rankings = [0, 0, 0, 0]
    for g in range(n):
        sc = arena.result(g)[0]
        order = sorted(range(4), key=lambda i: -int(sc[i]))
        rankings[order.index(g % 4)] += 1
    return rankings


@pytest.mark.parametrize("version", [4, 2])
def test_reference_engine_plays_one_vs_three(oracle, version):
    from libriichi.arena import OneVsThree

    from mortal_amd import arena as A

    import recorded_engine as R

    chal, cham = (R.RecordedEngine(R.decisions(f"v{version}", who), version, who) for who in R.ENGINES)
    old = A.BatchRunner.pool_cls
    if not REAL:  # (REAL: the product's own TablePool over libmortal_amd.so)
        import emu_pool

        A.BatchRunner.pool_cls = emu_pool.make_pool_class()
    try:
        env = OneVsThree(disable_progress_bar=True)
        got = env.py_vs_py(challenger=chal, champion=cham, seed_start=(10000, KEY), seed_count=1)
    finally:
        A.BatchRunner.pool_cls = old
    from mortal_amd.pool import default_deal_algo

    want = _oracle_rankings(oracle, chal, cham, (10000, KEY), 1, version, default_deal_algo())
    assert sum(got) == 4 and got == want == R.fixture()["one_vs_three"][f"v{version}"]["rankings"]
    print(f"reference engine.py + model.py (recorded), py_vs_py v{version} on {'libmortal_amd.so' if REAL else 'the host emulator'}: rankings {got} == oracle loop")
