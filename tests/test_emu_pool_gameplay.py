"""Training samples and Grp from a pool's device log (mortal_amd/csrc/mj_gameplay.hip behind mj_replay_load_pool / mj_pool_grp /
mj_grp_logs; GameplayLoader.load_pool, TablePool.log_grp, Grp.from_packed), run on the host emulation of the device code.  The
cases and their yardsticks live in tests/pool_gameplay_cases.py, shared with the `-m gpu` leg."""
import gc
import os
import shutil
import sys

import numpy as np
import pytest

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
if HOST not in sys.path:
    sys.path.insert(0, HOST)

from emu_alloc import first_samples as _first_samples, stats as _stats  # noqa: E402
import pool_gameplay_cases as G  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    import emu_pool

    return emu_pool.make_pool_class()


@pytest.fixture(scope="module")
def played(emu):
    """Three finished games and their logs as the host reads them, shared and left unchanged."""
    pool = G.play(emu, 3)
    yield pool, pool.read_logs()
    pool.close()


def test_pool_route_equals_the_reference_loader(oracle, emu, played):
    pool, logs = played
    assert G.check_range(oracle, pool, logs, 3, 1, [15, 6], True) > 500


def test_invisible_obs_from_the_seed(oracle, emu):
    assert G.check_invisible(oracle, emu, n=2, version=1) > 400


def test_skipped_in_mid_run_and_a_table_in_error(oracle, emu):
    G.check_skipped_and_error(oracle, emu, n=3, victim=1)


def test_refused_calls_leave_the_destination_usable(emu, played):
    G.check_refusals(emu, played[0])


def test_grp_golden_game(emu):
    G.check_grp_golden(emu._L)


def test_grp_truncated_and_empty_logs(emu):
    G.check_grp_truncated(emu._L)


def test_grp_batch_of_130_cuts(emu, monkeypatch):
    G.check_grp_batch(emu._L)
    monkeypatch.setenv("MJ_LOG_GRID", "2")  # two workgroups: every wavefront takes 16 or 17 logs, one after the other
    G.check_grp_batch(emu._L)


def test_grp_tagged_log(emu):
    G.check_grp_tagged(emu._L)


def test_batch_runner_gameplays(oracle, emu):
    """BatchRunner.gameplays after run(): the engines' names by seat, the samples of the reference loader."""
    import test_sharding as TS

    from mortal_amd import arena as A
    from mortal_amd import mjai_log as ML
    from mortal_amd.dataset import GameplayLoader

    old = A.BatchRunner.pool_cls
    A.BatchRunner.pool_cls = emu
    try:
        seeds = [(10000, G.KEY), (10001, G.KEY)]
        aos = np.array([0b0001, 0b0100], dtype=np.uint8)
        runner = A.BatchRunner([TS._LowestLegalEngine("a"), TS._LowestLegalEngine("b")], seeds, aos, deal_algo=0, keep_stat=True)
        runner.run()
        loader = GameplayLoader(3, oracle=False, player_names=["b"])
        got = runner.gameplays(loader)
        logs = runner.pool.read_logs()
        assert [[g.player_id for g in per] for per in got] == [[0], [2]]
        for t, per in enumerate(got):
            names = ["b" if (int(aos[t]) >> s) & 1 else "a" for s in range(4)]
            ev = [dict(type="start_game", names=names, seed=list(seeds[t]))] + ML.decode_events(logs[t]) + [dict(type="end_game")]
            assert per[0].player_name == "b" and G.check_gameplay(oracle, per[0], ev, 3, True) > 0
        assert [len(per) for per in runner.gameplays(loader, seats=[0, 15])] == [0, 1]
        runner.close()
        plain = A.BatchRunner([TS._LowestLegalEngine("a"), TS._LowestLegalEngine("b")], seeds, aos, deal_algo=0)
        with pytest.raises(RuntimeError, match="device log is off"):
            plain.gameplays(loader)
        plain.close()
    finally:
        A.BatchRunner.pool_cls = old


# ---- allocation and synchronise failures in mj_replay_load_pool (as tests/test_emu_alloc_failures.py sweeps the other calls)
@pytest.mark.parametrize("deal_from_seed", [False, True])
def test_replay_load_pool_allocation_failures(emu, played, deal_from_seed):
    """For every allocation and every synchronise the call makes: the call fails, nothing is freed twice, the destination still
    replays the script it had (the golden game, loaded from the host) to the same bytes, and the call then succeeds and gives
    what it gives on a pool that never saw a failure."""
    from mortal_amd import mjai_log as ML

    src, _ = played
    L = emu._L
    n = 2
    script = ML.encode_events(G.golden_events())
    counts = np.zeros(3, dtype=np.int64)

    def fresh():
        p = emu(n, version=3)
        p.replay_load([script] * n, [0xF] * n)
        return p

    def call(p):
        return L.mj_replay_load_pool(p.h, src.h, 1, None, 1, int(deal_from_seed), counts.ctypes.data, None)

    gc.collect()
    base = _stats(L)["live"]
    p = fresh()
    want_old = _first_samples(p)
    before = _stats(L)
    assert call(p) == 0 and counts.tolist() == [n, 0, 0]
    made = {kind: _stats(L)[kind] - before[kind] for kind in ("alloc", "sync")}
    want_new = _first_samples(p)
    p.close()
    assert made["alloc"] >= 8 and made["sync"] >= 2 and want_new != want_old
    assert _stats(L)["live"] == base and _stats(L)["bad_frees"] == 0
    for kind, k in [(kind, k) for kind in made for k in range(1, made[kind] + 1)]:
        p = fresh()
        L.mj_emu_fail_nth(k if kind == "alloc" else 0, k if kind == "sync" else 0)
        rc = call(p)
        L.mj_emu_fail_nth(0, 0)
        assert rc == -1 and L.mj_last_error().decode(), (kind, k)
        assert _stats(L)["bad_frees"] == 0, (kind, k)
        assert _first_samples(p) == want_old, (kind, k)  # the script loaded before is still the one loaded, untouched
        assert call(p) == 0, (kind, k, L.mj_last_error().decode())
        assert _first_samples(p) == want_new, (kind, k)
        p.close()
        assert _stats(L)["live"] == base and _stats(L)["bad_frees"] == 0, (kind, k)
