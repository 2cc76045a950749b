"""libriichi's Stat reduced on the device (mortal_amd/csrc/mj_stat.hip: mj_k_log_stat behind mj_stat_logs / mj_pool_stat), run on
the host emulation of the device code.  Every case compares with the host reading `Stat.from_game(decode_events(words), seat)`
(mortal_amd/stat.py), per (log, seat) and in total, exactly; the cases shared with the `-m gpu` leg live in
tests/stat_device_cases.py."""
import os
import shutil
import sys

import numpy as np
import pytest

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
if HOST not in sys.path:
    sys.path.insert(0, HOST)

import stat_device_cases as S  # noqa: E402

KEY = 0xD5DFAA4CEF265CD7


@pytest.fixture(scope="module")
def emu():
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    import emu_pool

    return emu_pool.make_pool_class()


def test_counters_round_trip():
    from libriichi.stat import STAT_FIELDS, Stat

    assert len(STAT_FIELDS) == 44 and STAT_FIELDS[0] == "game" and STAT_FIELDS[-1] == "nagashi_mangan"
    st = Stat.from_counters(range(100, 144))
    assert st.counters() == list(range(100, 144)) and st.game == 100 and st.nagashi_mangan == 143
    assert Stat.from_counters((st + st).counters()) == st + st
    with pytest.raises(ValueError):
        Stat.from_counters([0] * 43)


def test_fixture_logs(oracle, emu):
    S.check_fixture_logs(oracle, emu._L)


def test_seat_masks_and_groups(oracle, emu):
    S.check_masks_and_groups(oracle, emu._L)


def test_alignment_sweep(emu):
    S.check_alignment_sweep(emu._L)


def test_alignment_sweep_grp(emu):
    S.check_alignment_sweep_grp(emu._L)


def test_bad_and_empty_input(emu):
    S.check_bad_and_empty_input(emu._L)


def test_pool_log_stat(emu):
    S.check_pool(emu, 8)


def test_pool_log_stat_needs_the_log_and_no_refill(emu):
    import parity_util

    pool = emu(2, version=3)
    pool.reset(parity_util.default_seeds(2), game_ids=np.arange(2), n_games_total=2)
    with pytest.raises(RuntimeError, match="log is not enabled"):  # (MortalAmdError)
        pool.log_stat()
    pool.enable_log()
    assert pool.log_stat()[2] == dict(reduced=0, skipped=2, malformed=0)
    pool.set_refill(2)
    with pytest.raises(RuntimeError, match="refill"):
        pool.log_stat()
    pool.close()


def test_one_vs_three_collect_stat(emu, tmp_path):
    """OneVsThree(collect_stat=True, log_dir=...) with the recorded reference engines of tests/test_one_vs_three_script.py: env.stats
    is what Stat.from_dir reads back from the dumped logs, for both names, and the return value is the recorded one -- the rankings
    that test pins for the same run without collect_stat.  (One run: the recorded engines need obs v4, minutes on the emulator;
    collect_stat without a log_dir runs in the two tests below.)"""
    import recorded_engine as R
    from libriichi.arena import OneVsThree
    from libriichi.stat import Stat

    from mortal_amd import arena as A

    chal, cham = (R.RecordedEngine(R.decisions("cfg0", who), 4, who) for who in R.ENGINES)
    old = A.BatchRunner.pool_cls
    A.BatchRunner.pool_cls = emu
    try:
        d = str(tmp_path / "logs")
        env = OneVsThree(disable_progress_bar=True, log_dir=d, collect_stat=True)
        assert env.stats is None
        got = env.py_vs_py(challenger=chal, champion=cham, seed_start=(10000, 0x55DFAA4CEF265CD7), seed_count=2)
    finally:
        A.BatchRunner.pool_cls = old
    assert got == R.fixture()["one_vs_three"]["cfg0"]["rankings"]
    assert sorted(env.stats) == sorted(R.ENGINES) and len(os.listdir(d)) == 8
    for name in R.ENGINES:
        assert env.stats[name] == Stat.from_dir(d, name, True), name
    st = env.stats["challenger"]
    assert st.game == 8 and [st.rank_1, st.rank_2, st.rank_3, st.rank_4] == got


def test_two_vs_two_collect_stat(emu, tmp_path):
    """TwoVsTwo, and two engines of one name: their seats are summed, as Stat.from_dir does with equal names."""
    import test_sharding as TS
    from libriichi.arena import TwoVsTwo
    from libriichi.stat import Stat

    from mortal_amd import arena as A

    old = A.BatchRunner.pool_cls
    A.BatchRunner.pool_cls = emu
    try:
        d = str(tmp_path / "logs")
        env = TwoVsTwo(disable_progress_bar=True, log_dir=d, deal_algo=0, collect_stat=True)
        assert env.py_vs_py(TS._LowestLegalEngine("a"), TS._LowestLegalEngine("b"), (10000, KEY), 1) is None
        same = TwoVsTwo(disable_progress_bar=True, deal_algo=0, collect_stat=True)
        same.py_vs_py(TS._LowestLegalEngine("x"), TS._LowestLegalEngine("x"), (10000, KEY), 1)
    finally:
        A.BatchRunner.pool_cls = old
    assert sorted(env.stats) == ["a", "b"] and env.stats["a"].game == env.stats["b"].game == 4
    for name in "ab":
        assert env.stats[name] == Stat.from_dir(d, name, True)
    assert list(same.stats) == ["x"] and same.stats["x"] == env.stats["a"] + env.stats["b"]


# ---- torch.distributed: the counters are summed over the ranks
def _worker(rank, world, port, q):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests"), os.path.join(root, "tests", "host")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    import emu_pool
    import test_sharding as TS
    from libriichi.arena import OneVsThree

    from mortal_amd import arena as A
    from mortal_amd import sharding

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    summed = sharding.allreduce_counters([rank + 1, -(1 << 40) * (rank + 1), 0, (1 << 62) - rank])
    A.BatchRunner.pool_cls = emu_pool.make_pool_class()
    env = OneVsThree(disable_progress_bar=True, deal_algo=0, collect_stat=True)
    got = env.py_vs_py(TS._LowestLegalEngine("a"), TS._LowestLegalEngine("b"), (10000, KEY), 2)
    q.put((rank, summed, got, {k: v.counters() for k, v in env.stats.items()}))
    dist.destroy_process_group()


def test_collect_stat_over_two_gloo_ranks(emu):
    import torch.multiprocessing as mp

    import test_sharding as TS
    from libriichi.arena import OneVsThree

    from mortal_amd import arena as A

    world, port = 2, 29543
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {r: rest for r, *rest in (q.get(timeout=600) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    old = A.BatchRunner.pool_cls
    A.BatchRunner.pool_cls = emu
    try:
        env = OneVsThree(disable_progress_bar=True, deal_algo=0, collect_stat=True)
        want = env.py_vs_py(TS._LowestLegalEngine("a"), TS._LowestLegalEngine("b"), (10000, KEY), 2)
    finally:
        A.BatchRunner.pool_cls = old
    stats = {k: v.counters() for k, v in env.stats.items()}
    assert stats["a"][0] == 8 and stats["b"][0] == 24
    for r in range(world):
        summed, hist, st = got[r]
        assert summed == [3, -3 * (1 << 40), 0, (1 << 63) - 1]
        assert hist == want and st == stats, r
