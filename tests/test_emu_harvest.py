"""Finished games collected from a pool in refill mode (mortal_amd/csrc/mj_harvest.hip behind mj_pool_enable_harvest /
mj_harvest_take / mj_harvest_stat / mj_harvest_grp / mj_replay_load_harvest; TablePool.take_harvest, Harvest,
GameplayLoader.load_harvest, arena.SelfPlayRunner), run on the host emulation of the device code.  The cases and their yardsticks
live in tests/harvest_cases.py, shared with the `-m gpu` leg (tests/test_gpu_harvest.py)."""
import ctypes as C
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
import harvest_cases as H  # noqa: E402
import pool_gameplay_cases as G  # noqa: E402

N = 3


@pytest.fixture(scope="module")
def emu():
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    import emu_pool

    return emu_pool.make_pool_class()


@pytest.fixture(scope="module")
def played(emu):
    """Three tables, two generations each, one take at the end: shared and left unchanged."""
    run, h, want = H.two_generations(emu, N)
    yield run, h, want
    h.close()
    run.close()


def test_two_generations_records_stat_grp(emu, played):
    H.check_two_generations(*played, emu._L)


def test_two_generations_samples_equal_the_reference_loader(oracle, played):
    run, h, _ = played
    assert H.check_samples(oracle, run, h, 2, [15, 6]) > 500  # games 2 and 3: the last of generation 0, the first of generation 1


def test_many_games_ending_in_one_step(emu):
    H.check_many_in_one_step(emu, 3, {0, 1, 2}, emu._L)


def test_odd_log_stride_takes_the_8_byte_copy(emu):
    """A log of an odd number of words per table: the tables' logs are not all 16-byte aligned, the kernel copies word by word."""
    H.check_many_in_one_step(emu, 3, {0, 2}, emu._L, log_cap=H.LOG_CAP - 1)


def test_taking_while_playing(emu):
    H.check_take_while_playing(emu, N)


def test_full_buffer_drops_and_counts(emu):
    H.check_full_buffer(emu, N)


def test_a_table_in_error(oracle, emu):
    H.check_table_in_error(oracle, emu, N, 1, emu._L)


def test_staggered_start(emu):
    H.check_staggered_start(emu, N, 40, emu._L)


def test_invisible_obs_from_the_recorded_seed(oracle, played):
    run, h, _ = played
    assert H.check_invisible(oracle, run, h, N, 2) > 400


def test_refusals(emu, played):
    run, h, _ = played
    H.check_refusals(emu, run, h)


def test_self_play_runner(oracle, emu):
    H.check_self_play_runner(oracle, emu, 2)


def test_self_play_runner_refuses_mjai_log_engines(emu):
    from mortal_amd import arena as A

    class Ev:
        engine_type = "mjai-log"
        name = "ev"

        def react_batch(self, *a):
            return []

        start_game = end_kyoku = end_game = react_batch

    old = A.SelfPlayRunner.pool_cls
    A.SelfPlayRunner.pool_cls = emu
    try:
        with pytest.raises(ValueError, match="mjai events"):
            A.SelfPlayRunner([Ev()], 2, (10000, H.KEY), max_games=8, max_words=1 << 15)
    finally:
        A.SelfPlayRunner.pool_cls = old
    import libriichi.arena

    assert libriichi.arena.SelfPlayRunner is A.SelfPlayRunner


# ---- allocation and synchronise failures of mj_harvest_take and mj_replay_load_harvest (as test_replay_load_pool_allocation_failures)
@pytest.mark.parametrize("deal_from_seed", [False, True])
def test_replay_load_harvest_allocation_failures(emu, played, deal_from_seed):
    """For every allocation and every synchronise the call makes: the call fails, nothing is freed twice, the destination still
    replays the script it had (the golden game, loaded from the host), the harvest is untouched, and the retried call gives the
    bytes of a run that never failed."""
    from mortal_amd import mjai_log as ML

    _, h, _ = played
    L = emu._L
    n = 2
    script = ML.encode_events(G.golden_events())
    counts = np.zeros(3, dtype=np.int64)
    want_h = H.harvest_bytes(h, first_samples=False)

    def fresh():
        p = emu(n, version=3)
        p.replay_load([script] * n, [0xF] * n)
        return p

    def call(p):
        return L.mj_replay_load_harvest(p.h, h.h, 2, None, 1, int(deal_from_seed), counts.ctypes.data, None)

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
    assert H.harvest_bytes(h, first_samples=False) == want_h


def test_harvest_take_allocation_failures(emu):
    """The same sweep over mj_harvest_take.  Every failing take leaves the pool's active buffer as it was (pending unchanged, no
    allocation left over, nothing freed twice); the take that follows the whole sweep returns all games, byte for byte what the
    take of a run that never saw a failure returns, and every live allocation is back at the baseline after close().  (One
    sweep over one filled buffer: a successful take in between would empty it, and refilling it costs a hanchan.)"""
    L = emu._L
    gc.collect()
    base = _stats(L)["live"]

    def filled():
        run = H.Run(emu, 3, seeds=[(G.SEED_START, H.KEY)] * 3, policy="lowest")  # three equal games: they end, and are collected, together
        try:
            want = run.play_until(run.every_table(1), 8000)
            assert len(want) == 3 and run.pool.harvest_pending()["games"] == 3
        except BaseException:
            run.close()
            raise
        return run, want

    def everything(run, want):
        h = run.pool.take_harvest()
        try:
            H.check_records(run, h, want)
            return H.harvest_bytes(h, first_samples=False)
        finally:
            h.close()

    run, want = filled()
    try:
        before = _stats(L)
        never_failed = everything(run, want)
        # (the take itself, without what reading the harvest back allocates: counted on a second, empty take)
        before = _stats(L)
        h = run.pool.take_harvest()
        made = {kind: _stats(L)[kind] - before[kind] for kind in ("alloc", "sync")}
        assert h.n_games == 0
        h.close()
        assert made["alloc"] >= 8 and made["sync"] >= 3, made
    finally:
        run.close()
    gc.collect()
    assert _stats(L)["live"] == base
    run, want = filled()
    try:
        live_pool = _stats(L)["live"]
        pending = run.pool.harvest_pending()
        for kind, k in [(kind, k) for kind in made for k in range(1, made[kind] + 1)]:
            hp = C.c_void_p()
            L.mj_emu_fail_nth(k if kind == "alloc" else 0, k if kind == "sync" else 0)
            rc = L.mj_harvest_take(run.pool.h, C.byref(hp), None)
            L.mj_emu_fail_nth(0, 0)
            assert rc == -1 and not hp.value and L.mj_last_error().decode(), (kind, k)
            assert _stats(L)["bad_frees"] == 0 and _stats(L)["live"] == live_pool, (kind, k)
            assert run.pool.harvest_pending() == pending, (kind, k)
        assert everything(run, want) == never_failed
        assert run.pool.harvest_pending()["games"] == 0 and _stats(L)["live"] == live_pool
    finally:
        run.close()
    gc.collect()
    assert _stats(L)["live"] == base and _stats(L)["bad_frees"] == 0
