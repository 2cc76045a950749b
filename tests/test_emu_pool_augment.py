"""Suit augmentation on the device (mj_k_log_pack<true> behind MJ_LOAD_AUGMENT and mj_augment_logs; GameplayLoader.load_pool /
load_harvest(..., augmented=True), mjai_log.augment_logs), run on the host emulation of the device code.  The cases and their
yardsticks live in tests/pool_augment_cases.py, shared with the `-m gpu` leg (tests/test_gpu_pool_augment.py)."""
import gc
import os
import shutil
import sys

import numpy as np
import pytest

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
if HOST not in sys.path:
    sys.path.insert(0, HOST)

from emu_alloc import stats as _stats  # noqa: E402
import pool_augment_cases as A  # noqa: E402
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


def test_directed_words_at_every_window_offset(emu, monkeypatch):
    A.check_directed(emu._L)
    monkeypatch.setenv("MJ_LOG_GRID", "2")  # two workgroups: every wavefront takes eight or nine logs, one after the other
    A.check_directed(emu._L)


def test_pool_route_equals_the_reference_loader_on_swapped_events(oracle, emu, played):
    pool, logs = played
    assert A.check_pool_route(oracle, emu, pool, logs, 3, 3) > 1000


@pytest.mark.parametrize("deal_algo", [0, 1])
def test_invisible_obs_swapped_events_wall_as_dealt(emu, deal_algo):
    assert A.check_invisible(emu, 2, 1, deal_algo) > 400


def test_harvest_route_and_a_record_in_error(oracle, emu):
    assert A.check_harvest_route(oracle, emu) > 500


def test_runners_pass_the_keyword_on(emu):
    A.check_runners(emu)


def test_refusals_leave_the_destination_usable(emu, played):
    A.check_refusals(emu, played[0])


# ---- allocation and synchronise failures (as tests/test_emu_pool_gameplay.py sweeps the plain load)
def _sweep(L, made):
    for kind in made:
        for k in range(1, made[kind] + 1):
            yield kind, k, (k if kind == "alloc" else 0, k if kind == "sync" else 0)


def test_augment_logs_allocation_failures(emu):
    """For every allocation and every synchronise mj_augment_logs makes: the call fails, nothing stays live, nothing is freed
    twice, and the call that follows gives the words of a call that never saw a failure."""
    L = emu._L
    logs, want = A.directed_logs()
    gc.collect()
    base = _stats(L)
    got, counts = A.raw_augment(L, logs)
    made = {kind: _stats(L)[kind] - base[kind] for kind in ("alloc", "sync")}
    assert made["alloc"] >= 6 and made["sync"] >= 1, made
    assert _stats(L)["live"] == base["live"]
    off = np.zeros(len(logs) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in logs])
    words = np.concatenate(logs)
    for kind, k, nth in _sweep(L, made):
        out = np.zeros(len(words), dtype=np.uint64)
        c3 = np.zeros(3, dtype=np.int64)
        L.mj_emu_fail_nth(*nth)
        rc = L.mj_augment_logs(words.ctypes.data, off.ctypes.data, len(logs), out.ctypes.data, c3.ctypes.data, None)
        L.mj_emu_fail_nth(0, 0)
        assert rc == -1 and L.mj_last_error().decode(), (kind, k)
        assert _stats(L)["live"] == base["live"] and _stats(L)["bad_frees"] == 0, (kind, k)
        again, counts2 = A.raw_augment(L, logs)
        assert counts2 == counts and all((a == b).all() for a, b in zip(again, want)), (kind, k)
        assert _stats(L)["live"] == base["live"] and _stats(L)["bad_frees"] == 0, (kind, k)


@pytest.mark.parametrize("deal_from_seed", [False, True])
def test_augmenting_load_allocation_failures(emu, played, deal_from_seed):
    """The same over mj_replay_load_pool with MJ_LOAD_AUGMENT: a failing call leaves the destination replaying the script it had, the
    retried call gives the bytes of a fresh pool, nothing stays live."""
    from mortal_amd import mjai_log as ML

    src, _ = played
    L = emu._L
    n = 2
    flags = 2 | int(deal_from_seed)
    script = ML.encode_events(G.golden_events())
    counts = np.zeros(3, dtype=np.int64)

    def fresh():
        p = emu(n, version=3)
        p.replay_load([script] * n, [0xF] * n)
        return p

    def call(p):
        return L.mj_replay_load_pool(p.h, src.h, 1, None, 1, flags, counts.ctypes.data, None)

    gc.collect()
    base = _stats(L)["live"]
    p = fresh()
    want_old = A.first_samples(p, 8)
    before = _stats(L)
    assert call(p) == 0 and counts.tolist() == [n, 0, 0]
    made = {kind: _stats(L)[kind] - before[kind] for kind in ("alloc", "sync")}
    want_new = A.first_samples(p, 8)
    p.close()
    assert made["alloc"] >= 8 and made["sync"] >= 2 and want_new != want_old and len(want_new) > 1000
    q = emu(n, version=3)  # the un-augmented load of the same tables gives other bytes
    assert L.mj_replay_load_pool(q.h, src.h, 1, None, 1, int(deal_from_seed), counts.ctypes.data, None) == 0
    assert A.first_samples(q, 8) != want_new
    q.close()
    assert _stats(L)["live"] == base and _stats(L)["bad_frees"] == 0
    for kind, k, nth in _sweep(L, made):
        p = fresh()
        L.mj_emu_fail_nth(*nth)
        rc = call(p)
        L.mj_emu_fail_nth(0, 0)
        assert rc == -1 and L.mj_last_error().decode(), (kind, k)
        assert _stats(L)["bad_frees"] == 0, (kind, k)
        assert A.first_samples(p, 8) == want_old, (kind, k)
        assert call(p) == 0, (kind, k, L.mj_last_error().decode())
        assert A.first_samples(p, 8) == want_new, (kind, k)
        p.close()
        assert _stats(L)["live"] == base and _stats(L)["bad_frees"] == 0, (kind, k)
