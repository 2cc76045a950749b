"""Allocation failures in the C-ABI host code (mortal_amd/csrc/mj_capi.hip), on the emulated runtime: its registry counts live
buffers, events and streams and the frees of something not live, and makes the k-th allocation from now on fail -- or the k-th
stream synchronise, which is where the real runtime reports a failure of the work queued before it and the one fallible step
between the allocation and the free of a call's temporaries (tests/host/emu/hip/hip_runtime.h, through mj_emu_alloc_stats /
mj_emu_fail_nth).  For every call that allocates, and for every allocation and every synchronise k it makes: the call reports the
failure, nothing is freed twice, the pool is as it was before the call (include/mortal_amd.h; mj_pool_enable_log leaves the log
disabled instead) -- the same call then succeeds and a short game gives the bytes it gives on a pool that never saw a failure --
and destroying the pool leaves nothing behind."""
import ctypes as C
import gc
import json
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "host")
if HOST not in sys.path:
    sys.path.insert(0, HOST)

from emu_alloc import stats  # noqa: E402

N = 4            # tables of every pool here
CYCLES = 6       # of the scenario: the deal and five rounds of decisions, every row through mj_k_sp (or the small-pool schedule)
REPLAY_STEPS = 8
LOG_WORDS = 512
SEEDS = [(9000 + t, 0x5EED) for t in range(N)]


@pytest.fixture(scope="module")
def emu():
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    import emu_pool

    return emu_pool.make_pool_class()


@pytest.fixture(autouse=True)
def small_sp_work_areas(monkeypatch):
    monkeypatch.setenv("MJ_SP_GRID", "1")
    monkeypatch.setenv("MJ_SP_WIDE", "0")


def arm(L, kind=None, k=0):
    L.mj_emu_fail_nth(k if kind == "alloc" else 0, k if kind == "sync" else 0)


def baseline(L):
    gc.collect()  # pools of other tests that still wait for the collector
    st = stats(L)
    assert st["bad_frees"] == 0
    return st["live"]


def last_error(L):
    return L.mj_last_error().decode()


def scripts():
    """Two replay scripts per table from the example game: the whole game, and the game from its second kyoku on."""
    from mortal_amd import mjai_log

    with open(os.path.join(HERE, "golden", "example_game.jsonl")) as f:
        events = [json.loads(line) for line in f if line.strip()]
    starts = [i for i, e in enumerate(events) if e["type"] == "start_kyoku"]
    return mjai_log.encode_events(events), mjai_log.encode_events(events[:1] + events[starts[1]:])


class Args:
    """The host arrays of the calls under test (kept alive here)."""

    def __init__(self):
        from mortal_amd import mjai_log

        self.nonces = np.array([s[0] for s in SEEDS], dtype=np.uint64)
        self.keys = np.array([s[1] for s in SEEDS], dtype=np.uint64)
        a, b = scripts()
        self.script = {}
        for name, words, tracked in (("a", a, 0xF), ("b", b, 0x5)):
            off = np.arange(N + 1, dtype=np.uint32) * np.uint32(len(words))
            self.script[name] = (np.ascontiguousarray(np.tile(words, N), dtype=np.uint64), off, np.full(N, tracked, dtype=np.uint8))
        self.event = mjai_log.encode_events([{"type": "end_kyoku"}])
        self.q_args = np.zeros(8, dtype=np.int32)
        self.q_out = np.zeros(8, dtype=np.int32)
        self.algo_q = np.zeros(2 * 72, dtype=np.uint8)
        self.algo_q[[62, 72 + 62]] = 5  # MjAlgoQuery.op 5 = Point::calc of arg1 fu, arg2 han
        self.algo_q[[64, 72 + 64]] = 30, 40
        self.algo_q[[65, 72 + 65]] = 2, 3
        self.algo_r = np.zeros(2 * 8, dtype=np.int32)
        self.seats = np.full(N, 0xF, dtype=np.uint8)
        self.groups = np.zeros(N, dtype=np.uint8)
        self.totals = np.zeros(2 * 44, dtype=np.int64)
        self.per_seat = np.zeros(N * 4 * 44, dtype=np.int64)
        self.counts = np.zeros(3, dtype=np.int64)


def ptr(a):
    return a.ctypes.data


def new_pool(emu):
    return emu(N, version=4, deal_algo=1)


def reset(pool):
    pool.reset(SEEDS)


def first_step(pool):
    reset(pool)
    assert pool.step()[0] > 0


def replay_load(pool, A, which):
    script, off, tracked = A.script[which]
    return pool._L.mj_replay_load(pool.h, ptr(script), ptr(off), ptr(tracked), N, 1, None, None)


def replay_samples(pool):
    """Rows, obs (v3: the SP kernel's row counter stays what the scenario expects), masks and meta of the first replay steps."""
    pool.configure(0, version=3)
    out = []
    for _ in range(REPLAY_STEPS):
        if pool.replay_step():
            obs, masks = pool.encode(0)
            out += [pool.rows(0).tobytes(), obs.numpy().tobytes(), masks.numpy().tobytes(), pool.replay_meta().numpy().tobytes()]
    pool.configure(0, version=4)
    assert len(out) >= 4
    return b"".join(out)


def counters(pool):
    cnt = (C.c_uint64 * 8)()
    assert pool._L.mj_counters(pool.h, cnt, None) == 0
    return np.array(cnt, dtype=np.uint64)


def scenario(pool):
    """A short game at obs v4 under the device's greedy policy -> every byte the caller sees of it.  Counter words 6 and 7 (SP
    overflows, SP rows) count since the pool was created, not since the reset: they are taken over the scenario alone, so that the
    rows of a successful first encode before it do not show."""
    reset(pool)
    before = counters(pool)
    acts = obs = masks = None
    for c in range(CYCLES):
        assert pool.step(acts)[0] > 0
        obs, masks = pool.encode(0)
        acts = pool.greedy_policy(0, masks, obs, 5, c)
    cnt = counters(pool)
    cnt[6:] -= before[6:]
    scores, done = pool.results()
    return b"".join([obs.numpy().tobytes(), masks.numpy().tobytes(), cnt.tobytes(), scores.tobytes(), done.tobytes()])


# name -> (environment, what brings a fresh pool to the call, the call -> its status)
def _cases():
    def c_reset(p, A):
        return p._L.mj_pool_reset(p.h, ptr(A.nonces), ptr(A.keys), None, None, N)

    def c_log(p, A):
        return p._L.mj_pool_enable_log(p.h, LOG_WORDS)

    def c_apply(p, A):
        return p._L.mj_table_apply_event(p.h, 1, ptr(A.event), len(A.event), None)

    def c_query(p, A):
        return p._L.mj_table_query(p.h, 1, 2, 3, ptr(A.q_args), ptr(A.q_out), None)

    def c_algo(p, A):
        return p._L.mj_algo_query(ptr(A.algo_q), 2, ptr(A.algo_r), None)

    def c_stat_logs(p, A):
        script, off, _ = A.script["a"]
        return p._L.mj_stat_logs(ptr(script), ptr(off), N, ptr(A.seats), ptr(A.groups), ptr(A.totals), ptr(A.per_seat), ptr(A.counts), None)

    def c_pool_stat(p, A):
        return p._L.mj_pool_stat(p.h, ptr(A.seats), ptr(A.totals), ptr(A.per_seat), ptr(A.counts), None)

    def c_encode(p, A):
        import torch

        n = p.n_rows[0]
        A.obs = torch.zeros((n, 1012, 34), dtype=torch.float32)
        A.masks = torch.zeros((n, 46), dtype=torch.bool)
        return p._L.mj_encode(p.h, 0, A.obs.data_ptr(), A.masks.data_ptr(), None)

    def log_then_reset(p, A):
        assert c_log(p, A) == 0
        reset(p)

    def load_a(p, A):
        assert replay_load(p, A, "a") == 0

    nothing = lambda p, A: None
    return {
        "mj_pool_reset": ({}, lambda p, A: reset(p), c_reset),  # (a reset pool: the result buffers of the first reset are replaced)
        "mj_pool_enable_log": ({}, nothing, c_log),
        "mj_pool_enable_log_again": ({}, lambda p, A: p.enable_log(64), c_log),
        "mj_replay_load": ({}, nothing, lambda p, A: replay_load(p, A, "a")),
        "mj_replay_load_again": ({}, load_a, lambda p, A: replay_load(p, A, "b")),
        "mj_encode_sp_setup": ({}, lambda p, A: first_step(p), c_encode),
        "mj_encode_sp_setup_wide": ({"MJ_SP_WIDE": "1"}, lambda p, A: first_step(p), c_encode),
        "mj_table_apply_event": ({}, lambda p, A: reset(p), c_apply),
        "mj_table_query": ({}, lambda p, A: reset(p), c_query),
        "mj_algo_query": ({}, nothing, c_algo),
        "mj_stat_logs": ({}, nothing, c_stat_logs),
        "mj_pool_stat": ({}, log_then_reset, c_pool_stat),
    }


CASES = _cases()


@pytest.fixture(scope="module")
def expected(emu):
    """What a pool that never saw a failure gives: the scenario per environment, and the replay samples of script a."""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MJ_SP_GRID", "1")
        for wide in ("1", "0"):
            mp.setenv("MJ_SP_WIDE", wide)
            pool = new_pool(emu)
            out[wide] = scenario(pool)
            pool.close()
        pool = new_pool(emu)
        assert replay_load(pool, Args(), "a") == 0
        out["replay"] = replay_samples(pool)
        pool.close()
    assert out["0"] == out["1"]  # (the small-pool schedule is bit-identical to mj_k_sp alone)
    return out


def check_left_behind(L, base):
    st = stats(L)
    assert st["live"] == base and st["bad_frees"] == 0, st


def test_pool_create_allocation_failures(emu, expected):
    L = emu._L
    base = baseline(L)
    before = stats(L)
    new_pool(emu).close()
    n = stats(L)["alloc"] - before["alloc"]
    assert n == 9 and stats(L)["sync"] == before["sync"]
    check_left_behind(L, base)
    for k in range(1, n + 1):
        arm(L, "alloc", k)
        h = L.mj_pool_create(N, 4, 1, 0)
        arm(L)
        assert not h and last_error(L), k
        check_left_behind(L, base)  # nothing of the half-built pool survives
        pool = new_pool(emu)
        assert scenario(pool) == expected["0"], k
        pool.close()
        check_left_behind(L, base)


@pytest.mark.parametrize("name", list(CASES))
def test_allocation_failures(emu, expected, monkeypatch, name):
    env, prepare, call = CASES[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    L = emu._L
    A = Args()
    base = baseline(L)
    # how many allocations and stream synchronises the call makes
    pool = new_pool(emu)
    prepare(pool, A)
    before = stats(L)
    assert call(pool, A) == 0, last_error(L)
    n = {kind: stats(L)[kind] - before[kind] for kind in ("alloc", "sync")}
    pool.close()
    check_left_behind(L, base)
    assert n["alloc"] >= 1
    for kind, k in [(kind, k) for kind in n for k in range(1, n[kind] + 1)]:
        pool = new_pool(emu)
        prepare(pool, A)
        arm(L, kind, k)
        rc = call(pool, A)
        arm(L)
        assert rc == -1 and last_error(L), (name, kind, k)
        assert stats(L)["bad_frees"] == 0, (name, kind, k)
        if name == "mj_replay_load":
            assert L.mj_replay_step(pool.h, None) == -1 and last_error(L) == "mj_replay_load first", k
        if name == "mj_replay_load_again":
            assert replay_samples(pool) == expected["replay"], k  # script a is still the one loaded, untouched
        if name.startswith("mj_pool_enable_log"):
            lens = np.zeros(N, dtype=np.uint32)
            assert L.mj_log_lengths(pool.h, ptr(lens), None) == -1 and last_error(L) == "event log is not enabled", k
            first_step(pool)
        assert call(pool, A) == 0, (name, kind, k, last_error(L))
        assert scenario(pool) == expected[env.get("MJ_SP_WIDE", "0")], (name, kind, k)
        assert stats(L)["bad_frees"] == 0, (name, kind, k)
        pool.close()
        check_left_behind(L, base)


def test_pool_with_every_optional_resource_is_released(emu, monkeypatch):
    """Destructor order of MjPool with the log, the SP work areas, the schedule's stream / events / pinned word, the step's events,
    the timing events and a loaded replay all present."""
    monkeypatch.setenv("MJ_SP_WIDE", "1")
    L = emu._L
    A = Args()
    base = baseline(L)
    pool = new_pool(emu)
    reset(pool)
    pool.enable_log(LOG_WORDS)
    pool.encode_timing(True)
    acts = None
    for c in range(10):
        assert pool.step(acts)[0] > 0
        obs, masks = pool.encode(0)
        acts = pool.greedy_policy(0, masks, obs, 5, c)
    assert pool.sp_schedule_stats()["hybrid_launches"] == 10
    live = stats(L)["live"]
    assert live[1] - base[1] >= 2 + 2 + 4 and live[2] - base[2] == 1  # step + schedule + timing events, the second stream
    assert replay_load(pool, A, "a") == 0
    pool.close()
    check_left_behind(L, base)
