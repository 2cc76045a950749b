"""Shared by tests/test_gpu_pool_gameplay.py (the real library, `-m gpu`) and tests/test_emu_pool_gameplay.py (host emulation of
the device code): training samples and Grp straight from a pool's device log (GameplayLoader.load_pool, TablePool.log_grp,
mj_replay_load_pool / mj_pool_grp / mj_grp_logs).

The yardsticks are never the code under test: samples are compared with the reference loader restated on the oracle
(tests/dataset_ref.py) over `decode_events(pool.read_logs()[t])`, Grp with the host `Grp.load_events` over the same events and
with the reference-derived numbers of the golden example game (the values tests/test_dataset.py::test_grp_example_game asserts)."""
import json
import os

import numpy as np

import dataset_ref
import stat_device_cases as S

from mortal_amd import mjai_log as ML
from mortal_amd.dataset import GameplayLoader, Grp, grp_logs

KEY = 0xD5DFAA4CEF265CD7
# Table t of every pool here plays seed (SEED_START + t, KEY) under the greedy test policy (policy seed POLICY_SEED, keyed by table
# index and cycle).  The start was picked by playing the 70 tables of the GPU case on the CPU with the same policy and seeds and
# counting on the reference side (census() below) what tables 60..69 hold under the GPU case's seat masks:
#   start 31000: 15 kan labels with their select row, 2 games that end with riichi sticks on the table, 10 games with a honba > 0
#   (10000 and 52000 were tried first: 14 / 0 / 10 and 25 / 0 / 10 -- no game with sticks left, so they were not taken).
SEED_START = 31000
POLICY_SEED = 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example_game.jsonl")
NAMES = ["a", "b", "a", "c"]


def seeds(n):
    return [(SEED_START + t, KEY) for t in range(n)]


def play(pool_cls, n, version=3, deal_algo=0, at_cycle=None, poison=None, max_cycles=8000):
    """n tables, log on, every seat on the device's greedy policy, played to the end -> the pool (the caller closes it).
    at_cycle = (cycle, callback(pool)): called once in mid-run.  poison = (table, cycle): from that cycle on, the first answer
    of that table becomes action id 46, which no mask allows (tests/table_error_cases.py kind id_46)."""
    pool = pool_cls(n, version=version, deal_algo=deal_algo)
    try:
        pool.enable_log()
        pool.reset(seeds(n), game_ids=np.arange(n), n_games_total=n)
        acts = None
        poisoned = False
        for c in range(max_cycles):
            n_rows = pool.step(acts)
            if at_cycle is not None and c == at_cycle[0]:
                at_cycle[1](pool)
            if n_rows[0] == 0 and pool.counters()["games"] >= n:
                break
            acts = None
            if n_rows[0]:
                obs, masks = pool.encode(0)
                acts = pool.greedy_policy(0, masks, obs, POLICY_SEED, c)
                if poison is not None and not poisoned and c >= poison[1]:
                    hit = np.flatnonzero(pool.rows(0)[:, 0] == poison[0])
                    if len(hit):
                        acts[int(hit[0])] = 46
                        poisoned = True
        else:
            raise AssertionError("the pool did not finish")
        assert poison is None or poisoned
        return pool
    except BaseException:
        pool.close()
        raise


def ref_events(pool, logs, t, names=NAMES):
    """The game of table t as the reference's loader reads a log file: start_game with names and seed, the events, end_game."""
    nonce, key = seeds(pool.n_tables)[t]
    return [dict(type="start_game", names=list(names), seed=[nonce, key])] + ML.decode_events(logs[t]) + [dict(type="end_game")]


def census(oracle, events_list, seat_masks, always_kan):
    """Counted on the reference side over the compared games: kan labels followed by their select row (tracked seats), games whose
    raw final sum is below 100,000 (riichi sticks left on the table), games with a honba > 0 kyoku."""
    kan = sticks = honba = 0
    for ev, m in zip(events_list, seat_masks):
        for p in range(4):
            if (int(m) >> p) & 1:
                kan += sum(1 for _, k in dataset_ref.entry_event_indices(oracle, ev, p, always_kan) if k == 2)  # label 42 + select row
        g = Grp.load_events(ev)
        honba += bool((g.feature[:, 1] > 0).any())
        last = [e for e in ev if e["type"] == "start_kyoku"][-1]
        tail = ev[max(i for i, e in enumerate(ev) if e is last):]
        raw = sum(last["scores"]) + sum(sum(e["deltas"]) for e in tail if e["type"] in ("hora", "ryukyoku")) \
            - 1000 * sum(1 for e in tail if e["type"] == "reach_accepted")
        sticks += raw < 100_000
    return dict(kan_select=kan, sticks_left=sticks, honba=honba)


def same_grp(got, want):
    assert got.feature.dtype == np.float64 and got.feature.shape == want.feature.shape
    assert (got.feature.view(np.uint64) == want.feature.view(np.uint64)).all(), (got.feature, want.feature)
    assert got.rank_by_player == want.rank_by_player and got.final_scores == want.final_scores


def check_gameplay(oracle, gp, events, version, always_kan):
    """One Gameplay against the reference loader; -> its number of samples."""
    ref = dataset_ref.load_events_by_player(oracle, events, gp.player_id, version, always_kan)
    assert gp.player_name == ref["player_name"]
    assert gp.actions == ref["actions"], (gp.player_id, gp.actions[:20], ref["actions"][:20])
    assert gp.at_kyoku == ref["at_kyoku"] and gp.dones == ref["dones"] and gp.apply_gamma == ref["apply_gamma"]
    assert gp.at_turns == ref["at_turns"] and gp.shantens == ref["shantens"]
    same_grp(gp.grp, Grp.load_events(events))
    obs, masks = gp.take_obs(), gp.take_masks()
    assert len(obs) == len(ref["obs"]) == len(masks) == len(ref["actions"])
    for k in range(len(obs)):
        assert (masks[k] == ref["masks"][k]).all(), (gp.player_id, k)
        assert (obs[k].view(np.uint32) == ref["obs"][k].view(np.uint32)).all(), (gp.player_id, k, ref["actions"][k])
    return len(obs)


def check_range(oracle, pool, logs, version, table0, seat_masks, always_kan, want_census=False):
    """Case 1: load_pool over tables [table0, table0 + len(seat_masks)) against the reference loader, Gameplay by Gameplay."""
    n = len(seat_masks)
    names = [NAMES] * n
    loader = GameplayLoader(version, oracle=False, always_include_kan_select=always_kan)
    got = loader.load_pool(pool, table0=table0, n_tables=n, seats=seat_masks, names=names)
    assert len(got) == n
    events = [ref_events(pool, logs, table0 + i) for i in range(n)]
    if want_census:
        cs = census(oracle, events, seat_masks, always_kan)
        print("census", cs)
        assert cs["kan_select"] >= 1 and cs["sticks_left"] >= 1 and cs["honba"] >= 1, cs
    n_samples = 0
    for i in range(n):
        assert [g.player_id for g in got[i]] == [p for p in range(4) if (int(seat_masks[i]) >> p) & 1], i
        for g in got[i]:
            n_samples += check_gameplay(oracle, g, events[i], version, always_kan)
    # the pool's Grp on its own, every table of the range
    for i, g in enumerate(pool.log_grp(table0, n)):
        same_grp(g, Grp.load_events(events[i]))
    return n_samples


def check_invisible(oracle, pool_cls, n=5, version=1):
    """Case 2: oracle=True deals every wall from the table's seed, which travels from pool to pool on the device."""
    pool = play(pool_cls, n, version=version, deal_algo=0)  # (dataset_ref.invisibles_from_seed deals with the same shuffle, 0)
    try:
        logs = pool.read_logs()
        got = GameplayLoader(version, oracle=True, deal_algo=0).load_pool(pool)
        assert len(got) == n
        total = 0
        for t in range(n):
            ev = ref_events(pool, logs, t, ["", "", "", ""])
            assert [g.player_id for g in got[t]] == [0, 1, 2, 3]
            for g in got[t]:
                ref = dataset_ref.load_invisible_by_player(oracle, ev, g.player_id, version)
                inv = g.take_invisible_obs()
                assert len(inv) == len(ref) == len(g.actions) > 0
                for k in range(len(ref)):
                    assert (inv[k].view(np.uint32) == ref[k].view(np.uint32)).all(), (t, g.player_id, k)
                total += len(ref)
        return total
    finally:
        pool.close()


def samples_bytes(games):
    """Every byte of a load_pool / load_logs result."""
    out = []
    for per_table in games:
        for g in per_table:
            out += [bytes([g.player_id]), g.obs_dev.cpu().numpy().tobytes(), g.masks_dev.cpu().numpy().tobytes(),
                    np.array(g.actions + g.at_kyoku + g.at_turns + g.shantens, dtype=np.int64).tobytes(),
                    g.grp.feature.tobytes(), bytes(g.grp.rank_by_player)]
        out.append(b"|")
    return b"".join(out)


def check_skipped_and_error(oracle, pool_cls, n=4, victim=1, version=3):
    """Case 3, first two items: a pool probed in mid-run (every table skipped), and a pool with one table in error (skipped, its
    neighbours' samples what they are without it: compared with the reference loader, which never saw the pool)."""
    mid = {}

    def probe(pool):
        loader = GameplayLoader(version, oracle=False)
        mid["games"] = loader.load_pool(pool)
        mid["grp"] = pool.log_grp()
        rp = pool_cls(pool.n_tables, version=version)
        try:
            mid["counts"] = rp.replay_load_pool(pool)
            mid["rows"] = [rp.replay_step() for _ in range(3)]
            mid["done"] = rp.counters()["games"]
        finally:
            rp.close()

    pool = play(pool_cls, n, version=version, at_cycle=(40, probe), poison=(victim, 60))
    try:
        assert mid["counts"] == dict(loaded=0, skipped=n, malformed=0), mid["counts"]
        assert mid["games"] == [[] for _ in range(n)] and mid["grp"] == [None] * n
        assert mid["rows"] == [0, 0, 0] and mid["done"] == n  # empty scripts: no rows, every log finished at once
        code, tbl = pool.first_error()
        assert (code, tbl) == (1, victim)  # MJ_ERR_ILLEGAL_ACTION
        logs = pool.read_logs()
        loader = GameplayLoader(version, oracle=False)
        got = loader.load_pool(pool, names=[NAMES] * n)
        assert got[victim] == [] and pool.log_grp()[victim] is None
        rp = pool_cls(n, version=version)
        try:
            assert rp.replay_load_pool(pool) == dict(loaded=n - 1, skipped=1, malformed=0)
        finally:
            rp.close()
        for t in range(n):
            if t != victim:
                ev = ref_events(pool, logs, t)
                assert len(got[t]) == 4
                for g in got[t]:
                    assert check_gameplay(oracle, g, ev, version, True) > 0
    finally:
        pool.close()


def check_refusals(pool_cls, pool, version=3):
    """Case 3, last item: every refused call names its reason and leaves the destination usable -- a valid load that follows gives
    the bytes it gives on a fresh pool."""
    import pytest

    n = pool.n_tables
    loader = GameplayLoader(version, oracle=False)
    want = samples_bytes(loader.load_pool(pool, table0=0, n_tables=2))
    assert len(want) > 1000
    with pytest.raises(ValueError, match="augmented"):
        GameplayLoader(version, oracle=False, augmented=True).load_pool(pool)
    with pytest.raises(ValueError, match="are not in a pool"):
        loader.load_pool(pool, table0=n - 1, n_tables=2)
    plain = pool_cls(2, version=version)   # a source without a log
    plain.reset(seeds(2))
    refill = pool_cls(2, version=version)  # a source in refill mode
    refill.enable_log()
    refill.reset(seeds(2))
    refill.set_refill(8)
    dst = pool_cls(2, version=version)

    def replay(p):
        """The first samples of whatever dst has loaded."""
        out = []
        for _ in range(12):
            if p.replay_step():
                obs, masks = p.encode(0)
                out += [p.rows(0).tobytes(), obs.cpu().numpy().tobytes(), masks.cpu().numpy().tobytes(),
                        p.replay_meta().cpu().numpy().tobytes()]
        return b"".join(out)

    try:
        assert dst.replay_load_pool(pool) == dict(loaded=2, skipped=0, malformed=0)
        fresh = replay(dst)
        assert len(fresh) > 1000
        dst.replay_load_pool(pool)
        for _ in range(5):
            dst.replay_step()  # a replay under way when the refused calls arrive
        for src, kw, reason in ((plain, {}, "log of the source pool is not enabled"), (refill, {}, "refill mode"),
                                (dst, {}, "its own destination"), (pool, dict(table0=n - 1), "out of bounds"),
                                (pool, dict(table0=-1), "out of bounds")):
            with pytest.raises(RuntimeError, match=reason):
                dst.replay_load_pool(src, **kw)
        for src in (plain, refill):
            with pytest.raises(RuntimeError, match="log is not enabled|refill mode"):
                src.log_grp()
        with pytest.raises(RuntimeError, match="out of bounds"):
            pool.log_grp(n - 1, 2)
        assert dst.replay_load_pool(pool) == dict(loaded=2, skipped=0, malformed=0)
        assert replay(dst) == fresh
    finally:
        for p in (plain, refill, dst):
            p.close()
    assert samples_bytes(loader.load_pool(pool, table0=0, n_tables=2)) == want


# ---- case 4: the Grp kernel on explicit logs
def golden_events():
    with open(GOLDEN) as f:
        return [json.loads(line) for line in f if line.strip()]


def check_golden_grp(g):
    """The reference-derived numbers of the example game (tests/test_dataset.py::test_grp_example_game)."""
    f = g.feature
    assert f.dtype == np.float64 and f.shape == (3, 7)
    assert f[:, 0].tolist() == [0.0, 0.0, 1.0] and f[:, 1].tolist() == [0.0, 1.0, 0.0] and f[:, 2].tolist() == [0.0, 0.0, 0.0]
    assert f[0, 3:].tolist() == [2.5, 2.5, 2.5, 2.5]
    assert f[1, 3:].tolist() == [3.27, 2.5, 1.73, 2.5]
    assert f[2, 3:].tolist() == [3.27, 3.02, 1.31, 2.4]
    assert g.final_scores == [32700, 49200, -5900, 24000]
    assert g.rank_by_player == [1, 0, 3, 2]


def check_grp_golden(lib):
    import pytest

    words = ML.encode_events(golden_events())
    (g,) = Grp.from_packed([words], lib=lib)
    check_golden_grp(g)
    check_golden_grp(Grp.load_events(golden_events()))  # (the host yardstick itself)
    grps, n_kyoku, counts = grp_logs([words], max_kyoku=3, lib=lib)
    check_golden_grp(grps[0])
    assert n_kyoku.tolist() == [3] and counts == dict(reduced=1, skipped=0, malformed=0)
    # more kyoku than max_kyoku: malformed, zeros
    raw = raw_grp(lib, [words], 2)
    assert raw["counts"].tolist() == [0, 0, 1] and raw["n_kyoku"].tolist() == [-1]
    assert not raw["feat"].any() and not raw["rank"].any() and not raw["final"].any()
    with pytest.raises(ValueError, match="log 0"):
        Grp.from_packed([words], max_kyoku=2, lib=lib)


def raw_grp(lib, words_list, max_kyoku):
    """mj_grp_logs itself, outputs pre-filled with a pattern: every row must be written."""
    n = len(words_list)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in words_list])
    words = np.ascontiguousarray(np.concatenate(words_list) if n else np.zeros(0), dtype=np.uint64)
    out = dict(feat=np.full((n, max_kyoku, 7), 0x55AA, dtype=np.int32), n_kyoku=np.full(n, 77, dtype=np.int32),
               rank=np.full((n, 4), 9, dtype=np.int32), final=np.full((n, 4), 123, dtype=np.int32), counts=np.full(3, 5, dtype=np.int64))
    rc = lib.mj_grp_logs(words.ctypes.data, off.ctypes.data, n, max_kyoku, out["feat"].ctypes.data, out["n_kyoku"].ctypes.data,
                         out["rank"].ctypes.data, out["final"].ctypes.data, out["counts"].ctypes.data, None)
    assert rc == 0, lib.mj_last_error().decode()
    return out


def starts_of(words):
    """Word index of every start_kyoku header, found by walking the chain (a payload word can look like a header)."""
    out, i = [], 0
    while i < len(words):
        w = int(words[i])
        t = w & 15
        if t == ML.LG_START_KYOKU:
            out.append(i)
            i += 27 if (w >> 63) & 1 else 10
        else:
            i += (4 if t == ML.LG_HORA else 3 if t == ML.LG_RYUKYOKU else 1) + (0 if t == ML.LG_START_KYOKU else (w >> 43) & 1)
    return out


def host_grp_of_prefix(words):
    """What a cut log must give: the host reading if its chain ends at its end and it has a start_kyoku, else None (malformed)."""
    try:
        ev = ML.decode_events(words)
    except (IndexError, ValueError):
        return None
    # decode_events reads payload words by index: a cut inside the last payload raises IndexError above; a cut inside a
    # start_kyoku's tile words shows as a short tehais list
    for e in ev:
        if e["type"] == "start_kyoku" and any(len(h) != 13 for h in e["tehais"]):
            return None
    if not any(e["type"] == "start_kyoku" for e in ev):
        return None
    return Grp.load_events(ev)


def check_grp_truncated(lib):
    words = ML.encode_events(golden_events())
    st = starts_of(words)
    assert len(st) == 3
    cut = words[:st[1] + 4]  # inside the second start_kyoku's payload
    empty = np.zeros(0, dtype=np.uint64)
    raw = raw_grp(lib, [words, cut, empty, words], 8)
    assert raw["counts"].tolist() == [2, 1, 1] and raw["n_kyoku"].tolist() == [3, -1, 0, 3]
    for i in (1, 2):
        assert not raw["feat"][i].any() and not raw["rank"][i].any() and not raw["final"][i].any()
    assert (raw["feat"][0] == raw["feat"][3]).all() and raw["feat"][0, :3].any() and not raw["feat"][0, 3:].any()
    assert raw["final"][0].tolist() == raw["final"][3].tolist() == [32700, 49200, -5900, 24000]
    grps, n_kyoku, counts = grp_logs([words, cut, empty, words], lib=lib)
    assert grps[1] is None and grps[2] is None and counts == dict(reduced=2, skipped=1, malformed=1)
    check_golden_grp(grps[0])
    check_golden_grp(grps[3])


def check_grp_batch(lib, n=130):
    """130 copies of the example game cut at different points: every log's outputs are what the host gives for that prefix alone,
    whatever its neighbours are."""
    words = ML.encode_events(golden_events())
    cuts = [len(words) - (i * 37) % (len(words) - 5) for i in range(n)]
    logs = [words[:c] for c in cuts]
    want = [host_grp_of_prefix(w) for w in logs]
    n_good = sum(1 for g in want if g is not None)
    assert 10 <= n_good <= n - 10  # both kinds, interleaved
    grps, n_kyoku, counts = grp_logs(logs, max_kyoku=8, lib=lib)
    assert counts == dict(reduced=n_good, skipped=0, malformed=n - n_good), counts
    for i in range(n):
        if want[i] is None:
            assert grps[i] is None and n_kyoku[i] == -1, (i, cuts[i])
        else:
            same_grp(grps[i], want[i])
    raw = raw_grp(lib, logs, 8)
    for i in range(n):
        if want[i] is None:
            assert not raw["feat"][i].any() and not raw["rank"][i].any() and not raw["final"][i].any(), i


def check_grp_tagged(lib):
    """A tag word behind every reaction header (as the arena writes them) changes nothing."""
    for k, lead in ((0, 0), (29, 1), (58, 0)):
        plain, tagged = S.synthetic_words(k, lead, False), S.synthetic_words(k, lead, True)
        assert len(tagged) > len(plain)
        gp, gt = Grp.from_packed([plain, tagged], lib=lib)
        same_grp(gt, gp)
        same_grp(gp, Grp.load_events(S.synthetic_events(k, lead)))
        assert gp.feature.shape == (2, 7) and sum(gp.final_scores) == 100_000
