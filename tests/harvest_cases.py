"""Shared by tests/test_gpu_harvest.py (the real library, `-m gpu`) and tests/test_emu_harvest.py (host emulation of the device
code): finished games collected from a pool in refill mode (mortal_amd/csrc/mj_harvest.hip behind mj_pool_enable_harvest /
mj_harvest_take; TablePool.take_harvest, Harvest, GameplayLoader.load_harvest).

The yardsticks are never the code under test:
  words    the host's own reading of the table's log (TablePool.read_logs), taken between the step that finished the game and the
           step that rewound it: the logs are read after every step on which counters()["games"] rose, and the finished tables are
           those whose flags (mj_debug_table) carry TF_DONE | TF_ENDED;
  seeds    (seed of the table + g * stride, key) and id t + g * n_tables for generation g, counted by the test itself;
  scores   mj_results for generation 0 (it covers no later one), Grp.final_scores of the snapshot's events for every generation;
  Stat     stat.stat_logs over the snapshot words and the second reading of tests/stat_device_cases.py (Stat.from_game);
  Grp      Grp.load_events(decode_events(words));
  samples  the reference loader restated on the oracle (tests/dataset_ref.py) through pool_gameplay_cases.check_gameplay, on events
           built from the snapshot words and the seed the test counted."""
import numpy as np
import torch

import dataset_ref
import pool_gameplay_cases as G
import stat_device_cases as S

from mortal_amd import mjai_log as ML
from mortal_amd.dataset import GameplayLoader, Grp
from mortal_amd.stat import stat_logs

KEY = G.KEY
TF_ENDED, TF_DONE = 1 << 1, 1 << 3  # mortal_amd/csrc/mj_state.h
LOG_CAP = 16384


def even(n):
    return (int(n) + 1) & ~1


class Run:
    """A pool in refill mode driven by one of the two test policies, with the host's snapshot of every game that finishes.
    snaps[t] = one dict(words, err, cycle, g) per finished game of table t, in order; key (t, g) names generation g of table t."""

    def __init__(self, pool_cls, n, version=3, stride=None, stagger=0, max_games=None, max_words=None, seeds=None,
                 policy="greedy", poison=None, harvest=True, log_cap=LOG_CAP):
        self.n, self.stride, self.policy, self.poison = n, n if stride is None else stride, policy, poison
        self.seeds = list(seeds) if seeds is not None else G.seeds(n)
        self.first_g = 1 if stagger else 0  # a parked table is started by the refill path: its first game is generation 1
        self.pool = pool = pool_cls(n, version=version, deal_algo=0)
        try:
            pool.enable_log(log_cap)
            pool.reset(self.seeds, game_ids=np.arange(n), n_games_total=n)
            pool.set_refill(self.stride)
            if stagger:
                pool.set_start_stagger(stagger)
            if harvest:
                mg = 8 * n if max_games is None else max_games
                pool.enable_harvest(mg, mg * 4096 if max_words is None else max_words)
        except BaseException:
            pool.close()
            raise
        self.snaps = [[] for _ in range(n)]
        self.acts, self.c, self.games_seen, self.poisoned = None, 0, 0, False
        self.last_new = []  # keys snapshotted by the last step: finished, not yet restarted, so not yet collected

    def close(self):
        self.pool.close()

    def step(self):
        pool = self.pool
        n_rows = pool.step(self.acts)
        games = pool.counters()["games"]
        self.last_new = []
        if games > self.games_seen:
            logs = pool.read_logs()
            for t in range(self.n):
                d = pool.debug_table(t)
                fl = int(d["flags"][0])
                if (fl & TF_DONE) and (fl & TF_ENDED):
                    g = self.first_g + len(self.snaps[t])
                    self.snaps[t].append(dict(words=logs[t], err=int(d["err"][0]), cycle=self.c, g=g))
                    self.last_new.append((t, g))
            assert len(self.last_new) == games - self.games_seen, (self.last_new, games, self.games_seen)
            self.games_seen = games
        self.acts = None
        if n_rows[0]:
            obs, masks = pool.encode(0)
            if self.policy == "greedy":
                self.acts = pool.greedy_policy(0, masks, obs, G.POLICY_SEED, self.c)
            else:  # the lowest legal action, from the masks
                self.acts = masks.int().argmax(1).to(torch.int32).contiguous()
            if self.poison is not None and not self.poisoned and self.c >= self.poison[1]:
                hit = np.flatnonzero(pool.rows(0)[:, 0] == self.poison[0])
                if len(hit):
                    self.acts[int(hit[0])] = 46  # tests/table_error_cases.py kind id_46: no mask allows it
                    self.poisoned = True
        self.c += 1

    def play_until(self, cond, cap):
        """Step until cond(self), then once more (the step that restarts -- and collects -- what finished last).  Hitting the cap
        is a failure.  -> the keys every take so far must hold between them: all snapshots but those of the last step."""
        while not cond(self):
            assert self.c < cap, f"cycle cap {cap} hit"
            self.step()
        self.step()
        return self.collected()

    def collected(self):
        return sorted(set((t, s["g"]) for t in range(self.n) for s in self.snaps[t]) - set(self.last_new))

    def every_table(self, k):
        return lambda r: all(len(s) >= k for s in r.snaps)

    def snap(self, key):
        t, g = key
        return self.snaps[t][g - self.first_g]

    def seed(self, key):
        t, g = key
        return (self.seeds[t][0] + g * self.stride, self.seeds[t][1])

    def game_id(self, key):
        return key[0] + key[1] * self.n

    def events(self, key, names=G.NAMES):
        return [dict(type="start_game", names=list(names), seed=list(self.seed(key)))] + ML.decode_events(self.snap(key)["words"]) \
            + [dict(type="end_game")]


def mask_tag_rows(words):
    """The words with the two row fields of every reaction tag word cleared (LG_TAG_BIT: cycle | main row << 20 | kan-select row + 1
    << 38 | ...): the row of a table's seat in a cycle's batch is the one thing that differs between equal games on different tables.
    Tag words are found by walking the chain (a payload word can look like a header)."""
    out, i = np.array(words, dtype=np.uint64), 0
    rows = np.uint64(((1 << 36) - 1) << 20)
    while i < len(out):
        w = int(out[i])
        t = w & 15
        if t == ML.LG_START_KYOKU:
            i += 27 if (w >> 63) & 1 else 10
            continue
        tagged = (w >> 43) & 1
        if tagged:
            out[i + 1] &= ~rows
        i += (4 if t == ML.LG_HORA else 3 if t == ML.LG_RYUKYOKU else 1) + tagged
    assert i == len(out)
    return out


def keys_of(run, h):
    """The (table, generation) of every record, in the harvest's order."""
    return [(int(r["table"]), int(r["game_id"]) // run.n) for r in h.games]


def check_records(run, h, want_keys, aos=0):
    """The harvest holds exactly want_keys, sorted by (game_id, table), every field and every word as the host saw them."""
    keys = keys_of(run, h)
    assert h.n_games == len(h.games) == len(keys)
    assert sorted(keys) == sorted(want_keys), (sorted(set(want_keys) - set(keys)), sorted(set(keys) - set(want_keys)))
    assert keys == sorted(keys, key=lambda k: (run.game_id(k), k[0])), "not sorted by (game_id, table)"
    logs = h.read_logs()
    scores0, done0 = run.pool.results()
    n_err = 0
    for i, key in enumerate(keys):
        r, sn = h.games[i], run.snap(key)
        assert (int(r["seed_nonce"]), int(r["seed_key"])) == run.seed(key), (key, r)
        assert int(r["game_id"]) == run.game_id(key) and int(r["agent_of_seat"]) == aos
        assert int(r["err"]) == sn["err"], (key, r["err"], sn["err"])
        assert int(r["cycle"]) == sn["cycle"] + 1, key  # collected by the step after the one that finished it
        if sn["err"]:
            n_err += 1
            assert int(r["n_words"]) == 0 and len(logs[i]) == 0
            continue
        assert int(r["n_words"]) == len(sn["words"]) and int(r["first_word"]) % 2 == 0
        assert (logs[i] == sn["words"]).all(), key
        final = Grp.load_events(ML.decode_events(sn["words"])).final_scores
        assert r["scores"].tolist() == final, (key, r["scores"], final)
        if key[1] == 0:
            assert done0[key[0]] == 1 and scores0[key[0]].tolist() == r["scores"].tolist(), key
    assert h.n_errors == n_err and h.n_words == sum(int(x) for x in h.games["n_words"])
    return keys


def check_stat_and_grp(run, h, lib, aos=0):
    """Harvest.stat() and Harvest.grp() against the host route over the snapshot words."""
    keys = keys_of(run, h)
    words = [run.snap(k)["words"] if not run.snap(k)["err"] else np.zeros(0, dtype=np.uint64) for k in keys]
    n = len(keys)
    n_skip = sum(1 for w in words if len(w) == 0)
    totals, rows, counts = h.stat(per_seat=True)
    assert counts == dict(reduced=n - n_skip, skipped=n_skip, malformed=0), counts
    want_tot, want_rows, want_counts = stat_logs(words, groups=np.full(n, aos, dtype=np.uint8), per_seat=True, lib=lib)
    assert want_counts == counts
    assert (rows == want_rows).all() and (rows == S.expected(words)).all()
    assert [t.counters() for t in totals] == [t.counters() for t in want_tot]
    assert totals[0].game + totals[1].game == 4 * (n - n_skip)
    seats = np.array([(5, 10, 15, 0)[i % 4] for i in range(n)], dtype=np.uint8)
    tot2, rows2, _ = h.stat(seats=seats, per_seat=True)
    want2 = S.totals_of(want_rows, seats, np.full(n, aos, dtype=np.uint8))
    assert (np.array([t.counters() for t in tot2], dtype=np.int64) == want2).all()
    grps = h.grp()
    assert len(grps) == n
    for i, k in enumerate(keys):
        if len(words[i]) == 0:
            assert grps[i] is None
        else:
            G.same_grp(grps[i], Grp.load_events(ML.decode_events(words[i])))
    if n > 2:  # a range
        for g, w in zip(h.grp(1, n - 2), words[1:-1]):
            if len(w):
                G.same_grp(g, Grp.load_events(ML.decode_events(w)))


def check_samples(oracle, run, h, game0, seat_masks, version=3, always_kan=True):
    """load_harvest over games [game0, game0 + len(seat_masks)) against the reference loader, Gameplay by Gameplay."""
    keys = keys_of(run, h)
    k = len(seat_masks)
    loader = GameplayLoader(version, oracle=False, always_include_kan_select=always_kan)
    got = loader.load_harvest(h, game0=game0, n_games=k, seats=seat_masks, names=[G.NAMES] * k)
    assert len(got) == k
    total = 0
    for i in range(k):
        key = keys[game0 + i]
        if run.snap(key)["err"]:
            assert got[i] == [], key
            continue
        assert [g.player_id for g in got[i]] == [p for p in range(4) if (int(seat_masks[i]) >> p) & 1], key
        ev = run.events(key)
        for g in got[i]:
            total += G.check_gameplay(oracle, g, ev, version, always_kan)
    return total


def check_invisible(oracle, run, h, game0, k, version=1):
    """Case 7: oracle=True deals every wall from the seed recorded with the game."""
    keys = keys_of(run, h)
    got = GameplayLoader(version, oracle=True, deal_algo=0).load_harvest(h, game0=game0, n_games=k)
    assert len(got) == k
    total = 0
    for i in range(k):
        key = keys[game0 + i]
        assert key[1] >= 1  # a game whose seed is not the one the pool was reset with
        ev = run.events(key, ["", "", "", ""])
        assert [g.player_id for g in got[i]] == [0, 1, 2, 3]
        for g in got[i]:
            ref = dataset_ref.load_invisible_by_player(oracle, ev, g.player_id, version)
            inv = g.take_invisible_obs()
            assert len(inv) == len(ref) == len(g.actions) > 0
            for j in range(len(ref)):
                assert (inv[j].view(np.uint32) == ref[j].view(np.uint32)).all(), (key, g.player_id, j)
            total += len(ref)
    return total


def harvest_bytes(h, first_samples=True):
    """Every byte a harvest hands out: records, words, Stat rows, and the samples of its first game."""
    out = [h.games.tobytes()] + [w.tobytes() for w in h.read_logs()]
    totals, rows, counts = h.stat(per_seat=True)
    out += [rows.tobytes(), repr(counts).encode(), repr([t.counters() for t in totals]).encode()]
    if first_samples and h.n_games:
        out.append(G.samples_bytes(GameplayLoader(3, oracle=False).load_harvest(h, 0, 1)))
    return b"".join(out)


# ---- case 1 (its run is shared by cases 7 and 8)
def two_generations(pool_cls, n):
    """n tables, obs v3, greedy policy, refill with stride n, no stagger, until every table has finished two games; one take at the
    end.  -> (run, harvest, keys).  The cap of three times the first generation's cycle count is a failure when hit."""
    run = Run(pool_cls, n)
    try:
        run.play_until(run.every_table(1), 8000)
        first = run.c
        want = run.play_until(run.every_table(2), 3 * first)
        pending = run.pool.harvest_pending()
        h = run.pool.take_harvest()
        assert pending["games"] == h.n_games and pending["dropped"] == h.dropped == 0
        return run, h, want
    except BaseException:
        run.close()
        raise


def check_two_generations(run, h, want, lib):
    """Every game that was restarted is in the take, exactly once; both generations of every table are among them.  (A table may
    finish a third game before the slowest finishes its second: the take then holds it too, as the snapshots say.)"""
    n = run.n
    assert set(want) >= set((t, g) for t in range(n) for g in (0, 1)) and len(want) >= 2 * n
    print("two generations:", len(want), "games,", run.c, "cycles")
    keys = check_records(run, h, want)
    assert keys[:n] == [(t, 0) for t in range(n)] and keys[n:2 * n] == [(t, 1) for t in range(n)]
    # both tails of the 16-byte copy: logs of an odd and of an even number of words
    assert set(int(x) & 1 for x in h.games["n_words"]) == {0, 1}
    check_stat_and_grp(run, h, lib)


# ---- case 2
def check_many_in_one_step(pool_cls, n, same, lib, log_cap=LOG_CAP):
    """The tables `same` share one seed and every seat plays the lowest legal action: their games end on the same cycle, so one
    launch of the kernel collects several games per wavefront, from every block that holds some."""
    seeds = [(G.SEED_START if t in same else G.SEED_START + 1 + t, KEY) for t in range(n)]
    run = Run(pool_cls, n, seeds=seeds, policy="lowest", log_cap=log_cap)
    try:
        want = run.play_until(lambda r: all(len(r.snaps[t]) >= 1 for t in same), 8000)
        ends = set(run.snaps[t][0]["cycle"] for t in same)
        assert len(ends) == 1, ends
        h = run.pool.take_harvest()
        try:
            keys = check_records(run, h, want)
            logs = h.read_logs()
            mine = [i for i, k in enumerate(keys) if k[0] in same and k[1] == 0]
            assert len(mine) == len(same)
            ranges = sorted((int(h.games["first_word"][i]), int(h.games["n_words"][i])) for i in mine)
            for (a, na), (b, _nb) in zip(ranges, ranges[1:]):
                assert a + even(na) <= b, ranges  # no two games share a word
            # word for word the host snapshot, and word for word each other -- but for the row index a reaction's tag word carries
            # (the row of the table's seat in that cycle's batch, which no two tables share): those two fields are masked out
            first = mask_tag_rows(logs[mine[0]])
            for i in mine:
                assert len(logs[i]) > 64 and (logs[i] == run.snaps[keys[i][0]][0]["words"]).all()
                assert len(logs[i]) == len(first) and (mask_tag_rows(logs[i]) == first).all()
            check_stat_and_grp(run, h, lib)
        finally:
            h.close()
    finally:
        run.close()


# ---- case 3
def check_take_while_playing(pool_cls, n):
    run = Run(pool_cls, n)
    try:
        want1 = run.play_until(run.every_table(1), 8000)
        first = run.c
        p1 = run.pool.harvest_pending()
        h1 = run.pool.take_harvest()
        assert run.pool.harvest_pending() == dict(games=0, words=0, dropped=0)
        check_records(run, h1, want1)
        assert p1["games"] == h1.n_games and p1["words"] == sum(even(x) for x in h1.games["n_words"]) and p1["dropped"] == 0
        bytes1 = harvest_bytes(h1)
        all_keys = run.play_until(run.every_table(2), 3 * first)
        p2 = run.pool.harvest_pending()
        h2 = run.pool.take_harvest()
        want2 = sorted(set(all_keys) - set(want1))
        check_records(run, h2, want2)  # the two harvests together hold every game exactly once
        assert p2["games"] == h2.n_games == len(want2) and p2["words"] == sum(even(x) for x in h2.games["n_words"])
        assert harvest_bytes(h1) == bytes1  # untouched by the later steps and by the second take
        h2.close()
        assert harvest_bytes(h1) == bytes1
        h1.close()
    finally:
        run.close()


# ---- case 4
def check_full_buffer(pool_cls, n):
    """max_games = 2, then max_words just below two games' words: what does not fit is dropped and counted, the pool plays on, and
    after a take collection resumes."""
    run = Run(pool_cls, n, max_games=2)
    try:
        want = run.play_until(run.every_table(1), 8000)
        first = run.c
        assert len(want) >= n > 2
        assert run.pool.harvest_pending() == dict(games=2, words=run.pool.harvest_pending()["words"], dropped=len(want) - 2)
        assert run.pool.first_error()[0] == 0
        h = run.pool.take_harvest()
        kept = keys_of(run, h)
        assert h.n_games == 2 and h.dropped == len(want) - 2 and set(kept) <= set(want)
        check_records(run, h, kept)
        h.close()
        games_before = run.pool.counters()["games"]
        later = run.play_until(lambda r: r.pool.counters()["games"] >= games_before + 2, 3 * first)
        assert run.pool.first_error()[0] == 0 and run.pool.counters()["games"] > games_before
        h = run.pool.take_harvest()  # collection has resumed
        kept2 = keys_of(run, h)
        assert h.n_games == 2 and set(kept2) <= set(later) - set(want) and h.dropped == len(later) - len(want) - 2
        check_records(run, h, kept2)
        h.close()
        order = sorted(want, key=lambda k: run.snap(k)["cycle"])
        lens = [len(run.snap(k)["words"]) for k in order]
    finally:
        run.close()
    max_words = even(lens[0]) + even(lens[1]) - 2  # whichever of the first two arrives second does not fit
    run = Run(pool_cls, n, max_games=64, max_words=max_words)
    try:
        want = run.play_until(run.every_table(1), 8000)
        p = run.pool.harvest_pending()
        h = run.pool.take_harvest()
        kept = keys_of(run, h)
        assert 1 <= h.n_games < len(want) and h.dropped == len(want) - h.n_games == p["dropped"] and set(kept) <= set(want)
        for r in h.games:  # no record's word range leaves the buffer
            assert int(r["first_word"]) + even(r["n_words"]) <= max_words, (r, max_words)
        assert p["words"] <= max_words
        check_records(run, h, kept)
        assert run.pool.first_error()[0] == 0
        h.close()
    finally:
        run.close()


# ---- case 5
def check_table_in_error(oracle, pool_cls, n, victim, lib):
    run = Run(pool_cls, n, poison=(victim, 60))
    try:
        run.play_until(run.every_table(1), 8000)
        first = run.c
        want = run.play_until(lambda r: len(r.snaps[victim]) >= 2 and r.every_table(1)(r), 3 * first)
        assert run.poisoned and run.snaps[victim][0]["err"] == 1  # MJ_ERR_ILLEGAL_ACTION
        assert run.snaps[victim][1]["err"] == 0
        h = run.pool.take_harvest()
        try:
            keys = check_records(run, h, want)
            i = keys.index((victim, 0))
            assert int(h.games["err"][i]) == 1 and int(h.games["n_words"][i]) == 0 and h.n_errors == 1
            check_stat_and_grp(run, h, lib)  # (skipped: counts and None)
            rp = pool_cls(n, version=3)
            try:
                assert rp.replay_load_harvest(h, 0) == dict(loaded=n - 1, skipped=1, malformed=0)
            finally:
                rp.close()
            assert check_samples(oracle, run, h, 0, [15] * n) > 0  # generation 0: the victim's list is empty, the neighbours' are the reference's
            j = keys.index((victim, 1))  # the table's next generation is collected normally
            assert int(h.games["n_words"][j]) == len(run.snaps[victim][1]["words"]) > 64
            assert check_samples(oracle, run, h, j, [9]) > 0
        finally:
            h.close()
    finally:
        run.close()


# ---- case 6
def check_staggered_start(pool_cls, n, stagger, lib):
    run = Run(pool_cls, n, stagger=stagger)
    try:
        for _ in range(stagger + 2):  # every table has entered play; the parked ones gave no record
            run.step()
        assert run.pool.harvest_pending()["games"] == len(run.collected())
        want = run.play_until(run.every_table(1), 8000)
        h = run.pool.take_harvest()
        try:
            keys = check_records(run, h, want)
            assert all(g >= 1 for _, g in keys) and set((t, 1) for t in range(n)) <= set(keys)
            for w in h.read_logs():
                ev = ML.decode_events(w)
                assert ev[0]["type"] == "start_kyoku" and (ev[0]["bakaze"], ev[0]["kyoku"], ev[0]["honba"]) == ("E", 1, 0)
                assert ev[0]["scores"] == [25000] * 4 and ev[-1]["type"] == "end_kyoku"
            check_stat_and_grp(run, h, lib)
        finally:
            h.close()
    finally:
        run.close()


# ---- case 8
def check_refusals(pool_cls, run, h):
    """Each refused call names its reason and leaves things usable."""
    import pytest

    pool = run.pool
    want = harvest_bytes(h)
    plain = pool_cls(2, version=3)  # no log
    plain.reset(G.seeds(2))
    nohv = pool_cls(2, version=3)   # a log, refill, no harvest
    nohv.enable_log()
    nohv.reset(G.seeds(2))
    nohv.set_refill(2)
    dst = pool_cls(2, version=3)
    try:
        with pytest.raises(RuntimeError, match="log is not enabled"):
            plain.enable_harvest(4, 4096)
        for call in (nohv.take_harvest, nohv.harvest_pending):
            with pytest.raises(RuntimeError, match="harvesting is not enabled"):
                call()
        for game0 in (-1, h.n_games - 1, h.n_games):
            with pytest.raises(RuntimeError, match="out of bounds"):
                dst.replay_load_harvest(h, game0)
        with pytest.raises(RuntimeError, match="out of bounds"):
            h.grp(h.n_games - 1, 2)
        with pytest.raises(ValueError, match="augmented"):
            GameplayLoader(3, oracle=False, augmented=True).load_harvest(h)
        with pytest.raises(ValueError, match="are not in a harvest"):
            GameplayLoader(3, oracle=False).load_harvest(h, h.n_games - 1, 2)
        # the pool routes still refuse a pool in refill mode
        with pytest.raises(RuntimeError, match="refill mode"):
            pool.log_stat()
        with pytest.raises(RuntimeError, match="refill mode"):
            pool.log_grp()
        with pytest.raises(RuntimeError, match="refill mode"):
            dst.replay_load_pool(pool)
        with pytest.raises(RuntimeError, match="refill mode"):
            GameplayLoader(3, oracle=False).load_pool(pool)
        assert dst.replay_load_harvest(h, 0) == dict(loaded=2, skipped=0, malformed=0)  # dst is usable
        assert dst.replay_step() > 0
        assert harvest_bytes(h) == want
        pool.harvest_pending()  # so is the pool
        # a closed harvest
        h2 = pool.take_harvest()
        h2.close()
        h2.close()
        for call in (h2.read_logs, h2.stat, h2.grp, lambda: dst.replay_load_harvest(h2), lambda: GameplayLoader(3, oracle=False).load_harvest(h2, 0, 1)):
            with pytest.raises(RuntimeError, match="closed"):
                call()
    finally:
        for p in (plain, nohv, dst):
            p.close()


# ---- case 10
def check_self_play_runner(oracle, pool_cls, n_tables):
    """SelfPlayRunner with two lowest-legal engines "a" and "b": Stat by engine name and the samples of b's seats against the host
    snapshot of every game, taken the same way as Run takes them."""
    import test_sharding as TS

    from mortal_amd import arena as A
    from mortal_amd.stat import Stat

    old = A.SelfPlayRunner.pool_cls
    A.SelfPlayRunner.pool_cls = pool_cls
    try:
        aos = np.array([(0b0001, 0b0100, 0b1010, 0b0110)[t % 4] for t in range(n_tables)], dtype=np.uint8)
        runner = A.SelfPlayRunner([TS._LowestLegalEngine("a"), TS._LowestLegalEngine("b")], n_tables, (10000, KEY), aos, deal_algo=0,
                                  max_games=8 * n_tables, max_words=8 * n_tables * 4096)
        try:
            pool = runner.pool
            snaps = {}
            seen = [0]
            counts = [0] * n_tables

            def watch(_runner):
                games = pool.counters()["games"]
                if games > seen[0]:
                    logs = pool.read_logs()
                    for t in range(n_tables):
                        fl = int(pool.debug_table(t)["flags"][0])
                        if (fl & TF_DONE) and (fl & TF_ENDED):
                            snaps[(t, counts[t])] = logs[t]
                            counts[t] += 1
                    seen[0] = games

            h = runner.play(min_games=2 * n_tables, on_step=watch)
            try:
                assert h.n_games >= 2 * n_tables and h.n_errors == 0 and h.dropped == 0
                keys = [(int(r["table"]), int(r["game_id"]) // n_tables) for r in h.games]
                logs = h.read_logs()
                want = {"a": Stat(), "b": Stat()}
                for i, key in enumerate(keys):
                    t, g = key
                    assert (logs[i] == snaps[key]).all(), key
                    assert (int(h.games["seed_nonce"][i]), int(h.games["seed_key"][i])) == (10000 + t + g * n_tables, KEY)
                    assert int(h.games["agent_of_seat"][i]) == int(aos[t])  # the same for every generation of a table
                    ev = ML.decode_events(snaps[key])
                    for s in range(4):
                        want["b" if (int(aos[t]) >> s) & 1 else "a"] += Stat.from_game(ev, s)
                got = runner.stats(h)
                assert set(got) == {"a", "b"}
                for name in want:
                    assert got[name].counters() == want[name].counters(), name
                k = min(h.n_games, 3)
                loader = GameplayLoader(3, oracle=False, player_names=["b"])
                gps = runner.gameplays(loader, h)
                assert len(gps) == h.n_games
                for i, key in enumerate(keys):
                    t = key[0]
                    assert [g.player_id for g in gps[i]] == [s for s in range(4) if (int(aos[t]) >> s) & 1], key
                    assert all(g.player_name == "b" for g in gps[i])
                for i in range(k):
                    t, g = keys[i]
                    names = ["b" if (int(aos[t]) >> s) & 1 else "a" for s in range(4)]
                    ev = [dict(type="start_game", names=names, seed=[10000 + t + g * n_tables, KEY])] + ML.decode_events(snaps[keys[i]]) \
                        + [dict(type="end_game")]
                    for gp in gps[i]:
                        assert G.check_gameplay(oracle, gp, ev, 3, True) > 0
                assert [len(x) for x in runner.gameplays(loader, h, seats=[0] * h.n_games)] == [0] * h.n_games
            finally:
                h.close()
        finally:
            runner.close()
    finally:
        A.SelfPlayRunner.pool_cls = old
