"""Shared by tests/test_gpu_sample_store.py (the real library, `-m gpu`) and tests/test_emu_sample_store.py (host emulation of the
device code): the sample store (mortal_amd/csrc/mj_samples.hip behind mj_samples_*; SampleStore, GameplayLoader.store_pool /
store_harvest, BatchRunner.sample_store / SelfPlayRunner.sample_store).

The yardsticks are never the code under test: every sample is compared with the reference loader restated on the oracle
(tests/dataset_ref.py, through pool_gameplay_cases.check_gameplay and ref_events) over `decode_events(pool.read_logs()[t])`, the
invisible obs with dataset_ref.load_invisible_by_player (walls from invisibles_from_seed), the augmented samples with the yardstick
of tests/pool_augment_cases.py (the reference loader over the suit-swapped events), the harvest's with the host's own snapshot of
every finished game (tests/harvest_cases.py Run).  Obs are compared bit for bit, masks and columns exactly, and every sample of a
compared game is compared.

Games come from pool_gameplay_cases.play (seeds SEED_START + t under the greedy test policy).  The parity range is tables 1 and 2
under the seat masks [15, 6]; counted on the reference side (census() below) it holds 7 kan labels with their select row and 8
events that give rows to two seats of one game (tables 0 and 1 were tried first: 4 and 4 -- the range with more was taken)."""
import numpy as np
import pytest
import torch

import dataset_ref
import harvest_cases as H
import pool_augment_cases as A
import pool_gameplay_cases as G

from mortal_amd._lib import MortalAmdError
from mortal_amd.dataset import GameplayLoader, Grp
from mortal_amd.pool import OBS_ROWS
from mortal_amd.samples import SampleStore

TABLE0, SEATS = 1, [15, 6]
OBS_POISON, MASK_POISON = 0x7FC0DEAD, 0xA5  # a NaN no encoder writes; a byte no bool holds


class Played:
    """A finished pool, its logs as the host reads them, and the reference's reading of its games, each computed once."""

    def __init__(self, oracle, pool_cls, n):
        self.oracle, self.pool_cls, self.lib = oracle, pool_cls, pool_cls._L
        self.pool = G.play(pool_cls, n)
        self.logs = self.pool.read_logs()
        self._ref = {}

    def close(self):
        self.pool.close()

    def events(self, t, names=G.NAMES):
        return G.ref_events(self.pool, self.logs, t, names)

    def ref(self, t, seat, version):
        """The reference loader's Gameplay of (table, seat) -- shared, never changed."""
        key = (t, seat, version)
        if key not in self._ref:
            self._ref[key] = dataset_ref.load_events_by_player(self.oracle, self.events(t), seat, version, True)
        return self._ref[key]

    def store(self, version, batch_rows, capacity=4000):
        return SampleStore(capacity, version, batch_rows=batch_rows, lib=self.lib)


def seats_of(mask):
    return [p for p in range(4) if (int(mask) >> p) & 1]


def census(oracle, events_list, seat_masks):
    """Counted on the reference side: kan labels followed by their select row; events that give rows to two seats of one game;
    rows that share their event (and so their record) with another row of the game."""
    kan = two_seat = shared_rows = 0
    for ev, m in zip(events_list, seat_masks):
        rows_at = {}
        for p in seats_of(m):
            for i, k in dataset_ref.entry_event_indices(oracle, ev, p, True):
                kan += k == 2
                rows_at.setdefault(i, []).append(k)
        two_seat += sum(1 for v in rows_at.values() if len(v) >= 2)
        shared_rows += sum(sum(v) for v in rows_at.values() if sum(v) >= 2)
    return dict(kan_select=kan, two_seat_events=two_seat, shared_rows=shared_rows)


def shared_rows_of(meta):
    """The same count on the store side: rows of meta whose (game, event index) another row has too."""
    _, inv, cnt = np.unique(meta[:, [1, 7]], axis=0, return_inverse=True, return_counts=True)
    return int((cnt[inv.reshape(-1)] >= 2).sum())


def steps_to_done_ref(dones, apply_gamma):
    """mortal/dataloader.py:110-113, as written there."""
    n = len(dones)
    out = np.zeros(n, dtype=np.int64)
    for i in reversed(range(n)):
        if not dones[i]:
            out[i] = out[i + 1] + int(apply_gamma[i])
    return out


def poisoned(n, tail, device, dtype):
    """n rows and one guard row of the poison pattern."""
    if dtype == torch.bool:
        return torch.full((n + 1,) + tail, MASK_POISON, dtype=torch.uint8, device=device).view(torch.bool)
    return torch.full((n + 1,) + tail, OBS_POISON, dtype=torch.int32, device=device).view(torch.float32)


def is_poison(t):
    if t.dtype == torch.bool:
        return bool((t.view(torch.uint8) == MASK_POISON).all())
    return bool((t.view(torch.int32) == OBS_POISON).all())


def encode_guarded(store, idx):
    """store.encode into poisoned buffers -> (obs, masks) as numpy; the guard row behind the batch must keep its pattern."""
    n = len(idx)
    obs, masks = poisoned(n, (store.C, 34), store.device, torch.float32), poisoned(n, (46,), store.device, torch.bool)
    o, m = store.encode(idx, obs=obs, masks=masks)
    assert o.data_ptr() == obs.data_ptr() and m.data_ptr() == masks.data_ptr() and len(o) == len(m) == n
    assert is_poison(obs[n:]) and is_poison(masks[n:]), "the guard row was written"
    return o.cpu().numpy(), m.view(torch.uint8).cpu().numpy()


def truth(P, store, table0, seat_masks, version):
    """The reference's obs and mask of every sample, by store index: sample span(g, p)[k] is entry k of the reference's Gameplay
    (the order itself is checked by check_parity).  -> (obs uint32 [count, C, 34], masks uint8 [count, 46])."""
    obs = np.zeros((store.count, OBS_ROWS[version], 34), dtype=np.uint32)
    masks = np.full((store.count, 46), 0xFF, dtype=np.uint8)
    seen = np.zeros(store.count, dtype=bool)
    for g, m in enumerate(seat_masks):
        for p in seats_of(m):
            ref, span = P.ref(table0 + g, p, version), store.span(g, p)
            assert len(span) == len(ref["obs"])
            for k, i in enumerate(span):
                obs[i], masks[i] = ref["obs"][k].view(np.uint32), ref["masks"][k]
            seen[span] = True
    assert seen.all(), "a sample belongs to no compared Gameplay"
    return obs, masks


# ---- case 1
def check_parity(P, version, table0, seat_masks, batch_rows, want_census=False):
    """store_pool over tables [table0, table0 + len(seat_masks)) against the reference loader, Gameplay by Gameplay, then the
    columns over the whole store.  -> the number of samples compared (= the store's count)."""
    n = len(seat_masks)
    events = [P.events(table0 + g) for g in range(n)]
    store = P.store(version, batch_rows)
    try:
        got = GameplayLoader(version, oracle=False).store_pool(P.pool, table0, n, seats=seat_masks, names=[G.NAMES] * n, store=store)
        assert got is store and store.count == len(store) > 0 and len(store.grps) == n
        total = 0
        pos_seen = np.zeros(store.count, dtype=bool)
        for g in range(n):
            assert store.wanted[g] == seats_of(seat_masks[g])
            G.same_grp(store.grps[g], Grp.load_events(events[g]))
            for p in store.wanted[g]:
                total += G.check_gameplay(P.oracle, store.gameplay(g, p), events[g], version, True)
                # the columns, in the reference's order, against the reference's lists
                ref = P.ref(table0 + g, p, version)
                pos = np.flatnonzero((store.game == g) & (store.seat == p))
                assert len(pos) == len(ref["actions"]) and (np.diff(pos) == 1).all() and not pos_seen[pos].any()
                pos_seen[pos] = True
                assert (store.order[pos] == store.span(g, p)).all()
                for col, key in (("actions", "actions"), ("at_kyoku", "at_kyoku"), ("at_turns", "at_turns"), ("shantens", "shantens"),
                                 ("apply_gamma", "apply_gamma"), ("dones", "dones")):
                    assert getattr(store, col)[pos].tolist() == ref[key], (g, p, col)
                assert (store.steps_to_done[pos] == steps_to_done_ref(ref["dones"], ref["apply_gamma"])).all(), (g, p)
        assert total == store.count and pos_seen.all()  # no sample left out
        assert sorted(store.order.tolist()) == list(range(store.count))
        if want_census:
            cs = census(P.oracle, events, seat_masks)
            print("census", cs)
            assert cs["kan_select"] >= 1 and cs["two_seat_events"] >= 1, cs
            assert shared_rows_of(store.meta) == cs["shared_rows"]
        store.check_overflow()
        return total
    finally:
        store.close()


# ---- case 2
def batch_plan(count, batch_rows, seed=5):
    """Index lists drawn from one fixed-seed permutation: 1, batch_rows, batch_rows + 1 and 3 * batch_rows - 5 of them, one batch
    with a duplicated index, one with the first and the last sample."""
    perm = np.random.default_rng(seed).permutation(count)
    sizes = [1, batch_rows, batch_rows + 1, 3 * batch_rows - 5]
    assert count >= sum(sizes) + 2
    plan, at = [], 0
    for k in sizes:
        plan.append(perm[at:at + k])
        at += k
    plan.append(np.array([perm[at], perm[at + 1], perm[at]]))
    plan.append(np.array([count - 1, 0]))
    return plan


def check_shuffled(P, version, table0, seat_masks, batch_rows):
    n = len(seat_masks)
    store = P.store(version, batch_rows)
    try:
        GameplayLoader(version, oracle=False).store_pool(P.pool, table0, n, seats=seat_masks, store=store)
        want_obs, want_masks = truth(P, store, table0, seat_masks, version)
        rows = 0
        for idx in batch_plan(store.count, batch_rows):
            obs, masks = encode_guarded(store, idx)
            assert (obs.view(np.uint32) == want_obs[idx]).all(), idx[:8]
            assert (masks == want_masks[idx]).all(), idx[:8]
            rows += len(idx)
        store.check_overflow()
        return rows
    finally:
        store.close()


# ---- case 3
def check_invisible(P, version, table, seat_mask, batch_rows=24):
    """oracle=True deals the walls from the table's seed; encode_oracle(span) is the reference's invisible_obs of that Gameplay."""
    store = P.store(version, batch_rows)
    try:
        GameplayLoader(version, oracle=True, deal_algo=0).store_pool(P.pool, table, 1, seats=[seat_mask], store=store)
        assert store.has_walls
        ev = P.events(table, ["", "", "", ""])
        total = 0
        for p in seats_of(seat_mask):
            ref = dataset_ref.load_invisible_by_player(P.oracle, ev, p, version)
            span = store.span(0, p)
            inv = store.encode_oracle(span).cpu().numpy()
            assert len(inv) == len(ref) == len(span) > 0
            for k in range(len(ref)):
                assert (inv[k].view(np.uint32) == ref[k].view(np.uint32)).all(), (p, k)
            assert np.stack(store.gameplay(0, p).invisible_obs).tobytes() == inv.tobytes()
            total += len(ref)
        assert total == store.count
        return total
    finally:
        store.close()


# ---- case 4
def check_augmented(P, table, seat_mask, version=3, batch_rows=24):
    """store_pool(augmented=True) against the reference loader over the suit-swapped events."""
    store = P.store(version, batch_rows)
    try:
        loader = GameplayLoader(version, oracle=False)
        loader.store_pool(P.pool, table, 1, seats=[seat_mask], names=[G.NAMES], augmented=True, store=store)
        ev = A.ref_game(G.seeds(P.pool.n_tables)[table], P.logs[table], G.NAMES)
        total = sum(G.check_gameplay(P.oracle, store.gameplay(0, p), ev, version, True) for p in seats_of(seat_mask))
        assert total == store.count > 0
        swapped = encode_guarded(store, np.arange(store.count))[0].tobytes()
        store.clear()
        loader.store_pool(P.pool, table, 1, seats=[seat_mask], names=[G.NAMES], store=store)
        assert total == store.count and encode_guarded(store, np.arange(store.count))[0].tobytes() != swapped
        return total
    finally:
        store.close()


# ---- case 5
def check_harvest(oracle, pool_cls, n=2, victim=1, version=3, batch_rows=24):
    """Two store_harvest calls into one store, over a harvest that holds a game in error."""
    run = H.Run(pool_cls, n, poison=(victim, 60))
    try:
        run.play_until(run.every_table(1), 8000)
        h = run.pool.take_harvest()
        store = SampleStore(8000, version, batch_rows=batch_rows, lib=pool_cls._L)
        try:
            keys = H.keys_of(run, h)
            bad = [i for i, k in enumerate(keys) if run.snap(k)["err"]]
            assert bad and len(keys) - len(bad) >= 1 and len(keys) >= 2
            masks = [(3, 12, 15)[i % 3] for i in range(len(keys))]
            loader = GameplayLoader(version, oracle=False)
            cut = max(1, len(keys) // 2)
            loader.store_harvest(h, 0, cut, seats=masks[:cut], names=[G.NAMES] * cut, store=store)
            assert len(store.grps) == cut
            first = store.count
            loader.store_harvest(h, cut, None, seats=masks[cut:], names=[G.NAMES] * (len(keys) - cut), store=store)
            assert len(store.grps) == len(keys) and store.count >= first  # games numbered on
            total = 0
            for i, key in enumerate(keys):
                if i in bad:  # a game in error contributes nothing
                    assert store.grps[i] is None and store.wanted[i] == [] and not (store.game == i).any()
                    continue
                ev = run.events(key)
                G.same_grp(store.grps[i], Grp.load_events(ev))
                assert store.wanted[i] == seats_of(masks[i])
                for p in store.wanted[i]:
                    total += G.check_gameplay(oracle, store.gameplay(i, p), ev, version, True)
            assert total == store.count > 0
            assert int(store.meta[:first, 1].max(initial=-1)) < cut <= int(store.meta[first:, 1].min(initial=cut))
            h.close()
            with pytest.raises(MortalAmdError, match="Harvest is closed"):
                loader.store_harvest(h, store=store)
            assert store.count == total
            return total
        finally:
            store.close()
            h.close()
    finally:
        run.close()


# ---- case 6
def store_bytes(store):
    obs, masks = encode_guarded(store, np.arange(store.count))
    return obs.tobytes() + masks.tobytes() + store.meta.tobytes()


def check_capacity_and_refusals(P, version=3, batch_rows=24):
    pool, lib = P.pool, P.lib
    loader = GameplayLoader(version, oracle=False)
    probe = loader.store_pool(pool, 1, 1, seats=[2], capacity=4000, batch_rows=batch_rows)
    n1 = probe.count
    loader.store_pool(pool, 2, 1, seats=[4], store=probe)
    n2 = probe.count - n1
    want_both = store_bytes(probe)
    probe.close()
    assert n1 > 50 and n2 > 50
    # filled to exactly its capacity
    exact = SampleStore(n1 + n2, version, batch_rows=batch_rows, lib=lib)
    short = SampleStore(n1 + n2 - 1, version, batch_rows=batch_rows, lib=lib)
    try:
        loader.store_pool(pool, 1, 1, seats=[2], store=exact)
        loader.store_pool(pool, 2, 1, seats=[4], store=exact)
        assert exact.count == exact.capacity == n1 + n2 and store_bytes(exact) == want_both
        # one sample short: the second call raises and the store is what it was
        loader.store_pool(pool, 1, 1, seats=[2], store=short)
        before, grps = store_bytes(short), list(short.grps)
        with pytest.raises(MortalAmdError, match="do not fit a store"):
            loader.store_pool(pool, 2, 1, seats=[4], store=short)
        assert short.count == n1 and short.grps == grps and len(short.names) == len(short.wanted) == 1
        assert store_bytes(short) == before
        with pytest.raises(ValueError, match="are not in a pool"):
            loader.store_pool(pool, pool.n_tables - 1, 2, store=short)
        with pytest.raises(ValueError, match=r"augmented.*per call"):
            GameplayLoader(version, oracle=False, augmented=True).store_pool(pool, store=short)
        with pytest.raises(ValueError, match="the store holds obs v3"):
            GameplayLoader(1, oracle=False).store_pool(pool, 1, 1, store=short)
        assert short.count == n1 and short.grps == grps and store_bytes(short) == before
        # refused indices: nothing is written
        for bad in ([-1], [0, short.count], [3, -1, 2]):
            obs, masks = poisoned(len(bad), (short.C, 34), short.device, torch.float32), poisoned(len(bad), (46,), short.device, torch.bool)
            with pytest.raises(MortalAmdError, match="is not in a store of"):
                short.encode(bad, obs=obs, masks=masks)
            assert is_poison(obs) and is_poison(masks)
            out = poisoned(len(bad), (lib.mj_oracle_obs_rows(version), 34), short.device, torch.float32)
            with pytest.raises(MortalAmdError, match="is not in a store of"):
                short.encode_oracle(bad, out=out)
            assert is_poison(out)
        assert short.encode([])[0].shape == (0, short.C, 34)
        # an append from a pool with no script
        plain = P.pool_cls(2, version=version)
        try:
            plain.reset(G.seeds(2))
            with pytest.raises(MortalAmdError, match="no replay script"):
                short.append(plain, 0)
        finally:
            plain.close()
        assert short.count == n1 and store_bytes(short) == before
        with pytest.raises(MortalAmdError, match=r"mj_samples_truncate"):
            short.truncate(n1 + 1)
        # a capacity of 2^28
        with pytest.raises(MortalAmdError, match="capacity 268435456 is not in"):
            SampleStore(1 << 28, version, batch_rows=batch_rows, lib=lib)
        with pytest.raises(MortalAmdError, match="batch_rows"):
            SampleStore(16, version, batch_rows=0, lib=lib)
        # truncate, then the same games again: the same bytes
        short.clear()
        assert short.count == 0 and short.grps == []
        loader.store_pool(pool, 1, 1, seats=[2], store=short)
        assert store_bytes(short) == before
        short.truncate(n1 // 2)
        assert short.meta.tobytes() == np.frombuffer(before[-n1 * 32:], dtype=np.int32).reshape(n1, 8)[:n1 // 2].tobytes()
        # a closed store
        short.close()
        for call in (lambda: short.encode([0]), lambda: short.encode_oracle([0]), lambda: short.truncate(0),
                     lambda: loader.store_pool(pool, 1, 1, store=short), short.check_overflow):
            with pytest.raises(MortalAmdError, match="SampleStore is closed"):
                call()
    finally:
        exact.close()
        short.close()


# ---- case 8
def check_size(lib):
    for version in (1, 2, 3, 4):
        store = SampleStore(8, version, batch_rows=4, lib=lib)
        try:
            assert store.bytes_per_sample == lib.mj_debug_table_size() + 36
            assert store.bytes_per_sample * 50 < OBS_ROWS[version] * 34 * 4 + 46
            assert (store.count, store.capacity) == (0, 8)
        finally:
            store.close()


# ---- the runners' routes
def check_batch_runner(oracle, pool_cls):
    """BatchRunner.sample_store after run(): the engines' names by seat, the samples of the reference loader."""
    import test_sharding as TS

    from mortal_amd import arena as AR
    from mortal_amd import mjai_log as ML

    old = AR.BatchRunner.pool_cls
    AR.BatchRunner.pool_cls = pool_cls
    try:
        seeds = [(10000, G.KEY), (10001, G.KEY)]
        aos = np.array([0b0001, 0b0100], dtype=np.uint8)
        runner = AR.BatchRunner([TS._LowestLegalEngine("a"), TS._LowestLegalEngine("b")], seeds, aos, deal_algo=0, keep_stat=True)
        try:
            runner.run()
            store = runner.sample_store(GameplayLoader(3, oracle=False, player_names=["b"]), batch_rows=24)
            try:
                logs = runner.pool.read_logs()
                assert store.wanted == [[0], [2]]
                total = 0
                for t in range(2):
                    names = ["b" if (int(aos[t]) >> s) & 1 else "a" for s in range(4)]
                    ev = [dict(type="start_game", names=names, seed=list(seeds[t]))] + ML.decode_events(logs[t]) + [dict(type="end_game")]
                    total += G.check_gameplay(oracle, store.gameplay(t, store.wanted[t][0]), ev, 3, True)
                assert total == store.count > 0
            finally:
                store.close()
        finally:
            runner.close()
    finally:
        AR.BatchRunner.pool_cls = old


def check_self_play_runner(oracle, pool_cls, n_tables=2):
    """SelfPlayRunner.sample_store over a harvest of play(): b's seats by table, the samples of the reference loader over the
    harvest's words as the host reads them."""
    import test_sharding as TS

    from mortal_amd import arena as AR
    from mortal_amd import mjai_log as ML

    old = AR.SelfPlayRunner.pool_cls
    AR.SelfPlayRunner.pool_cls = pool_cls
    try:
        aos = np.array([(0b0001, 0b0100)[t % 2] for t in range(n_tables)], dtype=np.uint8)
        runner = AR.SelfPlayRunner([TS._LowestLegalEngine("a"), TS._LowestLegalEngine("b")], n_tables, (10000, G.KEY), aos, deal_algo=0,
                                   max_games=8 * n_tables, max_words=8 * n_tables * 4096)
        try:
            h = runner.play(min_games=n_tables)
            store = None
            try:
                assert h.n_games >= n_tables and h.n_errors == 0
                store = runner.sample_store(GameplayLoader(3, oracle=False, player_names=["b"]), h, batch_rows=24)
                logs = h.read_logs()
                total = 0
                for i, r in enumerate(h.games):
                    t = int(r["table"])
                    assert store.wanted[i] == seats_of(aos[t]) and store.names[i] == ["b" if (int(aos[t]) >> s) & 1 else "a" for s in range(4)]
                    ev = [dict(type="start_game", names=store.names[i], seed=[int(r["seed_nonce"]), int(r["seed_key"])])] \
                        + ML.decode_events(logs[i]) + [dict(type="end_game")]
                    total += G.check_gameplay(oracle, store.gameplay(i, store.wanted[i][0]), ev, 3, True)
                assert total == store.count > 0
            finally:
                if store is not None:
                    store.close()
                h.close()
        finally:
            runner.close()
    finally:
        AR.SelfPlayRunner.pool_cls = old
