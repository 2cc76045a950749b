"""libriichi.dataset: `Grp` (dataset/grp.rs) and `GameplayLoader` / `Gameplay` (dataset/gameplay.rs) on the MI355X pool.

`Grp` is a host-side reduction of the event stream.  `GameplayLoader` replays whole batches of logs on the device:
one table per log, every seat's PlayerState advanced by the step kernel's event handlers (`mj_k_replay`), and every
decision of a wanted seat encoded by the arena's obs/mask kernels — obs, mask, label and bookkeeping are the
reference's (gameplay.rs:239-443), produced for all logs of a batch at once instead of one rayon task per player.

`oracle=True` adds the invisible obs of dataset/invisible.rs: the wall of every kyoku is either rebuilt on the device from
the game's seed (`trust_seed=True`, logs written by this engine / the reference arena) or reconstructed from the log with
the never-seen tiles filled in at random — like the reference, that filler is not reproducible.
"""
import gzip
import json

import numpy as np

from . import _lib, mjai_log
from .pool import OBS_ROWS, TablePool

GRP_SIZE = 7


def _read_gz(path):
    with gzip.open(path, "rt") as f:
        return f.read()


def _parse(raw_log):
    try:
        return [json.loads(l) for l in raw_log.splitlines() if l.strip()]
    except json.JSONDecodeError as ex:
        raise ValueError(f"failed to parse log: {ex}") from ex


class Grp:
    """dataset/grp.rs:20-165: per-kyoku [grand_kyoku, honba, kyotaku, scores/10000 x4] (f64), final ranks and scores."""

    def __init__(self, feature=None, rank_by_player=(0, 0, 0, 0), final_scores=(0, 0, 0, 0)):
        self.feature = np.zeros((0, GRP_SIZE), dtype=np.float64) if feature is None else feature
        self.rank_by_player = list(rank_by_player)
        self.final_scores = list(final_scores)

    @staticmethod
    def load_events(events):
        game_info = []
        rank_by_player = None
        final_deltas = [0, 0, 0, 0]
        final_scores = [0, 0, 0, 0]
        for ev in reversed(events):
            t = ev["type"]
            if t in ("hora", "ryukyoku"):
                if rank_by_player is None:
                    ds = ev.get("deltas")
                    if ds is None:
                        raise ValueError("invalid log: field `deltas` is required for Hora and Ryukyoku of AL")
                    final_deltas = [a + b for a, b in zip(final_deltas, ds)]
            elif t == "reach_accepted":
                if rank_by_player is None:
                    final_deltas[ev["actor"]] -= 1000
            elif t == "start_kyoku":
                if rank_by_player is None:
                    final_scores = [a + b for a, b in zip(ev["scores"], final_deltas)]
                    order = sorted(range(4), key=lambda i: -final_scores[i])  # Rankings::new (stable)
                    total = sum(final_scores)
                    if total < 100_000:  # assume the sum of scores to be 100k
                        final_scores[order[0]] += 100_000 - total
                    rank_by_player = [0] * 4
                    for r, pid in enumerate(order):
                        rank_by_player[pid] = r
                kyoku = ev["kyoku"]
                grand = {"E": kyoku - 1, "S": 3 + kyoku}.get(ev["bakaze"], 7 + kyoku)
                game_info.insert(0, [float(grand), float(ev["honba"]), float(ev["kyotaku"])]
                                 + [s / 10000.0 for s in ev["scores"]])
        if rank_by_player is None:
            raise ValueError("invalid log: no Hora or Ryukyoku after a StartKyoku")
        return Grp(np.array(game_info, dtype=np.float64).reshape(len(game_info), GRP_SIZE), rank_by_player, final_scores)

    @staticmethod
    def from_packed(words_list, max_kyoku=64, lib=None):
        """The same from packed event words (mjai_log.encode_events, TablePool.read_logs), every log of the list reduced on the
        device (mj_grp_logs) -> list of Grp.  ValueError for a log load_events would refuse (no start_kyoku), a malformed one
        or one of more than max_kyoku kyoku."""
        grps, _n_kyoku, _counts = grp_logs(words_list, max_kyoku, lib)
        for i, g in enumerate(grps):
            if g is None:
                raise ValueError(f"log {i}: invalid log (empty, malformed, no StartKyoku or more than {max_kyoku} kyoku)")
        return grps

    @staticmethod
    def load_log(raw_log):
        return Grp.load_events(_parse(raw_log))

    @staticmethod
    def load_gz_log_files(gzip_filenames):
        out = []
        for f in gzip_filenames:
            try:
                out.append(Grp.load_log(_read_gz(f)))
            except Exception as ex:
                raise RuntimeError(f"error when reading {f}: {ex}") from ex
        return out

    def __len__(self):
        return self.feature.shape[0]

    def take_feature(self):
        f, self.feature = self.feature, np.zeros((0, GRP_SIZE), dtype=np.float64)
        return f

    def take_rank_by_player(self):
        return list(self.rank_by_player)

    def take_final_scores(self):
        return list(self.final_scores)


def _grp_call(L, fn, head, n, max_kyoku, unit=None, first=0):
    """Shared by grp_logs, TablePool.log_grp and Harvest.grp: allocate the outputs, run `fn(*head, n, max_kyoku, feat ptr,
    n_kyoku ptr, rank ptr, final ptr, counts ptr, stream)` of library L and check it, wrap the result -> (list of Grp or None
    per log, n_kyoku int32 [n], counts dict).  unit ("table" / "game"): a malformed log is a ValueError that names log first + i."""
    n_logs, max_kyoku = max(int(n), 0), int(max_kyoku)  # (a negative n is the library's to refuse)
    feat = np.zeros((n_logs, max_kyoku, GRP_SIZE), dtype=np.int32)
    n_kyoku = np.zeros(n_logs, dtype=np.int32)
    rank = np.zeros((n_logs, 4), dtype=np.int32)
    final = np.zeros((n_logs, 4), dtype=np.int32)
    counts = np.zeros(3, dtype=np.int64)
    L.check(fn(*head, int(n), max_kyoku, feat.ctypes.data, n_kyoku.ctypes.data, rank.ctypes.data, final.ctypes.data,
               counts.ctypes.data, L.stream()))
    bad = np.flatnonzero(n_kyoku < 0)
    if unit and len(bad):
        raise ValueError(f"{unit} {first + int(bad[0])}: malformed event log (or more than {max_kyoku} kyoku)")
    grps = []
    for i in range(n_logs):
        k = int(n_kyoku[i])
        if k <= 0:
            grps.append(None)
            continue
        f = feat[i, :k].astype(np.float64)
        f[:, 3:] = feat[i, :k, 3:].astype(np.float64) / 10000.0  # grp.rs:144 `score as f64 / 10000.`
        grps.append(Grp(f, [int(x) for x in rank[i]], [int(x) for x in final[i]]))
    return grps, n_kyoku, dict(reduced=int(counts[0]), skipped=int(counts[1]), malformed=int(counts[2]))


def grp_logs(words_list, max_kyoku=64, lib=None):
    """`Grp.load_events` of every log on the device, from packed event words (mjai_log.encode_events, TablePool.read_logs;
    mj_grp_logs).  -> (list of Grp, None for an empty or malformed log; n_kyoku int32 [n]: 0 for an empty log, -1 for a malformed
    one -- no start_kyoku, more than max_kyoku of them, an unknown event or a chain that runs past the end; counts
    dict(reduced, skipped, malformed)).  `lib` is for the test suite (the host emulation of the same sources)."""
    L = lib or _lib.lib
    words, off, n = mjai_log.pack_logs(words_list, "grp_logs")
    return _grp_call(L, L.mj_grp_logs, (words.ctypes.data, off.ctypes.data), n, max_kyoku)


class Gameplay:
    """One player's samples of one game (gameplay.rs:46-64).  The `take_*` methods hand the per-move lists over like
    the reference's; the same data stays available as stacked device tensors (`obs_dev`, `masks_dev`) for consumers
    that batch on the GPU anyway (mortal/dataloader.py stacks them right after)."""

    def __init__(self, player_id, player_name, grp):
        self.player_id = player_id
        self.player_name = player_name
        self.grp = grp
        self.obs_dev = None
        self.masks_dev = None
        self.invisible_obs = []
        self.actions = []
        self.at_kyoku = []
        self.dones = []
        self.apply_gamma = []
        self.at_turns = []
        self.shantens = []

    def _take_list(self, name):
        v = getattr(self, name)
        setattr(self, name, [])
        return v

    def take_obs(self):
        t, self.obs_dev = self.obs_dev, None
        return [] if t is None else list(t.cpu().numpy())

    def take_masks(self):
        t, self.masks_dev = self.masks_dev, None
        return [] if t is None else list(t.cpu().numpy())

    def take_invisible_obs(self):
        return self._take_list("invisible_obs")

    def take_actions(self):
        return self._take_list("actions")

    def take_at_kyoku(self):
        return self._take_list("at_kyoku")

    def take_dones(self):
        return self._take_list("dones")

    def take_apply_gamma(self):
        return self._take_list("apply_gamma")

    def take_at_turns(self):
        return self._take_list("at_turns")

    def take_shantens(self):
        return self._take_list("shantens")

    def take_grp(self):
        g, self.grp = self.grp, Grp()
        return g

    def take_player_id(self):
        return self.player_id


class GameplayLoader:
    """dataset/gameplay.rs:21-165."""

    pool_cls = TablePool  # the test suite substitutes the host emulation of the same kernels (tests/host/emu_pool.py)

    def __init__(self, version, *, oracle=True, player_names=None, excludes=None, trust_seed=False,
                 always_include_kan_select=True, augmented=False, device="cuda:0", deal_algo=None):
        if version not in OBS_ROWS:
            raise ValueError(f"unsupported obs version {version}")
        self.version = version
        self.oracle = bool(oracle)
        self.player_names = list(player_names or [])
        self.excludes = list(excludes or [])
        self.trust_seed = bool(trust_seed)
        self.always_include_kan_select = bool(always_include_kan_select)
        self.augmented = bool(augmented)
        self.device = device
        # trust_seed: wall shuffle tried first when rebuilding a kyoku from its seed (None = pool.default_deal_algo());
        # the replay kernel falls back to the other rand generation before reporting MJ_ERR_WALL
        self.deal_algo = deal_algo
        # oracle + trust_seed + augmented: the reference augments the events but deals the invisible wall from the seed as it
        # was (gameplay.rs:126-164, invisible.rs:36-71); the replay kernel does the same (LG_SK_AUG_BIT)

    def __repr__(self):
        return (f"GameplayLoader {{ version: {self.version}, oracle: {self.oracle}, player_names: {self.player_names}, "
                f"excludes: {self.excludes}, trust_seed: {self.trust_seed}, "
                f"always_include_kan_select: {self.always_include_kan_select}, augmented: {self.augmented} }}")

    # ---- the reference's entry points
    def load_log(self, raw_log):
        return self.load_logs([raw_log])[0]

    def load_gz_log_files(self, gzip_filenames):
        raws = []
        for f in gzip_filenames:
            try:
                raws.append(_read_gz(f))
            except Exception as ex:
                raise RuntimeError(f"error when reading {f}: {ex}") from ex
        return self.load_logs(raws)

    def _wanted(self, names):
        ps, ex = set(self.player_names), set(self.excludes)
        out = []
        for i, name in enumerate(names):
            if ps:
                keep = name in ps
            elif ex:
                keep = name not in ex
            else:
                keep = True
            if keep:
                out.append(i)
        return out

    @staticmethod
    def _walls_from_events(events, augmented, rng):
        """Invisible::new without a seed (invisible.rs:24-149): per kyoku the 136-tile wall in the pool's layout —
        haipai 0..51, rinshan 52..55 (popped from the back), dora indicators 56..60 (back first), ura 61..65, yama 66..135
        (popped from the back) — known tiles from the log, the rest drawn at random from the unseen tiles."""
        tid = (lambda n: mjai_log.augment_tile_id(mjai_log.TILE_ID[n])) if augmented else (lambda n: mjai_log.TILE_ID[n])
        walls = []
        cur = None

        def fresh():
            unknown = [4] * 37
            for t in (4, 13, 22):
                unknown[t] = 3
            unknown[34] = unknown[35] = unknown[36] = 1
            return dict(hai=[], yama=[], rinshan=[], dora=[], ura=[], unknown=unknown, from_rinshan=False, ura_done=False)

        for ev in events:
            t = ev["type"]
            if t == "start_kyoku":
                cur = fresh()
                cur["dora"].append(tid(ev["dora_marker"]))
                cur["unknown"][cur["dora"][0]] -= 1
                for hand in ev["tehais"]:
                    for x in hand:
                        cur["hai"].append(tid(x))
                        cur["unknown"][tid(x)] -= 1
            elif cur is None:
                continue
            elif t == "tsumo":
                p = tid(ev["pai"])
                if cur["from_rinshan"]:
                    cur["rinshan"].append(p)
                    cur["from_rinshan"] = False
                else:
                    cur["yama"].append(p)
                cur["unknown"][p] -= 1
            elif t in ("ankan", "kakan", "daiminkan"):
                cur["from_rinshan"] = True
            elif t == "dora":
                cur["dora"].append(tid(ev["dora_marker"]))
                cur["unknown"][cur["dora"][-1]] -= 1
            elif t == "hora" and ev.get("ura_markers") is not None and not cur["ura_done"]:
                for x in ev["ura_markers"]:
                    cur["ura"].append(tid(x))
                    cur["unknown"][tid(x)] -= 1
                cur["ura_done"] = True
            elif t == "end_kyoku":
                if min(cur["unknown"]) < 0:
                    raise ValueError("invalid log: more than four copies of a tile")
                filler = [k for k, c in enumerate(cur["unknown"]) for _ in range(c)]
                rng.shuffle(filler)
                for key, size in (("yama", 70), ("rinshan", 4), ("dora", 5), ("ura", 5)):
                    while len(cur[key]) < size:
                        cur[key].append(filler.pop())
                assert not filler
                wall = [0] * 136
                wall[:52] = cur["hai"]
                for k in range(4):
                    wall[52 + 3 - k] = cur["rinshan"][k]
                for k in range(5):
                    wall[56 + 4 - k] = cur["dora"][k]
                    wall[61 + k] = cur["ura"][k]
                for k in range(70):
                    wall[66 + 69 - k] = cur["yama"][k]
                walls.append(wall)
                cur = None
        return walls

    def load_logs(self, raw_logs):
        """Batch entry point: list of raw log texts -> list (per log) of lists of Gameplay (one per wanted player)."""
        games = []
        for raw in raw_logs:
            events = _parse(raw)
            if not events or events[0].get("type") != "start_game":
                raise ValueError("empty or invalid game log")
            names = events[0].get("names", ["", "", "", ""])
            wanted = self._wanted(names)
            games.append(dict(events=events, names=names, wanted=wanted, grp=Grp.load_events(events)))
        n = len(games)
        if n == 0:
            return []
        nonces = keys = None
        if not self.oracle:
            scripts = [mjai_log.encode_events(g["events"], augmented=self.augmented) for g in games]
        else:
            rng = np.random.default_rng()
            seeds = [g["events"][0].get("seed") if self.trust_seed else None for g in games]
            nonces = np.array([s[0] if s else 0 for s in seeds], dtype=np.uint64)
            keys = np.array([s[1] if s else 0 for s in seeds], dtype=np.uint64)
            scripts = []
            for g, seed in zip(games, seeds):
                if seed:  # the game was emulated by this engine: use the seed directly (invisible.rs:36-71)
                    scripts.append(mjai_log.encode_events(g["events"], augmented=self.augmented, deal_from_seed=True))
                else:
                    walls = self._walls_from_events(g["events"], self.augmented, rng)
                    scripts.append(mjai_log.encode_events(g["events"], augmented=self.augmented, walls=walls))
        tracked = [sum(1 << p for p in g["wanted"]) for g in games]

        def fill(store):
            self._replay(store, self.pool_cls, self.device, self.deal_algo, n, lambda rp: rp.replay_load(
                scripts, tracked, self.always_include_kan_select, nonces, keys), sum(len(g["events"]) for g in games) + 8)

        return self._load(games, tracked, [len(s) for s in scripts], self.device, self.pool_cls._L, fill)

    def load_pool(self, pool, table0=0, n_tables=None, seats=None, names=None, augmented=False):
        """The samples of a pool's finished games straight from its device log (TablePool.enable_log), without JSON or files:
        tables [table0, table0 + n_tables) (None = to the last) are replayed on the device from the packed words the arena wrote
        (mj_replay_load_pool), and their Grp is reduced from the same words (mj_pool_grp).  Returns what load_logs returns for the
        same games: a list per table of Gameplay, one per wanted seat; the list of a table that is still playing or ended in
        error is empty.

        seats: 4-bit seat mask per table (None = all four seats); names: four player names per table (None = ""), filtered by
        player_names / excludes like the names of a log file when given.  oracle=True rebuilds every wall from the table's
        seed -- logs of this engine always come with their seed, trust_seed does not matter here.

        augmented=True gives the samples of the suit-swapped game (manzu <-> pinzu, gameplay.rs:126-128): the device swaps the tiles
        while it copies the log into the replay script, the pool's log stays as it is.  The keyword is per call: the reference builds
        one loader per pass over its files (mortal/dataloader.py: augmented False, then True), a pool is one object in memory that
        is read in both forms -- the two passes are two calls on one loader.  Grp holds no tile and is the same in both.  With
        oracle=True the invisible obs follows the reference's mix, as load_logs does: events swapped, wall as the seed deals it.
        A loader constructed with augmented=True is refused here (ValueError): pass the keyword instead.

        Memory: all obs of the range are materialised on the device at once (137 KB per obs-v4 sample, about 220 samples per
        game and seat), so the caller bounds memory by the table range it asks for.  At the peak that one copy, written in the
        reference's order, is resident beside the records of the replay, 2,148 B for each of sample_bound's samples: 1.9 GB
        beside 7.2 GB of obs v3 for all seats of 64 self-play games, 10.5 beside 29.5 GB for one seat of 1,024.  (Until the
        loaders went through the store, the obs of the replay steps, their concatenation and then its reordered copy were
        resident two at a time: 14.3 and 59.1 GB.)"""
        return self._load_device(pool, table0, n_tables, seats, names, augmented)

    def load_harvest(self, harvest, game0=0, n_games=None, seats=None, names=None, augmented=False):
        """The samples of the games a pool in refill mode has collected (TablePool.take_harvest), with the contract of load_pool:
        games [game0, game0 + n_games) of the harvest's sorted order (None = to the last) are replayed on the device from the
        collected words (mj_replay_load_harvest), their Grp reduced from the same words (mj_harvest_grp).  Returns a list per game
        of Gameplay, one per wanted seat; the list of a game that ended in error is empty.  seats / names as load_pool.
        oracle=True deals every wall from the seed recorded with the game.  augmented as in load_pool: per call, swapped on the
        device on the way into the script."""
        harvest._handle()  # (a closed Harvest is refused before anything else)
        return self._load_device(harvest, game0, n_games, seats, names, augmented)

    def store_pool(self, pool, table0=0, n_tables=None, seats=None, names=None, augmented=False, store=None, capacity=None,
                   batch_rows=1024):
        """load_pool into a SampleStore (mortal_amd/samples.py): the same tables, refusals, seat / name / skip semantics and
        `augmented` keyword, but every decision is kept as its 2 KB record instead of its obs, and no encoder or SP kernel runs
        until a batch is drawn (store.encode).  -> the store.

        store: append to this store (its games are numbered on from len(store.grps)) -- how successive pools or harvests fill one
        buffer; None: a new one of `capacity` samples (default 4,096 per table of the call) and `batch_rows` rows per encode launch.
        On any failure -- the capacity, an illegal log -- the caller's store is back at its count and games on entry.  With
        oracle=True the walls are dealt from the seeds and store.encode_oracle gives the invisible obs."""
        return self._store_device(pool, table0, n_tables, seats, names, augmented, store, capacity, batch_rows)

    def store_harvest(self, harvest, game0=0, n_games=None, seats=None, names=None, augmented=False, store=None, capacity=None,
                      batch_rows=1024):
        """load_harvest into a SampleStore, as store_pool: games [game0, game0 + n_games) of the harvest's sorted order."""
        harvest._handle()
        return self._store_device(harvest, game0, n_games, seats, names, augmented, store, capacity, batch_rows)

    def _device_games(self, who, src, first, count, seats, names):
        """What load_* and store_* check and prepare: logs [first, first + count) of a device source -> (n, per log dict(names,
        wanted, grp), tracked seat masks).  `src` is a TablePool or a Harvest: n_logs, log_units / log_where (what the messages
        call it), pool_cls, device, deal_algo, log_cap, log_words(first, n), grp(first, n) -> the Grps (None = skipped)."""
        unit, where, n_src = src.log_units, src.log_where, src.n_logs
        if self.augmented:
            raise ValueError(f"{who}: a loader constructed with augmented=True is not accepted here (a pool or a harvest is read in "
                             f"both forms by one loader): construct it without and pass {who}(..., augmented=True) per call")
        n = n_src - first if count is None else int(count)
        if first < 0 or n < 0 or first + n > n_src:
            raise ValueError(f"{who}: {unit} [{first}, {first + n}) are not in a {where} of {n_src}")
        if n == 0:
            return 0, [], []
        masks = np.full(n, 15, dtype=np.uint8) if seats is None else np.ascontiguousarray(seats, dtype=np.uint8)
        if masks.shape != (n,):
            raise ValueError(f"seats: expected {n} masks, got shape {masks.shape}")
        if names is not None and len(names) != n:
            raise ValueError(f"names: expected {n} lists of four names, got {len(names)}")
        grps = src.grp(first, n)
        games = []
        for t in range(n):
            nm = list(names[t]) if names is not None else ["", "", "", ""]
            wanted = [p for p in (self._wanted(nm) if names is not None else range(4)) if (int(masks[t]) >> p) & 1]
            games.append(dict(names=nm, wanted=wanted if grps[t] is not None else [], grp=grps[t]))
        return n, games, [sum(1 << p for p in g["wanted"]) for g in games]

    def _replay(self, store, pool_cls, device, deal_algo, n, load, max_steps, first=0):
        """The one way from logs to samples: a replay pool of n tables takes its scripts from `load(pool)`, and every decision of
        every step becomes a record of `store`, its games numbered on from len(store.grps).  first = what the messages call the
        pool's table 0."""
        rp = pool_cls(n, version=self.version, device=device, max_rows=8 * n + 64, deal_algo=deal_algo)
        try:
            load(rp)
            game0 = len(store.grps)
            for _ in range(max_steps):
                if rp.replay_step():
                    store.append(rp, game0)
                elif rp.counters()["games"] >= n:
                    break
            else:
                raise RuntimeError("log replay did not terminate")
            code, tbl = rp.first_error()
            if code:
                raise ValueError(f"log {first + tbl}: the event stream is not a legal game (error code {code})")
        finally:
            rp.close()

    def _replay_device(self, store, src, first, n, tracked, augmented):
        """_replay of logs [first, first + n) of a device source (TablePool.replay_load_pool / replay_load_harvest)."""
        def load(rp):
            getattr(rp, f"replay_load_{src.log_where}")(src, first, tracked, self.always_include_kan_select,
                                                        deal_from_seed=self.oracle, augmented=augmented)
        # every step applies at least one event of every unfinished log, and an event takes at least one word
        self._replay(store, src.pool_cls, str(src.device), src.deal_algo, n, load, src.log_cap + 8, first)

    def _load(self, games, tracked, words, device, lib, fill):
        """load_logs / load_pool / load_harvest: `fill(store)` replays the games into a store of this call's own, sized by
        sample_bound and so never refused for its size; its Gameplays, encoded once and in the reference's order, are all that
        is left of it."""
        from .samples import MAX_CAPACITY, SampleStore

        store = SampleStore(min(max(sample_bound(tracked, words), 1), MAX_CAPACITY), self.version,
                            batch_rows=load_batch_rows(len(games)), device=device, lib=lib)
        try:
            fill(store)
            store._add_games(games, self.oracle)
            out = store.gameplays(invisible=self.oracle)
            store.check_overflow(RuntimeError("obs v4: a sample's single-player state graph exceeded the device scratch capacity"))
            return out
        finally:
            store.close()

    def _load_device(self, src, first, count, seats, names, augmented):
        """load_pool / load_harvest: logs [first, first + count) of a device source -> the Gameplays."""
        n, games, tracked = self._device_games(f"load_{src.log_where}", src, first, count, seats, names)
        if n == 0:
            return []
        return self._load(games, tracked, src.log_words(first, n), str(src.device), src._L,
                          lambda store: self._replay_device(store, src, first, n, tracked, augmented))

    def _store_device(self, src, first, count, seats, names, augmented, store, capacity, batch_rows):
        """store_pool / store_harvest: _load_device into the caller's store, or a new one that is handed over."""
        from .samples import SampleStore

        who = f"store_{src.log_where}"
        n, games, tracked = self._device_games(who, src, first, count, seats, names)
        own = store is None
        if own:
            store = SampleStore(4096 * max(n, 1) if capacity is None else capacity, self.version, batch_rows=batch_rows,
                                device=str(src.device), lib=src._L)
        else:
            store._handle()
            if store.version != self.version or store._L is not src._L:
                raise ValueError(f"{who}: the store holds obs v{store.version} samples of "
                                 f"{'another' if store._L is not src._L else 'the same'} library, the loader reads v{self.version}")
        mark = store._mark()
        try:
            if n:
                self._replay_device(store, src, first, n, tracked, augmented)
            store._add_games(games, self.oracle)
        except BaseException:
            store.close() if own else store._rollback(mark)
            raise
        return store


def load_batch_rows(n):
    """Rows per encode launch of the store behind a load_* of n games.  For obs v4 the encode context sizes the SP work areas
    (mj_capi.hip sp_setup: min(1024, r) + spare + wide areas of 8.1 MB, spare = max(8, t / 4) rounded down to even, at most
    512, wide = max(2, t / 16), at most 256) from its t = r = batch_rows, where the replay pool of a load sized them from
    t = n, r = 8 n + 64.  This rule never takes more areas than that did: 69 for 82 at n = 1, 567 for 596 at n = 64, 850 for
    894 at n = 100, and from n = 120 on 1,008 for 1,061 and more."""
    return min(768, 6 * n + 48)


def sample_bound(tracked, words):
    """The most samples a replay can give: tracked = the 4-bit seat mask of every log, words = its length in script words.
    mj_k_replay gives rows only after it applied an event, every event is at least one word, and an applied event gives a tracked
    seat that can act one main row and at most one kan-select row.  Every event handler first clears all four seats' `cans`
    (ev_prologue) and then sets them for the actor alone (tsumo, chi / pon, reach) or for the other three (dahai, the chankan of
    kakan): at most min(tracked seats, 3) seats act, whatever the words say, so a log gives at most 2 * min(popcount(tracked), 3)
    samples per word.  (A legal game stays within min(4, popcount + 1) per event, since only the seat that declares the kan gets
    a select row -- tests/loader_cases.py counts that on the reference's side.  The replay labels an event before it knows whether
    the next one is legal: behind a discard, a kakan or ankan word would give every caller a select row, hence the wider bound.)"""
    return sum(2 * min(bin(int(t)).count("1"), 3) * int(w) for t, w in zip(tracked, words))
