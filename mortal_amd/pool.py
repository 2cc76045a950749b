"""TablePool: the SoA pool of concurrent tables in HBM, driven through the C-ABI (include/mortal_amd.h).

PyTorch is used only for device memory and the HIP stream; all compute is in libmortal_amd.so.
Reference counterpart: `BatchGame::run` (libriichi/src/arena/game.rs:230-316).
"""
import ctypes as C

import numpy as np
import torch

from . import tables
from ._lib import MortalAmdError, lib

OBS_ROWS = {1: 938, 2: 942, 3: 934, 4: 1012}
ACTION_SPACE = 46
DEAL_RAND08, DEAL_RAND09 = 0, 1  # include/mortal_amd.h MJ_DEAL_*


def default_deal_algo():
    """The wall shuffle of `Board::init_from_seed` (arena/board.rs:99-109) depends on the `rand` crate generation.
    Default = rand 0.9.1, the version the reference's Cargo.lock pins (Cargo.lock:1042-1043), so the same (seed, key)
    gives today's reference's games; MORTAL_AMD_DEAL_ALGO=rand08 selects the older Fisher-Yates (the shuffle of the
    reference's published example log)."""
    import os

    v = os.environ.get("MORTAL_AMD_DEAL_ALGO", "rand09").strip().lower()
    if v in ("0", "rand08", "rand0.8", "0.8"):
        return DEAL_RAND08
    if v in ("1", "rand09", "rand0.9", "0.9", "0.9.1"):
        return DEAL_RAND09
    raise ValueError(f"MORTAL_AMD_DEAL_ALGO={v!r}: expected rand08 or rand09")

_tables_ready = False


def _ensure_tables():
    global _tables_ready
    if not _tables_ready:
        p = tables.payload()
        lib.check(lib.mj_tables_upload(p, len(p)))
        _tables_ready = True


def _load_flags(deal_from_seed, augmented):
    """include/mortal_amd.h MJ_LOAD_DEAL_FROM_SEED | MJ_LOAD_AUGMENT"""
    return (1 if deal_from_seed else 0) | (2 if augmented else 0)


# include/mortal_amd.h MjHarvestGame
HARVEST_GAME_DTYPE = np.dtype([("seed_nonce", "<u8"), ("seed_key", "<u8"), ("first_word", "<u8"), ("n_words", "<u4"),
                               ("game_id", "<u4"), ("table", "<u4"), ("cycle", "<u4"), ("scores", "<i4", (4,)), ("err", "u1"),
                               ("agent_of_seat", "u1"), ("reserved", "u1", (6,))])
assert HARVEST_GAME_DTYPE.itemsize == 64


class Harvest:
    """The finished games a pool in refill mode has collected (TablePool.take_harvest): what the reference's arena returns as
    a list of GameResult (arena/game.rs:291-296, arena/result.rs:19-51), kept on the device.  It owns its device memory and is
    independent of the pool from then on: later steps and later takes do not change it.

    n_games / n_words / dropped (games that found the buffer full while it was the pool's active one) / n_errors;
    games: structured array of the records (HARVEST_GAME_DTYPE), sorted by (game_id, table) -- "game i" is row i."""

    log_units, log_where, _src_name = "games", "harvest", "a Harvest"  # what messages call this source (as TablePool's)
    n_logs = property(lambda s: s.n_games)

    def __init__(self, pool, handle):
        L = self._L = pool._L
        self.pool_cls = type(pool)
        self.device = pool.device
        self.deal_algo = pool.deal_algo
        self.log_cap = pool.log_cap
        self.h = handle
        info = np.zeros(4, dtype=np.int64)
        L.check(L.mj_harvest_info(self.h, info.ctypes.data))
        self.n_games, self.n_words, self.dropped, self.n_errors = (int(x) for x in info)
        self.games = np.zeros(self.n_games, dtype=HARVEST_GAME_DTYPE)
        L.check(L.mj_harvest_games(self.h, self.games.ctypes.data if self.n_games else None))

    def __len__(self):
        return self.n_games

    def close(self):
        if getattr(self, "h", None):
            self._L.mj_harvest_destroy(self.h)
            self.h = None

    __del__ = close

    def _handle(self):
        if not getattr(self, "h", None):
            raise MortalAmdError("the Harvest is closed")
        return self.h

    def read_logs(self):
        """-> list (one per game) of uint64 arrays: the event words of the game, as TablePool.read_logs returned them for its
        table before the restart (empty for a game in error)."""
        h = self._handle()
        out = []
        for i in range(self.n_games):
            buf = np.empty(int(self.games["n_words"][i]), dtype=np.uint64)
            self._L.check(self._L.mj_harvest_read(h, i, buf.ctypes.data if len(buf) else None))
            out.append(buf)
        return out

    def stat(self, seats=None, per_seat=False):
        """libriichi's Stat of the collected games, reduced on the device (mj_harvest_stat) -> what TablePool.log_stat returns:
        (totals [Stat of agent 0's seats, Stat of agent 1's seats], per-seat int64 [n_games, 4, 44] or None, counts); a game in
        error is skipped."""
        from .stat import _stat_call

        return _stat_call(self._L, self._L.mj_harvest_stat, (self._handle(),), self.n_games, seats, per_seat)

    def grp(self, game0=0, n=None, max_kyoku=64):
        """dataset/grp.rs `Grp` of games [game0, game0 + n) (n None = to the last), reduced on the device (mj_harvest_grp), as
        TablePool.log_grp: None for a game in error, ValueError for a malformed log."""
        from .dataset import _grp_call

        n = self.n_games - game0 if n is None else n
        return _grp_call(self._L, self._L.mj_harvest_grp, (self._handle(), int(game0)), n, max_kyoku, "game", game0)[0]

    def log_words(self, first, n):
        return self.games["n_words"][first:first + n]


class TablePool:
    _L = lib  # the C-ABI library (tests/host/emu_pool.py substitutes the host emulation of the same sources)

    def _stream(self):
        return self._L.stream()

    def _bind_device(self, device):
        if not torch.cuda.is_available():
            raise MortalAmdError("TablePool needs a HIP device (torch.cuda.is_available() is False)")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        _ensure_tables()

    def __init__(self, n_tables, version=4, deal_algo=None, device="cuda:0", max_rows=0):
        self._bind_device(device)
        self.n_tables = n_tables
        self.version = version
        self.C = OBS_ROWS[version]
        self.max_rows = max_rows or 8 * n_tables
        self.deal_algo = default_deal_algo() if deal_algo is None else int(deal_algo)
        self.h = self._L.check(self._L.mj_pool_create(n_tables, version, self.deal_algo, self.max_rows))
        self.n_rows = [0, 0]
        self.n_games_total = n_tables
        self.versions = [version, version]

    def close(self):
        if getattr(self, "h", None):
            self._L.mj_pool_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self, seeds, game_ids=None, agent_of_seat=None, n_games_total=None):
        """seeds: list of (nonce, key) per table; agent_of_seat: uint8 per table, bit s = agent of seat s."""
        assert len(seeds) == self.n_tables
        nonces = np.ascontiguousarray([s[0] for s in seeds], dtype=np.uint64)
        keys = np.ascontiguousarray([s[1] for s in seeds], dtype=np.uint64)
        gid = np.ascontiguousarray(game_ids if game_ids is not None else np.arange(self.n_tables), dtype=np.uint32)
        aos = np.ascontiguousarray(agent_of_seat if agent_of_seat is not None else np.zeros(self.n_tables),
                                   dtype=np.uint8)
        self.n_games_total = int(n_games_total or (int(gid.max()) + 1))
        self._L.check(self._L.mj_pool_reset(self.h, nonces.ctypes.data, keys.ctypes.data, gid.ctypes.data, aos.ctypes.data,
                                            self.n_games_total))
        self.n_rows = [0, 0]

    def configure(self, agent, enable_quick_eval=True, enable_rule_based_agari_guard=False, version=0):
        self._L.check(self._L.mj_pool_configure(self.h, agent, int(version), int(enable_quick_eval),
                                                int(enable_rule_based_agari_guard)))
        if version:
            self.versions[agent] = version

    def enable_log(self, words_per_table=16384):
        """Turn the per-table mjai event log on (call before reset/step).  16384 words cover ~60 kyoku."""
        self._L.check(self._L.mj_pool_enable_log(self.h, int(words_per_table)))
        self.log_cap = int(words_per_table)

    def log_lengths(self):
        """-> uint32 array [n_tables]: the words each table has logged so far (more than log_cap: that log has overflowed)."""
        lens = np.zeros(self.n_tables, dtype=np.uint32)
        self._L.check(self._L.mj_log_lengths(self.h, lens.ctypes.data, self._L.stream()))
        return lens

    def _read_logs(self, table0, lens):
        """The logs of tables [table0, table0 + len(lens)), cut to the lengths log_lengths gave for them."""
        over = np.flatnonzero(lens > self.log_cap)
        if len(over):
            raise MortalAmdError(f"event log overflow on table {table0 + int(over[0])}")
        buf = np.empty((len(lens), self.log_cap), dtype=np.uint64)
        self._L.check(self._L.mj_log_read(self.h, int(table0), len(lens), buf.ctypes.data, self._L.stream()))
        return [buf[i, :n].copy() for i, n in enumerate(lens)]

    def read_log(self, table, n_words=None):
        """-> uint64 array: the event words of one table (n_words: its length, when the caller has it from log_lengths)."""
        n = self.log_lengths()[table] if n_words is None else n_words
        return self._read_logs(table, np.array([n], dtype=np.uint32))[0]

    def read_logs(self, chunk=1024):
        """-> list (one per table) of uint64 arrays holding the event words logged so far."""
        lens = self.log_lengths()
        out = []
        for t0 in range(0, self.n_tables, chunk):
            out += self._read_logs(t0, lens[t0:t0 + chunk])
        return out

    def log_stat(self, seats=None, per_seat=False):
        """libriichi's Stat of every finished game, reduced from the device log in place (mj_pool_stat; needs enable_log).
        seats: 4-bit mask per table (None = all).  -> (totals [Stat of agent 0's seats, Stat of agent 1's seats], per-seat
        int64 array [n_tables, 4, 44] or None, counts dict(reduced, skipped, malformed)), as stat.stat_logs; tables still
        playing or in error are skipped."""
        from .stat import _stat_call

        return _stat_call(self._L, self._L.mj_pool_stat, (self.h,), self.n_tables, seats, per_seat)

    def log_grp(self, table0=0, n=None, max_kyoku=64):
        """dataset/grp.rs `Grp` of tables [table0, table0 + n) (n None = to the last), reduced from the device log in place
        (mj_pool_grp; needs enable_log).  -> list of Grp, None for a table that is still playing or in error; ValueError for a
        table whose log is malformed (or holds more than max_kyoku kyoku)."""
        from .dataset import _grp_call

        n = self.n_tables - table0 if n is None else n
        return _grp_call(self._L, self._L.mj_pool_grp, (self.h, int(table0)), n, max_kyoku, "table", table0)[0]

    # ---- what a source of finished games shows GameplayLoader and replay_load_*: Harvest has the same names, over its games
    log_units, log_where, _src_name = "tables", "pool", "a pool"
    n_logs = property(lambda s: s.n_tables)
    pool_cls = property(lambda s: type(s))

    def grp(self, first=0, n=None, max_kyoku=64):
        return self.log_grp(first, n, max_kyoku)

    def log_words(self, first, n):
        """The script words logs [first, first + n) have at most: mj_k_log_pack copies a log at its own length, never past log_cap."""
        return np.minimum(self.log_lengths()[first:first + n], self.log_cap)

    def _handle(self):
        return self.h

    # ---- log replay (dataset loader)
    def replay_load(self, scripts, tracked, always_include_kan_select=True, nonces=None, keys=None):
        """scripts: one uint64 word array per table (mjai_log.encode_events); tracked: 4-bit seat mask per table;
        nonces / keys: per-table game seeds for scripts that ask the device to rebuild the wall (trust_seed)."""
        assert len(scripts) == self.n_tables
        off = np.zeros(len(scripts) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(x) for x in scripts])
        script = np.ascontiguousarray(np.concatenate(scripts) if len(scripts) else np.zeros(0), dtype=np.uint64)
        tr = np.ascontiguousarray(tracked, dtype=np.uint8)
        n64 = np.ascontiguousarray(nonces, dtype=np.uint64) if nonces is not None else None
        k64 = np.ascontiguousarray(keys, dtype=np.uint64) if keys is not None else None
        self._L.check(self._L.mj_replay_load(self.h, script.ctypes.data, off.ctypes.data, tr.ctypes.data, len(scripts),
                                             int(always_include_kan_select), n64.ctypes.data if n64 is not None else None,
                                             k64.ctypes.data if k64 is not None else None))

    def replay_load_pool(self, src, table0=0, tracked=None, always_include_kan_select=True, deal_from_seed=False, augmented=False):
        """Load the device logs of src's tables [table0, table0 + self.n_tables) as this pool's replay scripts, on the device
        (mj_replay_load_pool; src needs enable_log).  tracked: 4-bit seat mask per table (None = all four seats);
        deal_from_seed: the walls are rebuilt from the tables' seeds, which come with the logs (the invisible obs);
        augmented: the copy swaps manzu and pinzu in every tile of the script (Event::augment; MJ_LOAD_AUGMENT), src's log stays.
        -> dict(loaded, skipped, malformed): a table still playing or in error is skipped, it replays as an empty log."""
        return self._replay_load_src(TablePool, src, table0, tracked, always_include_kan_select, deal_from_seed, augmented)

    def replay_load_harvest(self, harvest, game0=0, tracked=None, always_include_kan_select=True, deal_from_seed=False,
                            augmented=False):
        """The same from a Harvest: games [game0, game0 + self.n_tables) of its sorted order (mj_replay_load_harvest); the seeds
        come from the records; augmented as in replay_load_pool.  -> dict(loaded, skipped, malformed): a game in error is skipped."""
        return self._replay_load_src(Harvest, harvest, game0, tracked, always_include_kan_select, deal_from_seed, augmented)

    def _replay_load_src(self, cls, src, first, tracked, always_include_kan_select, deal_from_seed, augmented):
        """replay_load_pool / replay_load_harvest: logs [first, first + self.n_tables) of `src`, a `cls` (TablePool or Harvest)."""
        tr = None
        if tracked is not None:
            tr = np.ascontiguousarray(tracked, dtype=np.uint8)
            if tr.shape != (self.n_tables,):
                raise ValueError(f"tracked: expected {self.n_tables} masks, got shape {tr.shape}")
        if not isinstance(src, cls) or src._L is not self._L:
            raise MortalAmdError(f"replay_load_{cls.log_where}: the source must be {cls._src_name} of the same library")
        counts = np.zeros(3, dtype=np.int64)
        load = getattr(self._L, f"mj_replay_load_{cls.log_where}")
        self._L.check(load(self.h, src._handle(), int(first), tr.ctypes.data if tr is not None else None,
                           int(always_include_kan_select), _load_flags(deal_from_seed, augmented), counts.ctypes.data,
                           self._L.stream()))
        self.n_rows = [0, 0]
        return dict(loaded=int(counts[0]), skipped=int(counts[1]), malformed=int(counts[2]))

    def replay_step(self):
        self._L.check(self._L.mj_replay_step(self.h, self._L.stream()))
        out = (C.c_int32 * 2)()
        self._L.check(self._L.mj_rows_count(self.h, out, self._L.stream()))
        self.n_rows = [out[0], out[1]]
        return out[0]

    def replay_meta(self):
        """int32 cuda [n, 8] = label, log, seat, kyoku index, turn, shanten, is-kan-row, event index."""
        n = self.n_rows[0]
        meta = torch.empty((n, 8), dtype=torch.int32, device=self.device)
        if n:
            self._L.check(self._L.mj_replay_meta(self.h, meta.data_ptr(), self._L.stream()))
        return meta

    def set_refill(self, nonce_stride):
        self._L.check(self._L.mj_pool_set_refill(self.h, nonce_stride))

    def set_start_stagger(self, cycles):
        """Steady-state runs: table t starts its first hanchan at cycle hash(t) % cycles (after reset + set_refill)."""
        self._L.check(self._L.mj_pool_set_start_stagger(self.h, int(cycles), self._L.stream()))

    # ---- finished games of a pool in refill mode (include/mortal_amd.h mj_pool_enable_harvest ..)
    def enable_harvest(self, max_games, max_words):
        """Collect every finished game on the device just before its table is restarted (needs enable_log; collects while
        set_refill is on): room for max_games games and max_words log words.  A game that finds the buffer full is dropped
        and counted.  Calling it again replaces the buffer and discards what it held; max_games 0 turns harvesting off."""
        self._L.check(self._L.mj_pool_enable_harvest(self.h, int(max_games), int(max_words)))

    def harvest_pending(self):
        """-> dict(games, words, dropped) in the active buffer right now."""
        out = np.zeros(3, dtype=np.int64)
        self._L.check(self._L.mj_harvest_pending(self.h, out.ctypes.data, self._L.stream()))
        return dict(games=int(out[0]), words=int(out[1]), dropped=int(out[2]))

    def take_harvest(self):
        """Detach what has been collected as a Harvest; the pool goes on collecting into a fresh buffer.  A game that has
        finished but whose table has not been restarted yet (that happens in the next step) is in the next take."""
        hp = C.c_void_p()
        self._L.check(self._L.mj_harvest_take(self.h, C.byref(hp), self._L.stream()))
        return Harvest(self, hp)

    def step(self, actions0=None, actions1=None, q0=None, q1=None, ev0=None, ev1=None):
        """One arena cycle; actionsN = int32 cuda tensor with one action per row of agent N's last batch; qN = that
        batch's q-values (f32 cuda [n, 46]), needed only by an agent configured with the rule-based agari guard."""
        for a in (actions0, actions1):
            if a is not None:
                assert a.device.type == self.device.type and a.dtype == torch.int32 and a.is_contiguous()
        for q in (q0, q1):
            if q is not None:
                assert q.device.type == self.device.type and q.dtype == torch.float32 and q.is_contiguous() and q.shape[-1] == 46
        # one action per row of the batch the previous step produced: the step kernel indexes these tensors by row id
        for ag, (a, q) in enumerate(((actions0, q0), (actions1, q1))):
            if a is not None and a.numel() != self.n_rows[ag]:
                raise MortalAmdError(f"agent {ag}: {a.numel()} actions for a batch of {self.n_rows[ag]} rows")
            if q is not None and q.numel() != self.n_rows[ag] * ACTION_SPACE:
                raise MortalAmdError(f"agent {ag}: q-values of shape {tuple(q.shape)} for a batch of {self.n_rows[ag]} rows")
            ev = (ev0, ev1)[ag]
            if ev is not None and (ev.dtype != torch.int64 or ev.numel() != self.n_rows[ag] or not ev.is_contiguous()
                                   or ev.device.type != self.device.type):
                raise MortalAmdError(f"agent {ag}: reactions must be {self.n_rows[ag]} contiguous int64 event words on the device")
            if a is None and ev is None and self.n_rows[ag]:
                raise MortalAmdError(f"agent {ag}: the previous batch had {self.n_rows[ag]} rows but no actions were passed")
        p0 = actions0.data_ptr() if actions0 is not None and actions0.numel() else None
        p1 = actions1.data_ptr() if actions1 is not None and actions1.numel() else None
        pq0 = q0.data_ptr() if q0 is not None and q0.numel() else None
        pq1 = q1.data_ptr() if q1 is not None and q1.numel() else None
        pe0 = ev0.data_ptr() if ev0 is not None and ev0.numel() else None
        pe1 = ev1.data_ptr() if ev1 is not None and ev1.numel() else None
        L = self._L
        L.check(L.mj_step_ev(self.h, p0, p1, pq0, pq1, pe0, pe1, L.stream()))
        out = (C.c_int32 * 2)()
        L.check(L.mj_rows_count(self.h, out, L.stream()))
        self.n_rows = [out[0], out[1]]
        return self.n_rows

    def rows(self, agent):
        """Row descriptors of the current batch as an int64 cpu array [n, 3] = (table, seat, is_kan)."""
        n = self.n_rows[agent]
        ptr = self._L.mj_rows_dev(self.h, agent)
        d = torch.empty(n, dtype=torch.int32, device=self.device)
        if n:
            self._copy_rows(d.data_ptr(), ptr, 4 * n)
        v = d.cpu().numpy().view(np.uint32)
        return np.stack([v & 0x0FFFFFFF, (v >> 28) & 3, v >> 31], axis=1).astype(np.int64)

    def _copy_rows(self, dst, src, nbytes):
        torch.cuda.current_stream().synchronize()
        _memcpy_d2d(dst, src, nbytes)

    def encode(self, agent, obs=None, masks=None):
        """Encode agent's rows in place into (or into fresh) device tensors. Returns (obs [n,C,34] f32, masks [n,46] bool)."""
        n = self.n_rows[agent]
        if obs is None:
            obs = torch.empty((n, OBS_ROWS[self.versions[agent]], 34), dtype=torch.float32, device=self.device)
        if masks is None:
            masks = torch.empty((n, ACTION_SPACE), dtype=torch.bool, device=self.device)
        assert obs.is_contiguous() and masks.is_contiguous() and obs.shape[0] >= n and masks.shape[0] >= n
        if n:
            L = self._L
            L.check(L.mj_encode(self.h, agent, obs.data_ptr(), masks.data_ptr(), L.stream()))
        return obs[:n], masks[:n]

    def encode_oracle(self, agent, out=None):
        """Invisible ("oracle") obs of agent's rows (board.rs:679-782): f32 cuda [n, 211|217, 34]."""
        n = self.n_rows[agent]
        R = self._L.mj_oracle_obs_rows(self.versions[agent])
        if out is None:
            out = torch.empty((n, R, 34), dtype=torch.float32, device=self.device)
        assert out.device.type == self.device.type and out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] >= n
        assert tuple(out.shape[1:]) == (R, 34)
        self._L.check(self._L.mj_encode_oracle(self.h, agent, out.data_ptr(), self._L.stream()))
        return out[:n]

    def random_policy(self, agent, masks, seed, cycle, out=None):
        n = self.n_rows[agent]
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.device)
        if n:
            L = self._L
            L.check(L.mj_random_policy(self.h, agent, masks.data_ptr(), seed, cycle, out.data_ptr(), L.stream()))
        return out[:n]

    def greedy_policy(self, agent, masks, obs, seed, cycle, out=None):
        """Tenpai-seeking policy on device (mj_greedy_policy); obs = the encoded batch of this agent's rows."""
        n = self.n_rows[agent]
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.device)
        if n:
            L = self._L
            L.check(L.mj_greedy_policy(self.h, agent, masks.data_ptr(), obs.data_ptr(), seed, cycle, out.data_ptr(), L.stream()))
        return out[:n]

    def counters(self):
        out = (C.c_uint64 * 8)()
        self._L.check(self._L.mj_counters(self.h, out, self._L.stream()))
        return dict(steps=out[0], games=out[1], errors=out[2], decisions=out[3], quick=out[4], cycles=out[5],
                    sp_overflow=out[6])

    def check_sp_overflow(self, error=None):
        """Raise when an obs-v4 row of this pool outgrew the SP kernel's scratch; `error`: what to raise instead of the arena's."""
        if self.counters()["sp_overflow"]:
            raise error or MortalAmdError("obs v4: a decision's single-player state graph exceeded the device scratch capacity "
                                          "(SP_CAP in mortal_amd/csrc/mj_sp.hip); its SP planes would be incomplete")

    def results(self):
        scores = np.zeros((self.n_games_total, 4), dtype=np.int32)
        done = np.zeros(self.n_games_total, dtype=np.uint8)
        self._L.check(self._L.mj_results(self.h, scores.ctypes.data, done.ctypes.data, self._L.stream()))
        return scores, done

    def first_error(self):
        t = C.c_int(-1)
        code = self._L.check(self._L.mj_pool_first_error(self.h, C.byref(t), self._L.stream()))
        return code, t.value

    def encode_timing(self, enable=True):
        ms = C.c_double(0)
        n = C.c_int64(0)
        self._L.check(self._L.mj_encode_timing(self.h, int(enable), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def sp_timing(self):
        """(total ms, launches) of the SP-table kernel since the last call (recorded while encode timing is on)."""
        ms = C.c_double(0)
        n = C.c_int64(0)
        self._L.check(self._L.mj_sp_timing(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def sp_phase_ticks(self):
        """Cumulative mj_k_sp phase timers (workgroup ticks, 100 MHz) and counts since the pool was created."""
        out = (C.c_uint64 * 9)()
        self._L.check(self._L.mj_sp_phase_ticks(self.h, out, self._L.stream()))
        return dict(zip(("overflow", "rows", "setup", "expand", "level0", "eval", "write", "states", "dead_leaf_rows"), (int(x) for x in out)))

    def set_sp_schedule(self, mode=-2, max_rows=0, wide_grid=0, min_level1=0, min_level2=0):
        """Small-pool schedule of the SP kernel (include/mortal_amd.h mj_pool_set_sp_schedule): mode -1 auto / 0 never / 1 always."""
        self._L.check(self._L.mj_pool_set_sp_schedule(self.h, mode, max_rows, wide_grid, min_level1, min_level2))

    def sp_schedule_stats(self):
        out = (C.c_uint64 * 4)()
        self._L.check(self._L.mj_sp_schedule_stats(self.h, out, self._L.stream()))
        return dict(zip(("hybrid_launches", "rows_promoted", "rows_swept", "wide_gave_up"), (int(x) for x in out)))

    def debug_table(self, table):
        size = self._L.mj_debug_table_size()
        buf = (C.c_uint8 * size)()
        self._L.check(self._L.mj_debug_table(self.h, table, buf, size, self._L.stream()))
        raw = bytes(buf)
        out = {}
        for ent in self._L.mj_debug_layout().decode().strip(";").split(";"):
            name, size, count, off = ent.split(":")
            size, count, off = int(size), int(count), int(off)
            dt = {1: np.uint8, 2: np.uint16, 4: np.int32, 8: np.uint64}[size]
            out[name] = np.frombuffer(raw, dtype=dt, count=count, offset=off).copy()
        return out


def _memcpy_d2d(dst, src, nbytes):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rc = hip.hipMemcpy(dst, src, nbytes, 3)  # hipMemcpyDeviceToDevice
    if rc != 0:
        raise MortalAmdError(f"hipMemcpy failed: {rc}")
