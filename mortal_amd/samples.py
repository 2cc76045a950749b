"""SampleStore: replayed decisions kept on the device as records, encoded in batches on demand (include/mortal_amd.h mj_samples_*).

The reference's data loader keeps every obs of a batch of files in a buffer and shuffles it (mortal/dataloader.py:45-113
populate_buffer + random.shuffle), at 127 to 138 KB per sample.  The encoders read nothing of a decision but its snapshot record
(about 2 KB) and a row descriptor, so a store keeps those with the sample's bookkeeping and runs the unchanged obs / mask / SP
kernels over any list of its samples: what stays resident is 1/58 of the obs, and only the samples a batch draws are ever encoded.
A store is the one way from a replayed log to a sample: `GameplayLoader.store_pool` / `store_harvest` fill one and hand it over;
`load_logs` / `load_pool` / `load_harvest` fill one of their own, take `gameplays()` of it -- every obs of the range, encoded once
and in the reference's order -- and close it.
"""
import numpy as np
import torch

from ._lib import MortalAmdError, lib
from .pool import ACTION_SPACE, OBS_ROWS

MAX_CAPACITY = (1 << 28) - 1  # a sample's index takes the 28 table bits of a row descriptor


class SampleStore:
    """capacity samples of obs `version`; batch_rows = rows per encode launch (a larger batch is served in chunks; for obs v4 it
    sizes the SP work areas like a pool of that many tables).

    A sample has a store index (the order of arrival) and a place in the reference's order (by game, seat, event, the kan-select
    entry behind its main entry): `order[k]` is the store index of the k-th sample of that order, and every column below is an
    array in that order -- `actions[k]` belongs to sample `order[k]`.  A shuffled batch is a set of positions `pos` drawn from
    `range(count)`: `encode(order[pos])` with `actions[pos]`, `steps_to_done[pos]`, ...

    Games are numbered in the order they were added (GameplayLoader.store_pool / store_harvest): `grps[g]` is the Grp of game g
    (None for a game that was skipped), `names[g]` its four player names, `wanted[g]` the seats that were asked for."""

    _L = lib  # the C-ABI library; `lib=` is for the test suite (the host emulation of the same sources)

    def __init__(self, capacity, version, batch_rows=1024, device="cuda:0", lib=None):
        if version not in OBS_ROWS:
            raise ValueError(f"unsupported obs version {version}")
        L = self._L = lib or type(self)._L
        if L.host_emulation:
            self.device = torch.device("cpu")
        else:
            from .pool import _ensure_tables

            if not torch.cuda.is_available():
                raise MortalAmdError("SampleStore needs a HIP device (torch.cuda.is_available() is False)")
            self.device = torch.device(device)
            torch.cuda.set_device(self.device)
            _ensure_tables()
        self.version = version
        self.C = OBS_ROWS[version]
        self.batch_rows = int(batch_rows)
        self.h = None
        self.h = L.check(L.mj_samples_create(int(capacity), version, self.batch_rows))
        info = self._info()
        self.count, self.capacity, self.bytes_per_sample = 0, info[1], info[2]
        self.grps, self.names, self.wanted = [], [], []
        self.has_walls = True  # every game so far came with its walls (oracle=True): encode_oracle means something
        self._cache = {}

    def close(self):
        if getattr(self, "h", None):
            self._L.mj_samples_destroy(self.h)
            self.h = None

    __del__ = close

    def _handle(self):
        if not getattr(self, "h", None):
            raise MortalAmdError("the SampleStore is closed")
        return self.h

    def _info(self):
        out = np.zeros(4, dtype=np.int64)
        self._L.check(self._L.mj_samples_info(self._handle(), out.ctypes.data))
        return [int(x) for x in out]

    def __len__(self):
        return self.count

    # ---- filling
    def append(self, pool, log_base=0):
        """The rows of agent 0 of a replay pool's current batch (TablePool.replay_step) become the next samples, all or none;
        log_base = the game number of the pool's table 0.  -> the number of samples added."""
        L = self._L
        if getattr(pool, "_L", None) is not L:
            raise MortalAmdError("SampleStore.append: the pool must be a pool of the same library")
        L.check(L.mj_samples_append(self._handle(), pool.h, int(log_base), L.stream()))
        self.count += pool.n_rows[0]
        self._cache = {}
        return pool.n_rows[0]

    def truncate(self, n):
        """Forget the samples from store index n on."""
        self._L.check(self._L.mj_samples_truncate(self._handle(), int(n)))
        self.count = int(n)
        self._cache = {}

    def clear(self):
        self.truncate(0)
        self.grps, self.names, self.wanted = [], [], []
        self.has_walls = True

    def _mark(self):
        return self.count, len(self.grps), self.has_walls

    def _rollback(self, mark):
        count, n_games, self.has_walls = mark
        del self.grps[n_games:], self.names[n_games:], self.wanted[n_games:]
        if getattr(self, "h", None) and self.count != count:
            self.truncate(count)

    def _add_games(self, games, walls):
        for g in games:
            self.grps.append(g["grp"])
            self.names.append(list(g["names"]))
            self.wanted.append(list(g["wanted"]))
        self.has_walls = self.has_walls and bool(walls)
        self._cache = {}

    # ---- bookkeeping, in the reference's order
    def _cached(self, name, make):
        if name not in self._cache:
            self._cache[name] = make()
        return self._cache[name]

    def _fetch_meta(self):
        meta = np.zeros((self.count, 8), dtype=np.int32)
        if self.count:
            L = self._L
            L.check(L.mj_samples_meta(self._handle(), 0, self.count, meta.ctypes.data, L.stream()))
        return meta

    @property
    def meta(self):
        """int32 [count, 8] by store index = label, game, seat, kyoku index, turn, shanten, is kan-select row, event index."""
        return self._cached("meta", self._fetch_meta)

    @property
    def order(self):
        """The permutation that puts the samples in the reference's order: by game, seat, event, the kan-select entry behind its
        main entry (gameplay.rs:239-443 walks one player's events in order)."""
        m = self.meta
        return self._cached("order", lambda: np.lexsort((m[:, 6], m[:, 7], m[:, 2], m[:, 1])).astype(np.int64))

    def _sorted(self):
        return self._cached("sorted", lambda: self.meta[self.order])

    actions = property(lambda s: s._sorted()[:, 0].astype(np.int64))
    game = property(lambda s: s._sorted()[:, 1].astype(np.int64))
    seat = property(lambda s: s._sorted()[:, 2].astype(np.int64))
    at_kyoku = property(lambda s: s._sorted()[:, 3].astype(np.int64))
    at_turns = property(lambda s: s._sorted()[:, 4].astype(np.int64))
    shantens = property(lambda s: s._sorted()[:, 5].astype(np.int64))

    @property
    def apply_gamma(self):
        return self._sorted()[:, 0] <= 37  # only discard and kan will discount (gameplay.rs:423)

    @property
    def dones(self):
        """gameplay.rs:264-265: the last entry of a kyoku, per game and seat."""
        def make():
            m = self._sorted()
            d = np.ones(len(m), dtype=bool)
            if len(m) > 1:
                same = (m[1:, 1] == m[:-1, 1]) & (m[1:, 2] == m[:-1, 2])
                d[:-1] = ~same | (m[1:, 3] > m[:-1, 3])
            return d
        return self._cached("dones", make)

    @property
    def steps_to_done(self):
        """mortal/dataloader.py:110-113: the discounting entries between a sample and the end of its kyoku."""
        def make():
            n = self.count
            if n == 0:
                return np.zeros(0, dtype=np.int64)
            before = np.concatenate(([0], np.cumsum(self.apply_gamma.astype(np.int64))))  # discounting entries in front of k
            ends = np.flatnonzero(self.dones)
            end = ends[np.searchsorted(ends, np.arange(n))]  # the done entry at or behind k (the last entry is one)
            return before[end] - before[:n]
        return self._cached("steps_to_done", make)

    def _bounds(self, game, seat):
        """The positions [lo, hi) of one Gameplay (game, seat) in the reference's order."""
        key = self._cached("key", lambda: self._sorted()[:, 1].astype(np.int64) * 4 + self._sorted()[:, 2])
        return np.searchsorted(key, [game * 4 + seat, game * 4 + seat + 1])

    def span(self, game, seat):
        """The store indices of one Gameplay (game, seat), in the reference's order."""
        return self.order[slice(*self._bounds(game, seat))]

    # ---- encoding
    def _indices(self, idx):
        if isinstance(idx, torch.Tensor):
            idx = idx.cpu().numpy()
        a = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        if len(a) and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
            raise MortalAmdError(f"SampleStore: an index does not fit 32 bits (a store holds at most {MAX_CAPACITY} samples)")
        return a.astype(np.int32)

    def _out(self, t, n, tail, dtype, what):
        if t is None:
            return torch.empty((n,) + tail, dtype=dtype, device=self.device)
        if not (t.dtype == dtype and t.is_contiguous() and t.device.type == self.device.type and t.shape[0] >= n
                and tuple(t.shape[1:]) == tail):
            raise MortalAmdError(f"SampleStore: {what} must be a contiguous {dtype} tensor [>= {n}, {tail[0]}, ...] on {self.device}")
        return t

    def encode(self, idx, obs=None, masks=None):
        """-> (obs [n, C, 34] f32, masks [n, 46] bool) on the device: row i is sample idx[i] (store indices: any order,
        duplicates allowed), bit for bit what the arena's encoders gave when the decision was replayed.  An index outside the
        store is refused before anything is written."""
        h = self._handle()
        a = self._indices(idx)
        n = len(a)
        obs = self._out(obs, n, (self.C, 34), torch.float32, "obs")
        masks = self._out(masks, n, (ACTION_SPACE,), torch.bool, "masks")
        L = self._L
        L.check(L.mj_samples_encode(h, a.ctypes.data, n, obs.data_ptr(), masks.data_ptr(), L.stream()))
        return obs[:n], masks[:n]

    def encode_oracle(self, idx, out=None):
        """-> the invisible obs [n, 211 | 217, 34] f32 of samples idx (dataset/invisible.rs); the games must have come with their
        walls (a loader with oracle=True)."""
        h = self._handle()
        a = self._indices(idx)
        n = len(a)
        L = self._L
        out = self._out(out, n, (L.mj_oracle_obs_rows(self.version), 34), torch.float32, "out")
        L.check(L.mj_samples_encode_oracle(h, a.ctypes.data, n, out.data_ptr(), L.stream()))
        return out[:n]

    def check_overflow(self, error=None):
        """Raise (`error`, when given) when an encode of this store overflowed the encoder's op list or the SP kernel's scratch
        (its rows are incomplete)."""
        if self._info()[3]:
            raise error or MortalAmdError("SampleStore: an encoded sample overflowed the encoder's op list or, for obs v4, its "
                                          "single-player state graph exceeded the device scratch capacity (SP_CAP in mortal_amd/csrc/mj_sp.hip)")

    def _build(self, pairs, lo, hi, invisible):
        """The Gameplays (gameplay.rs:46-64) of `pairs` (game, seat), all within positions [lo, hi) of the reference's order:
        that range is encoded once, each Gameplay takes its slice."""
        from .dataset import Gameplay, Grp

        obs, masks = self.encode(self.order[lo:hi])
        inv = self.encode_oracle(self.order[lo:hi]).cpu().numpy() if (self.has_walls if invisible is None else invisible) else None
        cols = [getattr(self, c) for c in ("actions", "at_kyoku", "at_turns", "shantens", "apply_gamma", "dones")]
        out = []
        for game, seat in pairs:
            a, b = self._bounds(game, seat)
            g = self.grps[game]
            gp = Gameplay(seat, self.names[game][seat], Grp(g.feature.copy(), g.rank_by_player, g.final_scores))
            gp.obs_dev, gp.masks_dev = obs[a - lo:b - lo], masks[a - lo:b - lo]
            if inv is not None:
                gp.invisible_obs = list(inv[a - lo:b - lo])
            gp.actions, gp.at_kyoku, gp.at_turns, gp.shantens, gp.apply_gamma, gp.dones = (c[a:b].tolist() for c in cols)
            gp.dones = gp.dones or [True]  # (the reference's list ends in True even when it is empty: gameplay.rs:264-265)
            out.append(gp)
        return out

    def gameplays(self, invisible=None):
        """What GameplayLoader.load_pool returns: a list per game of Gameplay, one per wanted seat (none for a skipped game), their
        obs, masks (and invisible obs: default = the store has the walls) encoded now, once, in the reference's order."""
        self._handle()
        built = iter(self._build([(g, p) for g, seats in enumerate(self.wanted) for p in seats], 0, self.count, invisible))
        return [[next(built) for _ in seats] for seats in self.wanted]

    def gameplay(self, game, seat, invisible=None):
        """One Gameplay of gameplays(), encoded from span(game, seat) alone."""
        self._handle()
        if not 0 <= game < len(self.grps) or self.grps[game] is None or seat not in self.wanted[game]:
            raise ValueError(f"SampleStore.gameplay: the store has no Gameplay of game {game}, seat {seat}")
        return self._build([(game, seat)], *self._bounds(game, seat), invisible)[0]
