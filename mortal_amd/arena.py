"""Host side of the batched arena: mirrors `libriichi.arena` (reference libriichi/src/arena/one_vs_three.rs:17-113,
two_vs_two.rs:17-110) on top of the HIP table pool.

The poll/commit cycle of `BatchGame::run` (arena/game.rs:286-304) becomes, per cycle:
    mj_step (commit + poll + classify, on device)  ->  per agent: mj_encode -> engine.react_batch -> actions
The engine contract is the reference's (agent/mortal.rs:50-159): attributes `engine_type`, `name`, `is_oracle`,
`version`, `enable_quick_eval`, `enable_rule_based_agari_guard`, and
`react_batch(obs, masks, invisible_obs) -> (actions, q_values, masks, is_greedy)`.

Zero-copy: `MortalEngine._react_batch` (mortal/engine.py:53-55) does `torch.as_tensor(np.stack(obs, axis=0), device=..)`.
We pass `[proxy]` whose `__array_function__` answers `np.stack` with the pre-stacked device tensor, so the unchanged
engine consumes the encoded batch in place.  Engines that define `react_batch_device(obs, masks)` (our extension,
returns a device int tensor of actions) skip the `.tolist()` round trip as well.
"""
import os
import time

import numpy as np
import torch

from .pool import ACTION_SPACE, OBS_ROWS, TablePool
from ._lib import MortalAmdError


class _StackedBatch:
    """Stands in for a list of per-row numpy arrays; np.stack([proxy], axis=0) returns the device tensor."""

    def __init__(self, tensor):
        self.tensor = tensor

    def __array_function__(self, func, types, args, kwargs):
        if func is np.stack:
            return self.tensor
        return NotImplemented

    def __len__(self):
        return self.tensor.shape[0]


def _check_engine(engine):
    """agent/py_agent.rs:24-37: dispatch on `engine_type`."""
    et = getattr(engine, "engine_type")
    if et == "mjai-log":  # agent/mjai_log.rs:34-63
        for method in ("react_batch", "start_game", "end_kyoku", "end_game"):
            if not callable(getattr(engine, method, None)):
                raise TypeError(f"missing method {method}")
        # every decision gets a row (no quick-eval), nothing is encoded for it, reactions are explicit mjai events
        return dict(name=str(engine.name), version=0, quick=False, guard=False, oracle=False, mjai_log=True)
    if et != "mortal":
        raise ValueError(f"unknown engine type {et}")
    if not callable(getattr(engine, "react_batch", None)):
        raise TypeError("missing method react_batch")
    return dict(name=str(engine.name), version=int(engine.version), quick=bool(engine.enable_quick_eval),
                guard=bool(getattr(engine, "enable_rule_based_agari_guard")), oracle=bool(getattr(engine, "is_oracle")),
                mjai_log=False)


class GameState:
    """What an mjai-log engine's `react_batch` receives per decision (agent/mjai_log.rs:22-32)."""

    def __init__(self, game_index, state, events_json):
        self.game_index = game_index    # index of this player in the list given to `set_player_ids`
        self.state = state              # libriichi.state.PlayerState (a copy of the seat's state)
        self.events_json = events_json  # the current kyoku's log so far, a JSON array of mjai events


def pack_reaction(ev):
    """mjai reaction dict -> the header word of the device's event format (mj_state.h LG_*), 0 for {"type":"none"}."""
    from . import mjai_log as ML

    t = ev["type"]
    if t == "none":
        return 0
    if t in ("hora", "ryukyoku"):  # header only: deltas / ura markers are the board's business
        code = ML.LG_HORA if t == "hora" else ML.LG_RYUKYOKU
        return code | (int(ev.get("actor", 0)) << 4) | (int(ev.get("target", 0)) << 6)
    return int(ML.encode_events([ev])[0])


class _EngineRunner:
    """What BatchRunner and SelfPlayRunner share: the engine checks, the pool the engines play on, and a cycle's answer of one agent."""

    pool_cls = TablePool  # the test suite substitutes the host emulation of the same kernels (tests/host/emu_pool.py)
    keep_log = False

    def _open_pool(self, engines, n, device, deal_algo):
        """The engine checks and the pool they play on (shared with SelfPlayRunner)."""
        self.engines = engines
        self.cfg = [_check_engine(e) for e in engines]
        dev = device
        if dev is None:
            d0 = getattr(engines[0], "device", None)
            dev = d0 if isinstance(d0, torch.device) and d0.type == "cuda" else torch.device(
                f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else "cuda:0")
        self.device = torch.device(dev)
        versions = [c["version"] for c in self.cfg if c["version"]] or [3]
        for c in self.cfg:
            c["version"] = c["version"] or versions[0]  # an mjai-log agent's rows are never encoded
        self.pool = self.pool_cls(n, version=self.cfg[0]["version"], deal_algo=deal_algo, device=str(self.device))
        self.device = self.pool.device
        self.any_mjai_log = any(c["mjai_log"] for c in self.cfg)

    def _configure_agents(self):
        for a, c in enumerate(self.cfg):
            self.pool.configure(a, enable_quick_eval=c["quick"], version=c["version"], enable_rule_based_agari_guard=c["guard"])
        if len(self.engines) == 1:
            self.pool.configure(1, enable_quick_eval=self.cfg[0]["quick"], version=self.cfg[0]["version"],
                                enable_rule_based_agari_guard=self.cfg[0]["guard"])

    def _seat_names(self, agent_of_seat):
        """Per game its four seats named by the engine that plays them (game.rs:186); agent_of_seat: bit s = agent of seat s."""
        names = [c["name"] for c in self.cfg] * (2 if len(self.cfg) == 1 else 1)  # a single engine plays both agents' seats
        return [[names[(int(m) >> s) & 1] for s in range(4)] for m in agent_of_seat]

    def _policy(self, agent, obs, masks, invisible=None):
        """-> (actions int32 cuda [n], q_values f32 cuda [n,46] or None).  q-values are kept only for a guarded agent."""
        eng = self.engines[agent]
        guard = self.cfg[agent]["guard"]
        if hasattr(eng, "react_batch_device"):
            out = eng.react_batch_device(obs, masks, invisible) if invisible is not None else eng.react_batch_device(obs, masks)
            out = out if isinstance(out, tuple) else (out,)
            act, q, is_greedy = out[0], (out[1] if len(out) > 1 else None), (out[2] if len(out) > 2 else None)
            if guard and q is None:
                raise RuntimeError("enable_rule_based_agari_guard: react_batch_device must return (actions, q_values)")
            if self.keep_log and q is not None:  # per-decision metadata of the game logs (agent/mortal.rs:161-186)
                g = is_greedy if is_greedy is not None else torch.ones(obs.shape[0], dtype=torch.bool)
                self._last_meta = (q.float().cpu().numpy().reshape(-1, ACTION_SPACE), masks.cpu().numpy().astype(bool),
                                   g.cpu().numpy().astype(bool).reshape(-1))
            q = q.to(device=self.device, dtype=torch.float32).contiguous() if guard else None
            return act.to(device=self.device, dtype=torch.int32).contiguous(), q
        try:
            inv = [_StackedBatch(invisible)] if invisible is not None else None  # mortal.rs:137-145
            actions, q_values, _m, _g = eng.react_batch([_StackedBatch(obs)], [_StackedBatch(masks)], inv)
        except Exception as ex:  # same context string as agent/mortal.rs:149
            raise RuntimeError(f"failed to execute `react_batch` on Python engine: {ex}") from ex
        if len(actions) != obs.shape[0]:
            raise RuntimeError("react_batch returned a batch of the wrong size")
        if self.keep_log:  # per-decision metadata of the game logs (agent/mortal.rs:161-186)
            self._last_meta = (np.asarray(q_values, dtype=np.float32).reshape(-1, ACTION_SPACE),
                               np.asarray(_m, dtype=bool).reshape(-1, ACTION_SPACE), np.asarray(_g, dtype=bool).reshape(-1))
        q = torch.as_tensor(q_values, dtype=torch.float32, device=self.device).contiguous() if guard else None
        return torch.as_tensor(actions, dtype=torch.int32, device=self.device), q


    def _answer(self, a, n_rows):
        """Agent a's batch of this cycle encoded, put to its engine and checked -> (actions, q-values or None, the engine's ns)."""
        pool = self.pool
        obs, masks = pool.encode(a)
        inv = pool.encode_oracle(a) if self.cfg[min(a, len(self.cfg) - 1)]["oracle"] else None
        self._last_meta = None
        t0 = time.perf_counter_ns()
        acts, qs = self._policy(a, obs, masks, inv)
        if acts.numel() != n_rows or (qs is not None and tuple(qs.shape) != (n_rows, ACTION_SPACE)):
            raise RuntimeError(f"engine returned {acts.numel()} actions"
                               + (f" / q-values of shape {tuple(qs.shape)}" if qs is not None else "")
                               + f" for a batch of {n_rows} rows")
        return acts, qs, time.perf_counter_ns() - t0


    def close(self):
        self.pool.close()


class BatchRunner(_EngineRunner):
    """Drives N tables to completion with up to two engines (agent 0 / agent 1)."""

    def __init__(self, engines, seeds, agent_of_seat, device=None, deal_algo=None, keep_log=False, keep_stat=False):
        n = len(seeds)
        self._open_pool(engines, n, device, deal_algo)
        # mjai-log engines read the kyoku's events from the device log; keep_stat needs the log on the device and nothing else
        # (no q-values, no per-decision metadata: those are keep_log's)
        if keep_log or keep_stat or self.any_mjai_log:
            self.pool.enable_log()
        self.seeds = list(seeds)
        self.agent_of_seat = np.asarray(agent_of_seat, dtype=np.uint8)
        self.pool.reset(seeds, game_ids=np.arange(n), agent_of_seat=agent_of_seat, n_games_total=n)
        self._configure_agents()
        # player planning of the reference (one_vs_three.rs:140-191, two_vs_two.rs:138-190): per agent the seats it plays,
        # games in order, seats ascending; an mjai-log engine addresses its players by their index in that list
        self.player_index = [{}, {}]
        player_ids = [[], []]
        for g in range(n):
            for seat in range(4):
                a = (int(self.agent_of_seat[g]) >> seat) & 1 if len(engines) > 1 else 0
                self.player_index[a][(g, seat)] = len(player_ids[a])
                player_ids[a].append(seat)
        self._kyoku_ends = {}  # game -> end_kyoku events already reported to the mjai-log engines
        self._log_cache = {}   # game -> (words decoded, events): the mjai-log agents' view of the device event log
        self._lens, self._lens_cycle = None, -1
        for a, eng in enumerate(engines):
            if self.cfg[a]["mjai_log"]:
                if callable(getattr(eng, "set_player_ids", None)):
                    eng.set_player_ids(player_ids[a])
                for idx in range(len(player_ids[a])):
                    eng.start_game(idx)
        self.cycles = 0
        self.keep_log = keep_log
        self.meta_batches = {}  # step index -> per agent (q_values, masks, is_greedy, eval_time_ns) of the rows it commits

    def _fail(self, code, tbl):
        """Illegal action / rule violation on table `tbl`: the reference aborts the whole run with the offending event and
        the seat's `brief_info()` (arena/board.rs:524-533); here the table's state at the time of the check is dumped."""
        lines = [f"table {tbl} (seed {self.seeds[tbl] if 0 <= tbl < len(self.seeds) else '?'}): illegal action or rule violation "
                 f"(error code {code}, include/mortal_amd.h MJ_ERR_*)"]
        try:
            d = self.pool.debug_table(tbl)
            names = "1m 2m 3m 4m 5m 6m 7m 8m 9m 1p 2p 3p 4p 5p 6p 7p 8p 9p 1s 2s 3s 4s 5s 6s 7s 8s 9s E S W N P F C".split()
            lines.append(f"  kyoku {int(d['kyoku'][0])} honba {int(d['honba'][0])} kyotaku {int(d['kyotaku'][0])} scores "
                         f"{d['scores'].tolist()} tiles_left {int(d['tiles_left'][0])} pending seats {int(d['pending'][0]):04b}")
            for seat in range(4):
                mp, sz = int(d["hand_mp"][seat]), int(d["hand_sz"][seat])
                cnt = [(mp >> (3 * t)) & 7 for t in range(18)] + [(sz >> (3 * t)) & 7 for t in range(16)]
                hand = " ".join(names[t] for t in range(34) for _ in range(cnt[t]))
                lines.append(f"  seat {seat}: shanten {int(d['shanten'][seat])} cans 0x{int(d['cans'][seat]):x} "
                             f"last_self_tsumo {int(d['last_self_tsumo'][seat])} hand [{hand}]")
        except Exception as ex:  # noqa: BLE001 - the diagnostic must not hide the error itself
            lines.append(f"  (state dump unavailable: {ex})")
        return MortalAmdError("\n".join(lines))

    def _log_lengths(self):
        """Event-log lengths of every table: read ONCE per cycle (the mjai-log agents of a cycle share it)."""
        if self._lens_cycle != self.cycles:
            self._lens, self._lens_cycle = self.pool.log_lengths(), self.cycles
        return self._lens

    def _game_log(self, g):
        """The decoded event log of game g, kept across cycles: only the words appended since the last look are decoded (a log
        always ends on an event boundary), instead of the whole hanchan every cycle."""
        from . import mjai_log

        n = int(self._log_lengths()[g])
        done, events = self._log_cache.get(g, (0, []))
        if n > done:
            events.extend(mjai_log.decode_events(self.pool.read_log(g, n)[done:]))  # in place: callers only read the list
            self._log_cache[g] = (n, events)
        return events

    def _report_kyoku_ends(self, g, events):
        """end_kyoku(player index) for every kyoku of game g that has ended since the last look (game.rs:113-118)."""
        n_end = sum(1 for e in events if e["type"] == "end_kyoku")
        for _ in range(n_end - self._kyoku_ends.get(g, 0)):
            for a, eng in enumerate(self.engines):
                if self.cfg[a]["mjai_log"]:
                    for seat in range(4):
                        idx = self.player_index[a].get((g, seat))
                        if idx is not None:
                            eng.end_kyoku(idx)
        self._kyoku_ends[g] = n_end

    def _mjai_log_policy(self, agent):
        """agent/mjai_log.rs:65-150: GameState per acting seat -> engine.react_batch -> validated, packed reactions."""
        import json

        from .state import PlayerState

        eng = self.engines[agent]
        rows = self.pool.rows(agent)
        words = np.zeros(len(rows), dtype=np.int64)
        states, where = [], []
        logs = {}
        for r, (g, seat, is_kan) in enumerate(rows):
            if is_kan:
                continue  # kan-select rows belong to the mortal agent's protocol; the event names the tile itself
            g, seat = int(g), int(seat)
            if g not in logs:
                logs[g] = self._game_log(g)
                self._report_kyoku_ends(g, logs[g])
            evs = logs[g]
            start = max(i for i, e in enumerate(evs) if e["type"] == "start_kyoku")
            st = PlayerState.view(self.pool, g, seat)
            states.append(GameState(self.player_index[agent][(g, seat)], st, json.dumps(evs[start:], separators=(",", ":"))))
            where.append((r, st))
        try:
            raw = eng.react_batch(states) if states else []
        except Exception as ex:
            raise RuntimeError(f"failed to execute `react_batch` on Python engine: {ex}") from ex
        if len(raw) != len(states):
            raise RuntimeError("react_batch returned a batch of the wrong size")
        for (r, st), text in zip(where, raw):
            ev = json.loads(text)
            try:  # BoardState::step validates every reaction (board.rs:524-533)
                st.validate_reaction(ev)
            except ValueError as ex:
                raise MortalAmdError(f"invalid action: {ev}: {ex}\nstate:\n{st.brief_info()}") from ex
            words[r] = pack_reaction(ev)
        return torch.from_numpy(words).to(self.device)

    def run(self, max_cycles=1 << 30, progress=None):
        """progress: None = silent (disable_progress_bar), else a label: the reference's bar message
        (`cycles: N (x cycle/s), actions: M (y action/s)`, arena/game.rs:303-311) goes to stderr about once a second."""
        import sys

        pool = self.pool
        acts = [None, None]
        qs = [None, None]
        evs = [None, None]
        n_games = pool.n_tables
        t_start = t_last = time.perf_counter()

        def report(final=False):
            c = pool.counters()
            secs = max(time.perf_counter() - t_start, 1e-9)
            print(f"\r{progress + ' ' if progress else ''}{c['games']}/{n_games} games  cycles: {self.cycles} "
                  f"({self.cycles / secs:.3f} cycle/s), actions: {c['steps']} ({c['steps'] / secs:.3f} action/s)",
                  end="\n" if final else "", file=sys.stderr, flush=True)

        while True:
            if self.cycles >= max_cycles:
                raise MortalAmdError("max_cycles exceeded")
            n = pool.step(acts[0], acts[1], qs[0], qs[1], evs[0], evs[1])
            self.cycles += 1
            code, tbl = pool.first_error() if (self.cycles & 63) == 0 else (0, -1)
            if code:
                raise self._fail(code, tbl)
            if progress is not None and time.perf_counter() - t_last > 1.0:
                t_last = time.perf_counter()
                report()
            acts = [None, None]
            qs = [None, None]
            evs = [None, None]
            if n[0] == 0 and n[1] == 0:
                c = pool.counters()
                if c["games"] >= n_games:
                    break
                continue
            for a in (0, 1):
                if n[a] == 0:
                    continue
                if self.cfg[min(a, len(self.cfg) - 1)]["mjai_log"]:
                    evs[a] = self._mjai_log_policy(min(a, len(self.cfg) - 1))
                    continue
                acts[a], qs[a], eval_ns = self._answer(a, n[a])
                if self.keep_log and self._last_meta is not None:
                    # these rows are committed by the NEXT mj_step call, whose index the device writes into the log tags
                    self.meta_batches.setdefault(self.cycles, {})[a] = self._last_meta + (eval_ns,)
        if progress is not None:
            report(final=True)
        code, tbl = pool.first_error()
        if code:
            raise self._fail(code, tbl)
        pool.check_sp_overflow()
        scores, done = pool.results()
        if not (done == 1).all():
            raise MortalAmdError("some games did not finish")
        if self.any_mjai_log:  # the last kyoku's end_kyoku, then end_game(index, scores) (game.rs:113-118,199-201)
            for g in range(n_games):
                self._report_kyoku_ends(g, self._game_log(g))
                for a, eng in enumerate(self.engines):
                    if self.cfg[a]["mjai_log"]:
                        for seat in range(4):
                            idx = self.player_index[a].get((g, seat))
                            if idx is not None:
                                eng.end_game(idx, [int(x) for x in scores[g]])
        return scores

    def agent_stats(self):
        """After run(): [Stat of agent 0's seats, Stat of agent 1's seats] over every game, reduced on the device from the
        event log (keep_stat / keep_log)."""
        totals, _rows, counts = self.pool.log_stat()
        if counts["reduced"] != self.pool.n_tables:
            raise MortalAmdError(f"stats: {counts['skipped']} games unfinished or in error, {counts['malformed']} malformed logs")
        return totals

    def stats(self):
        """After run(): {engine name: Stat}, what `Stat.from_dir(log_dir, name)` gives on the dumped logs (engines of the same
        name are summed there too, stat.rs:443-498)."""
        return _stats_by_name([c["name"] for c in self.cfg], [t.counters() for t in self.agent_stats()])

    def gameplays(self, loader, seats=None, augmented=False):
        """After run(): the training samples of every game, replayed from the device log without a file in between
        (GameplayLoader.load_pool; keep_log / keep_stat, anything that enabled the device log) -> a list per game of Gameplay,
        one per wanted seat, named like the dumped logs name the seats (game.rs:186).  seats: 4-bit seat mask per game;
        augmented: the suit-swapped second pass of the reference's data loader (GameplayLoader.load_pool)."""
        if not getattr(self.pool, "log_cap", 0):
            raise MortalAmdError("gameplays: the device log is off (create the runner with keep_log or keep_stat)")
        return loader.load_pool(self.pool, seats=seats, names=self._seat_names(self.agent_of_seat), augmented=augmented)

    def sample_store(self, loader, seats=None, augmented=False, store=None, capacity=None, batch_rows=1024):
        """After run(): the same samples into a SampleStore (GameplayLoader.store_pool) -- every decision kept as its 2 KB record
        and encoded when a batch draws it, instead of every obs at once.  store: append to this one (successive runs fill one
        buffer); else a new one of `capacity` samples.  -> the store."""
        if not getattr(self.pool, "log_cap", 0):
            raise MortalAmdError("sample_store: the device log is off (create the runner with keep_log or keep_stat)")
        return loader.store_pool(self.pool, seats=seats, names=self._seat_names(self.agent_of_seat), augmented=augmented,
                                 store=store, capacity=capacity, batch_rows=batch_rows)

    @staticmethod
    def _meta(batch, row, tag, with_batch=False):
        """Metadata of one decision (agent/mortal.rs:161-186 gen_meta + :575-591), keys in the order of mjai::Metadata."""
        q, m, greedy, eval_ns = batch
        bits = 0
        for i in np.flatnonzero(m[row]):
            bits |= 1 << int(i)
        meta = {"q_values": [float(x) for x in q[row][m[row]]], "mask_bits": bits, "is_greedy": bool(greedy[row])}
        if with_batch:
            meta["batch_size"] = int(q.shape[0])
            meta["eval_time_ns"] = int(eval_ns)
        meta["shanten"] = tag["shanten"]
        meta["at_furiten"] = tag["at_furiten"]
        return meta

    def dump_logs(self, log_dir, splits):
        """Write one mjai `.json.gz` per game (result.rs:32-51, one_vs_three.rs:195-225); `splits` = files per seed."""
        from . import mjai_log

        os.makedirs(log_dir, exist_ok=True)
        names = self._seat_names(self.agent_of_seat)
        paths = []
        for g, words in enumerate(self.pool.read_logs()):
            tags = []
            events = mjai_log.decode_events(words, tags)
            for ev, tag in zip(events, tags):
                if tag is None:
                    continue
                agent = (int(self.agent_of_seat[g]) >> ev.get("actor", 0)) & 1
                batch = self.meta_batches.get(tag["cycle"], {}).get(agent)
                if batch is None:
                    continue  # device-side engine (react_batch_device): no q-values came back to the host
                meta = self._meta(batch, tag["row"], tag, with_batch=True)
                if tag["kan_row"] is not None:
                    meta["kan_select"] = self._meta(batch, tag["kan_row"], tag)
                ev["meta"] = meta
            name = f"{self.seeds[g][0]}_{self.seeds[g][1]}_{'abcd'[g % splits]}.json.gz"
            paths.append(mjai_log.write_game_log_as(os.path.join(log_dir, name), names[g], self.seeds[g], events))
        return paths


class SelfPlayRunner(_EngineRunner):
    """Self-play at full occupancy with the samples out, no files: a pool in refill mode whose finished games are collected on
    the device (TablePool.enable_harvest) while the other tables play on.  The reference loops over play, collect and load
    (mortal/client.py:35, player.py:120-157) and its arena hands each GameResult over as the game finishes
    (arena/game.rs:291-296); here `play` returns a Harvest whenever enough games are in, and `gameplays` / `stats` read it.
    An extension of this engine: the reference has no restarting arena.

    Table t plays seed (seed_start[0] + t + g * nonce_stride, seed_start[1]) and game id t + g * n_tables in its generation g
    (nonce_stride defaults to n_tables: no seed is played twice).  agent_of_seat [n_tables]: bit s = engine of seat s; a table
    keeps its agent_of_seat for every generation it plays.  stagger: the tables enter play spread over that many cycles
    (TablePool.set_start_stagger; a table's first game is then generation 1).  max_games / max_words size the harvest buffer: a
    game that finds it full is dropped and counted (Harvest.dropped), so take often enough.

    A table in error does not raise: its game is reported through its record (err, no words) and the table restarts like any
    other -- a long run must survive one bad answer.  Engines that answer with mjai events are refused."""

    def __init__(self, engines, n_tables, seed_start, agent_of_seat=None, *, nonce_stride=None, stagger=0, max_games, max_words,
                 deal_algo=None, device=None):
        n = int(n_tables)
        self._open_pool(engines, n, device, deal_algo)
        try:
            if self.any_mjai_log:
                raise ValueError("SelfPlayRunner: engines that answer with mjai events (engine_type 'mjai-log') are not supported: "
                                 "they are told about every game's start and end one by one, which a restarting pool does not do; "
                                 "use BatchRunner")
            self.seeds = [(int(seed_start[0]) + t, int(seed_start[1])) for t in range(n)]
            self.agent_of_seat = np.zeros(n, dtype=np.uint8) if agent_of_seat is None else np.asarray(agent_of_seat, dtype=np.uint8)
            if self.agent_of_seat.shape != (n,):
                raise ValueError(f"agent_of_seat: expected {n} masks, got shape {self.agent_of_seat.shape}")
            self.nonce_stride = n if nonce_stride is None else int(nonce_stride)
            if self.nonce_stride <= 0:
                raise ValueError("nonce_stride must be positive")
            self.pool.enable_log()
            self.pool.reset(self.seeds, game_ids=np.arange(n), agent_of_seat=self.agent_of_seat, n_games_total=n)
            self._configure_agents()
            self.pool.set_refill(self.nonce_stride)
            if stagger:
                self.pool.set_start_stagger(int(stagger))
            self.pool.enable_harvest(int(max_games), int(max_words))
        except BaseException:
            self.pool.close()
            raise
        self.cycles = 0
        self.keep_log = False
        self._acts, self._qs = [None, None], [None, None]

    def play(self, min_games, max_cycles=None, on_step=None, check_every=16):
        """Step until at least min_games finished games are collected, then take them -> Harvest (the caller closes it; games
        that finish later are in the next one).  The count of collected games costs a copy from the device and a stream
        synchronise, so it is read every check_every cycles only: the harvest may hold the few games more that finished in
        between.  max_cycles bounds this call.  on_step(runner) is called after every step."""
        pool = self.pool
        start = self.cycles
        check_every = max(1, int(check_every))
        while (self.cycles - start) % check_every or pool.harvest_pending()["games"] < min_games:
            if max_cycles is not None and self.cycles - start >= max_cycles:
                raise MortalAmdError(f"play: max_cycles exceeded with {pool.harvest_pending()['games']} of {min_games} games collected")
            n = pool.step(self._acts[0], self._acts[1], self._qs[0], self._qs[1])
            self.cycles += 1
            if on_step is not None:
                on_step(self)
            self._acts, self._qs = [None, None], [None, None]
            for a in (0, 1):
                if n[a]:
                    self._acts[a], self._qs[a], _ns = self._answer(a, n[a])
        pool.check_sp_overflow()
        return pool.take_harvest()

    def _names(self, harvest):
        return self._seat_names(harvest.games["agent_of_seat"])

    def gameplays(self, loader, harvest, seats=None, augmented=False):
        """The training samples of every game of the harvest (GameplayLoader.load_harvest) -> a list per game of Gameplay, one per
        wanted seat, the seats named by engine as BatchRunner.gameplays names them.  seats: 4-bit seat mask per game; augmented:
        the suit-swapped form of the same games."""
        return loader.load_harvest(harvest, seats=seats, names=self._names(harvest), augmented=augmented)

    def sample_store(self, loader, harvest, seats=None, augmented=False, store=None, capacity=None, batch_rows=1024):
        """The games of the harvest into a SampleStore (GameplayLoader.store_harvest), named as gameplays names them.  store:
        append to this one -- the replay buffer that successive harvests fill; else a new one of `capacity` samples."""
        return loader.store_harvest(harvest, seats=seats, names=self._names(harvest), augmented=augmented, store=store,
                                    capacity=capacity, batch_rows=batch_rows)

    def stats(self, harvest):
        """{engine name: Stat} over the games of the harvest (games in error are left out)."""
        totals, _rows, counts = harvest.stat()
        if counts["malformed"]:
            raise MortalAmdError(f"stats: {counts['malformed']} malformed logs")
        return _stats_by_name([c["name"] for c in self.cfg], [t.counters() for t in totals])


def _stats_by_name(names, agent_counters):
    """Per-agent counters -> {engine name: Stat}; a single engine plays both agents' seats."""
    from .stat import Stat

    names = list(names) * 2 if len(names) == 1 else list(names)
    out = {}
    for name, c in zip(names, agent_counters):
        out[name] = out.get(name, Stat()) + Stat.from_counters(c)
    return out


def _reduce_device(backend, dev):
    """Where a collective's tensor lives: the pool's GPU under nccl (the current one for a rank without games), else the host."""
    if backend != "nccl":
        return torch.device("cpu")
    return dev if dev is not None else torch.device(f"cuda:{torch.cuda.current_device()}")


def _rank_by_player(scores):
    """rankings.rs:8-21: stable sort by -score; ties favour the lower seat."""
    order = sorted(range(4), key=lambda i: -int(scores[i]))
    rank = [0] * 4
    for r, pid in enumerate(order):
        rank[pid] = r
    return rank


class _PyVsPy:
    """What OneVsThree and TwoVsTwo share: the options, and playing one rank's games with a BatchRunner."""

    def __init__(self, *, disable_progress_bar=False, log_dir=None, deal_algo=None, collect_stat=False):
        self.disable_progress_bar = disable_progress_bar
        self.log_dir = log_dir
        self.deal_algo = deal_algo  # None = pool.default_deal_algo() (rand 0.9.1 unless MORTAL_AMD_DEAL_ALGO says otherwise)
        # our extension: py_vs_py leaves {engine name: Stat} of the whole run in self.stats, counted on the device -- what
        # Stat.from_dir(log_dir, name) computes from the dumped files (mortal/player.py:62-71), without writing or reading them
        self.collect_stat = collect_stat
        self.stats = None

    def _play(self, challenger, champion, seeds, aos, progress, splits):
        """This rank's games -> (scores, [Stat counters of the challenger's seats, of the champion's] (zeros unless collect_stat),
        the pool's device); the logs are dumped, `splits` files per seed, when log_dir is set.  No games: (None, zeros, None)."""
        counters = [[0] * 44, [0] * 44]
        if not seeds:
            return None, counters, None
        runner = BatchRunner([challenger, champion], seeds, aos, keep_log=self.log_dir is not None, deal_algo=self.deal_algo,
                             keep_stat=self.collect_stat)
        try:
            scores = runner.run(progress=None if self.disable_progress_bar else progress)
            if self.collect_stat:
                counters = [t.counters() for t in runner.agent_stats()]
            if self.log_dir is not None:
                runner.dump_logs(self.log_dir, splits)
        finally:
            runner.close()
        return scores, counters, runner.device


class OneVsThree(_PyVsPy):
    """libriichi.arena.OneVsThree (arena/one_vs_three.rs:17-113)."""

    def py_vs_py(self, challenger, champion, seed_start, seed_count):
        """Returns the rank histogram [1st, 2nd, 3rd, 4th] of the challenger over seed_count*4 hanchan."""
        from . import sharding

        n = int(seed_count) * 4
        # One process per GPU (torch.distributed initialised, e.g. under torchrun): rank r plays the contiguous game range
        # [g0, g1) — multiples of 4, so the four seat rotations of a seed stay together — with its own pool and its own
        # copy of the engines; the only collective is the all-reduce of the 4-entry rank histogram,
        # so every rank returns the reference's whole-run result (one_vs_three.rs:55-60 sums it in-process).
        rank, world, backend = sharding.dist_info()
        g0, g1 = sharding.shard_range(n, rank, world) if world > 1 else (0, n)
        seeds = [(int(seed_start[0]) + g // 4, int(seed_start[1])) for g in range(g0, g1)]  # one_vs_three.rs:140-142
        # challenger (agent 0) sits at seat g % 4, the champion (agent 1) on the other three (one_vs_three.rs:144-191)
        aos = np.array([0xF & ~(1 << (g % 4)) for g in range(g0, g1)], dtype=np.uint8)
        rankings = [0, 0, 0, 0]
        scores, counters, dev = self._play(challenger, champion, seeds, aos, f"rank {rank}" if world > 1 else "", 4)
        for i, g in enumerate(range(g0, g1)):
            rankings[_rank_by_player(scores[i])[g % 4]] += 1  # one_vs_three.rs:55-60
        if world > 1:
            red_dev = _reduce_device(backend, dev)
            rankings = sharding.allreduce_rank_histogram(rankings, device=red_dev)
            if self.collect_stat:
                flat = sharding.allreduce_counters(counters[0] + counters[1], device=red_dev)
                counters = [flat[:44], flat[44:]]
        if self.collect_stat:
            self.stats = _stats_by_name([_check_engine(e)["name"] for e in (challenger, champion)], counters)
        return rankings

    def ako_vs_py(self, engine, seed_start, seed_count):
        raise NotImplementedError("akochan agents are out of scope (SURVEY.md §2 row 2)")

    def py_vs_ako(self, engine, seed_start, seed_count):
        raise NotImplementedError("akochan agents are out of scope (SURVEY.md §2 row 2)")


class TwoVsTwo(_PyVsPy):
    """libriichi.arena.TwoVsTwo (arena/two_vs_two.rs:17-110): seed_count*2 hanchan, returns None."""

    def py_vs_py(self, challenger, champion, seed_start, seed_count):
        from . import sharding

        n = int(seed_count) * 2
        rank, world, backend = sharding.dist_info()  # one process per GPU: contiguous seed ranges; only collect_stat reduces
        g0, g1 = sharding.shard_range(n, rank, world, group=2) if world > 1 else (0, n)
        seeds = [(int(seed_start[0]) + g // 2, int(seed_start[1])) for g in range(g0, g1)]  # two_vs_two.rs:138-140
        # split A: challenger at seats 0,2; split B: 1,3 (two_vs_two.rs:142-172)
        aos = np.array([0b1010 if g % 2 == 0 else 0b0101 for g in range(g0, g1)], dtype=np.uint8)
        scores, counters, dev = self._play(challenger, champion, seeds, aos, "", 2)
        if scores is not None:
            self.last_scores = scores
        if self.collect_stat:
            if world > 1:
                flat = sharding.allreduce_counters(counters[0] + counters[1], device=_reduce_device(backend, dev))
                counters = [flat[:44], flat[44:]]
            self.stats = _stats_by_name([_check_engine(e)["name"] for e in (challenger, champion)], counters)
        return None

    def ako_vs_py(self, *a, **k):
        raise NotImplementedError("akochan agents are out of scope")

    py_vs_ako = py_vs_ako_one = ako_vs_py


__all__ = ["OneVsThree", "TwoVsTwo", "BatchRunner", "ACTION_SPACE", "OBS_ROWS"]
