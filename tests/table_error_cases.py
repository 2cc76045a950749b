"""Shared by tests/test_emu_table_errors.py (host emulation of the device code), tests/test_gpu_table_errors.py (the real library)
and tests/test_table_error_plan.py / tools/find_table_error_plan.py (the oracle alone): tables driven into an ERROR CODE, and
what the rest of the pool must not notice.

The plan (tests/golden/table_error_plan.json) names, per run, the decisions that get a poisoned answer: (table, cycle, seat, row
kind, value).  The device pool and the oracle arena play the same seeds under the same counter-based policy
(oracle_lib.random_actions, keyed by game, seat, row kind and cycle -- not by row index, so it survives a shifting row list).  On
an entry's cycle the device gets the poisoned value for that row, the oracle gets the policy's legal one and keeps playing that
game; from the next cycle on the victim's rows are taken out of the oracle's list and the device's list must equal the rest.

Pinned behaviour (mj_step.hip): a table in error ends in the step that decodes the bad answer: err keeps its FIRST code, the table
contributes no row afterwards, mj_results' done flag is 2, counters()["errors"] counts it -- and so does counters()["games"]: the
close path bumps the games counter for every table that leaves play, errored or not (a driver that waits for `games` to reach the
number of tables terminates even when a table died).

Every value is a plain int32 answer; decode_action (mj_step.hip) treats it with compares only and never indexes by it.  Three
kinds are no action id.  `reaction_word` (run "words", tsumogiri policy): every row is answered through mj_step_ev with an event
word, one of them the discard of a tile the seat does not hold, which reaction_from_word refuses after bounding the tile id.
`guard_q_nan` / `guard_q_neg_inf` (run "guard", greedy policy, rule-based agari guard on): a legal 43 that rule_based_agari
rejects meets a q row of NaN -- total_cmp's maximum is the last index, 45, an error on a tsumo row; the device alone gets it --
or of -inf -- q[43] = f32::MIN stays the maximum, so the agari is played after all; both sides get it, nobody dies, and the
hora must show in the log.  The q-values are only compared, never used as an index.  Every comparison here is exact
(integers, f32 bit patterns); event logs are compared in full, event for event, for tables in mid-game too."""
import json
import os

import numpy as np
import pytest
import torch

import parity_util
from mortal_amd import mjai_log
from mortal_amd._lib import MortalAmdError

PLAN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_error_plan.json")
POLICY_SEED = 0x9E3779B97F4A7C15
INT32_MIN = -(2 ** 31)
FIXED = dict(riichi_without_can=37, chi_on_own_turn=39, pon_on_own_turn=41, pon_on_chi_only=41, kan_none=42, agari_none=43,
             ryukyoku_none=44, pass_own_turn=45, id_46=46, id_1000=1000, id_minus1=-1, id_int_min=INT32_MIN, kan_select_34=34)
GUARD_KINDS = {"guard_q_nan": "nan", "guard_q_neg_inf": "-inf"}  # the kind's q row; the answer itself is the policy's 43
KINDS = ("discard_not_in_hand", "red_five_plain_only") + tuple(FIXED) + ("kan_select_not_candidate", "reaction_word") + tuple(GUARD_KINDS)
KAN_KINDS = ("kan_select_not_candidate", "kan_select_34")
OWN_TURN_KINDS = ("discard_not_in_hand", "red_five_plain_only", "chi_on_own_turn", "pon_on_own_turn", "pass_own_turn", "reaction_word",
                  "guard_q_nan")
SURVIVES = ("guard_q_neg_inf",)  # the one kind that kills nobody (see run_poisoned)


def plan():
    with open(PLAN_PATH) as f:
        return json.load(f)


def dahai_word(seat, tile, tsumogiri):
    """The explicit reaction word (mj_step_ev) of a discard."""
    from mortal_amd.arena import pack_reaction

    return pack_reaction(dict(type="dahai", actor=int(seat), pai=mjai_log.TILE_NAMES[int(tile)], tsumogiri=bool(tsumogiri)))


def poisoned_value(kind, mask, is_kan, snapshot, seat=0):
    """The value the kind puts on a row with this mask, or None where the kind does not apply.  `snapshot`: () -> the oracle's
    PlayerState.snapshot() of the row's seat (only the hand kinds look at it).  Whatever is returned is no legal answer of
    the row: its mask bit is clear, or it lies outside 0..45.  Two kinds are no action id: `reaction_word` is the event word of
    a discard of a tile the seat does not hold (the run answers every row with a word), and a guard kind is the content of the
    row's q-values ("nan" / "-inf") under a legal answer of 43 that rule_based_agari rejects (`applies` checks that part)."""
    m = np.asarray(mask, dtype=bool)
    if is_kan != (kind in KAN_KINDS):
        return None
    own_turn = bool(m[:37].any()) and not is_kan
    if kind in OWN_TURN_KINDS and not own_turn:
        return None
    if kind in GUARD_KINDS:
        return GUARD_KINDS[kind] if m[43] else None
    if kind in ("discard_not_in_hand", "reaction_word"):
        absent = np.flatnonzero(np.asarray(snapshot()["tehai"]) == 0)
        v = int(absent[0]) if len(absent) else None
        if kind == "reaction_word":
            return None if v is None or m[v] else dahai_word(seat, v, False)
    elif kind == "red_five_plain_only":
        sn = snapshot()
        ks = [k for k in range(3) if sn["tehai"][4 + 9 * k] > 0 and not sn["akas_in_hand"][k]]
        v = 34 + ks[0] if ks else None
    elif kind == "kan_select_not_candidate":
        v = int(np.flatnonzero(~m[:34])[0])
    elif kind == "pon_on_chi_only":
        v = 41 if m[38:41].any() else None
    else:
        v = FIXED[kind]
    if v is not None and 0 <= v < 46 and m[v]:
        return None
    return v


def applies(entry, arena, rows, masks, act):
    """-> index of the entry's row in `rows` if the entry applies on this cycle (the row exists, the kind's condition holds and
    gives the recorded value; a kan-select answer only matters under a main-row answer of 42), else None."""
    hit = np.flatnonzero((rows[:, 0] == entry["table"]) & (rows[:, 1] == entry["seat"]) & (rows[:, 2] == int(entry["row"] == "kan")))
    if len(hit) != 1:
        return None
    r = int(hit[0])
    is_kan = entry["row"] == "kan"
    v = poisoned_value(entry["kind"], masks[r], is_kan, lambda: arena.player_state(entry["table"], entry["seat"]).snapshot(), entry["seat"])
    if v is None or v != entry["value"]:
        return None
    if entry["kind"] in GUARD_KINDS and not (act[r] == 43 and not arena.player_state(entry["table"], entry["seat"]).call(2)):
        return None  # (PlayerState call 2 = rule_based_agari: the guard steps in where it says no)
    if is_kan and not (r + 1 < len(rows) and tuple(rows[r + 1]) == (entry["table"], entry["seat"], 0) and act[r + 1] == 42):
        return None
    return r


def kyoku_ids(arena, n):
    """(kyoku, honba) of every game: it changes in the poll that deals the game's next kyoku."""
    return [tuple(int(x) for x in arena.game_view(g)[1:3]) for g in range(n)]


def by_cycle(entries):
    out = {}
    for e in entries:
        out.setdefault(e["cycle"], []).append(e)
    return out


def _greedy(arena, masks, rows, cycle, obs):
    d0 = parity_util.DISCARD_ROW[3]
    return parity_util.greedy_actions(masks, rows, cycle, obs[:, d0:d0 + 3] if len(rows) else obs, POLICY_SEED)


def policy_actions(oracle, run, arena, rows, masks, cycle, obs):
    """The run's policy on the oracle's batch: "random" (oracle_lib.random_actions, the default), "greedy" (it takes every
    agari it is offered: the guard run; needs the obs) or "tsumogiri" (the run that answers with reaction words)."""
    pol = run.get("policy", "random")
    if pol == "greedy":
        return _greedy(arena, masks, rows, cycle, obs)
    if pol == "tsumogiri":
        return parity_util.tsumogiri_actions(arena, masks, rows) if len(rows) else np.zeros(0, dtype=np.int32)
    return oracle.random_actions(masks, rows, cycle, seed=POLICY_SEED)


def replay_oracle_alone(oracle, run, on_cycle=None):
    """The run on the oracle alone (nobody is poisoned: on the oracle every game plays on) -> number of entries that apply, and
    of `deal_neighbour` claims that hold (a table of the victim's block of 64 is dealt a kyoku in the poll that follows the
    poisoned answer: the step that decodes the bad answer also serves that deal)."""
    n = run["n_tables"]
    arena = oracle.Arena(parity_util.default_seeds(n), deal_algo=0, enable_quick_eval=run["quick_eval"], version=3, keep_log=False)
    todo = by_cycle(run["entries"])
    fired = deals = 0
    watch, before = [], None
    for cycle in range(max(todo) + 2 if todo else 0):
        rows = arena.poll()
        if watch:
            after = kyoku_ids(arena, n)
            deals += sum(1 for e in watch if after[e["deal_neighbour"]] != before[e["deal_neighbour"]])
        obs, masks = arena.encode(0, len(rows), want_obs=run.get("policy") == "greedy")
        act = policy_actions(oracle, run, arena, rows, masks, cycle, obs)
        q = parity_util.fake_q_values(masks, rows, cycle, POLICY_SEED) if run.get("guard") else None
        if on_cycle:
            on_cycle(cycle, arena, rows, masks, act)
        for e in todo.get(cycle, ()):
            r = applies(e, arena, rows, masks, act)
            fired += r is not None
            if r is not None and e["kind"] in SURVIVES:
                q[r] = -np.inf  # (the oracle gets this row too: the game goes on from the agari it then plays)
        watch = [e for e in todo.get(cycle, ()) if e.get("deal_neighbour") is not None]
        if watch:
            before = kyoku_ids(arena, n)
        arena.commit(act, q)
    return fired, deals


def _dump(e):
    return json.dumps(e, separators=(",", ":"))


def _assert_logs_agree(got, want, what):
    """Event for event, in full.  Also for a table in mid-game: both sides have polled the same number of times, and events are
    logged by the poll alone (the oracle's commit only stores the reactions)."""
    a, b = [_dump(e) for e in got], [_dump(e) for e in want]
    if a != b:
        k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
        raise AssertionError(f"{what}: event {k} differs:\n oracle {b[k] if k < len(b) else None}\n device {a[k] if k < len(a) else None}")
    return len(a)


def run_poisoned(oracle, pool_cls, run, n_tables=None, version=3, tail=300, obs_cycles=(), sp_rows_checked=False,
                 to_completion=False, check_log_stat=False):
    """The poisoned lock-step.  n_tables < run["n_tables"]: the sub-plan whose victims fit (default_seeds(n) is a prefix of
    default_seeds(run's n) and games do not interact: the first n tables play the same games).  Runs `tail` cycles past the last
    entry, or to the end of every hanchan.  -> dict of counts; AssertionError on the first difference."""
    n = n_tables or run["n_tables"]
    entries = [e for e in run["entries"] if e["table"] < n]
    todo = by_cycle(entries)
    last = max(todo)
    seeds = parity_util.default_seeds(n)
    qe = run["quick_eval"]
    guard, words, greedy = bool(run.get("guard")), bool(run.get("words")), run.get("policy") == "greedy"
    lethal = [e for e in entries if e["kind"] not in SURVIVES]
    arena = oracle.Arena(seeds, deal_algo=0, enable_quick_eval=qe, version=version, keep_log=True)
    pool = pool_cls(n, version=version, deal_algo=0)
    try:
        pool.enable_log()
        pool.reset(seeds, game_ids=np.arange(n), n_games_total=n)
        for a in (0, 1):
            pool.configure(a, enable_quick_eval=qe, enable_rule_based_agari_guard=guard)
        n_cmp = pool.C if (version != 4 or sp_rows_checked) else 889
        dead, dying, frozen_len = [], [], {}
        fired = exp_steps = prev_steps = obs_checked = rows_total = neighbour_rows = 0
        actions = q_dev = ev_dev = None
        agari_due = []  # (table, seat, events the oracle had logged): a SURVIVES entry of the previous cycle
        lens = np.zeros(n, dtype=np.uint32)
        for cycle in range(100000 if to_completion else last + tail + 1):
            pool.step(actions, None, q_dev, None, ev_dev, None)
            rows_g = pool.rows(0)
            dev = pool.counters()
            assert pool._L.mj_log_lengths(pool.h, lens.ctypes.data, pool._stream()) == 0
            for t in dying:  # poisoned on the previous cycle: the step that has just run decoded the answer
                dead.append(t)
                frozen_len[t] = int(lens[t])
            dying = []
            rows_o = arena.poll()
            for t, seat, k in agari_due:  # the -inf row: q[43] = f32::MIN beats it, the agari the guard rejected is played
                new = arena.log(t)[k:]
                assert any(e["type"] == "hora" and e["actor"] == seat for e in new), (cycle, t, seat, new[:4])
            agari_due = []
            keep = ~np.isin(rows_o[:, 0], dead) if len(rows_o) else np.zeros(0, dtype=bool)
            want_rows = rows_o[keep]
            if len(want_rows) != len(rows_g) or not (want_rows == rows_g).all():
                k = next((i for i in range(min(len(want_rows), len(rows_g))) if not (want_rows[i] == rows_g[i]).all()),
                         min(len(want_rows), len(rows_g)))
                raise AssertionError(f"cycle {cycle}: row lists differ at index {k}: oracle without the victims "
                                     f"{want_rows[k] if k < len(want_rows) else None}, device {rows_g[k] if k < len(rows_g) else None} "
                                     f"(n {len(want_rows)} / {len(rows_g)}; dead {dead}; device error {pool.first_error()})")
            # ---- the victims
            code, first = pool.first_error()
            if dead:
                assert (code, first) == (1, min(dead)), (cycle, code, first, dead)
                _, done = pool.results()
                assert (done[dead] == 2).all() and not np.isin(rows_g[:, 0], dead).any(), (cycle, dead)
                for t in dead:
                    dbg = pool.debug_table(t)
                    assert int(dbg["pending"][0]) == 0 and int(dbg["err"][0]) == 1, (cycle, t, dbg["pending"], dbg["err"])
                    assert int(lens[t]) == frozen_len[t], (cycle, t, int(lens[t]), frozen_len[t])
            else:
                assert code == 0, (cycle, code, first)
            assert dev["errors"] == len(dead), (cycle, dev, dead)
            # ---- the neighbours
            n_o = len(rows_o)
            if n_o == 0 and arena.n_live == 0:
                break
            n_g = len(rows_g)
            obs_g = torch.full((n_g, pool.C, 34), float("nan"), dtype=torch.float32, device=pool.device)
            masks_g = torch.ones((n_g, 46), dtype=torch.bool, device=pool.device)
            obs_g, masks_g = pool.encode(0, obs_g, masks_g)
            want_obs = cycle in obs_cycles
            obs_o, masks_o = arena.encode(0, n_o, want_obs=want_obs or greedy)
            mg = masks_g.cpu().numpy().astype(np.uint8)
            if not (mg == masks_o[keep]).all():
                r = int(np.argwhere((mg != masks_o[keep]).any(axis=1))[0][0])
                raise AssertionError(f"cycle {cycle}: mask mismatch at row {r} {rows_g[r]}: oracle {np.flatnonzero(masks_o[keep][r]).tolist()} "
                                     f"device {np.flatnonzero(mg[r]).tolist()}")
            if want_obs and n_g:
                a = np.ascontiguousarray(obs_g.cpu().numpy()[:, :n_cmp]).view(np.uint32)
                b = np.ascontiguousarray(obs_o[keep][:, :n_cmp]).view(np.uint32)
                bad = np.argwhere(a != b)
                assert bad.size == 0, f"cycle {cycle}: obs mismatch at row {rows_g[bad[0][0]]}, obs rows {sorted(set(int(x[1]) for x in bad))[:20]}"
                obs_checked += n_g
            rows_total += n_g
            blocks_hit = {t >> 6 for t in dead}
            neighbour_rows += int(np.isin(rows_g[:, 0] >> 6, list(blocks_hit)).sum()) if blocks_hit else 0
            # ---- answers: the policy's everywhere, except the poisoned value on the device's copy of a plan row
            act = policy_actions(oracle, run, arena, rows_o, masks_o, cycle, obs_o)
            act_dev = np.ascontiguousarray(act[keep], dtype=np.int32)
            q = parity_util.fake_q_values(masks_o, rows_o, cycle, POLICY_SEED) if guard else None
            if words:  # every row answered with an event word: the discard the policy chose (the tile just drawn), or none
                ev = np.array([dahai_word(rows_o[r, 1], act[r], True) if act[r] < 37 else 0 for r in np.flatnonzero(keep)], dtype=np.int64)
            nan_rows = []
            for e in todo.get(cycle, ()):
                r = applies(e, arena, rows_o, masks_o, act)
                if r is None or e["table"] in dead or e["table"] in dying:
                    continue  # (counted: every caller asserts fired == len(entries))
                fired += 1
                if e["kind"] in SURVIVES:  # both sides get the row of -inf
                    q[r] = -np.inf
                    agari_due.append((e["table"], e["seat"], len(arena.log(e["table"]))))
                    continue
                if e["kind"] in GUARD_KINDS:  # the device alone gets the row of NaN: its maximum is the last index, 45
                    nan_rows.append(int(keep[:r].sum()))
                elif words:
                    ev[int(keep[:r].sum())] = e["value"]
                else:
                    act_dev[int(keep[:r].sum())] = e["value"]
                dying.append(e["table"])
            arena.commit(act, q)
            if guard:
                qd = np.ascontiguousarray(q[keep])
                qd[nan_rows] = np.nan
                q_dev = torch.from_numpy(qd).to(pool.device)
            actions = None if words else torch.from_numpy(act_dev).to(pool.device)
            ev_dev = torch.from_numpy(ev).to(pool.device) if words else None
            # ---- counters: the device's after its step k == the oracle's after its commit k, less the games only the oracle still plays
            done_o = arena.done_flags() != 0
            exp_steps += int(arena.steps) - prev_steps - sum(1 for t in dead if not done_o[t])
            prev_steps = int(arena.steps)
            assert dev["steps"] == exp_steps, (cycle, dev["steps"], exp_steps)
            assert dev["games"] == len(dead) + int(np.delete(done_o, dead).sum()), (cycle, dev["games"], dead)
        assert fired == len(entries), f"{fired} of {len(entries)} plan entries fired"
        assert len(dead) == len(lethal) and not dying and not agari_due
        # ---- the end of the run: scores and logs of everybody else; a victim's log is what the oracle logged up to the bad answer
        scores_g, done_g = pool.results()
        done_o = arena.done_flags() != 0
        alive = np.setdiff1d(np.arange(n), dead)
        assert ((done_g[alive] == 1) == done_o[alive]).all()
        fin = alive[done_o[alive]]
        assert all((scores_g[g] == arena.result(int(g))[0]).all() for g in fin), "final scores differ"
        if to_completion:
            assert len(fin) == len(alive)
        with_error = None
        try:
            logs = pool.read_logs()
        except MortalAmdError as e:
            with_error = e
        assert with_error is None, with_error
        n_ev = 0
        device_logs = []
        for g in range(n):
            got, want = mjai_log.decode_events(logs[g]), arena.log(g)
            device_logs.append(got)
            if g in dead:
                assert 0 < len(got) <= len(want), (g, len(got), len(want))
                n_ev += _assert_logs_agree(got, want[:len(got)], f"victim {g}")
            else:
                n_ev += _assert_logs_agree(got, want, f"table {g}")
        stats = dict(fired=fired, dead=list(dead), cycles=cycle, rows=rows_total, obs_checked=obs_checked, log_events=n_ev,
                     neighbour_rows=neighbour_rows, scores_checked=len(fin), counters=pool.counters())
        if check_log_stat:
            # TablePool.log_stat: an errored table is skipped like one still playing; the totals are the host Stat of the rest
            import stat_device_cases as S

            want = S.expected([logs[g] for g in fin])
            totals, rows, counts = pool.log_stat(per_seat=True)
            assert counts == dict(reduced=len(fin), skipped=n - len(fin), malformed=0), counts
            assert (rows[fin] == want).all() and not rows[dead].any()
            assert (np.array(totals[0].counters()) == want.sum(axis=(0, 1))).all()
            stats["log_stat"] = counts
        return stats
    finally:
        pool.close()


def check_row_capacity(oracle, pool_cls, n_clean=64):
    """A pool whose row arrays hold 8 rows meets a first batch of one row per table: the step fails with "row capacity exceeded",
    the batch stays invalid -- mj_encode and mj_encode_oracle straight through the C-ABI are refused instead of walking rows[]
    past its allocation, and so is mj_replay_meta after a replay step that overflows a pool of one row --, the pools close, and a normal pool created afterwards in the same process is clean for 50 cycles of lock-step."""
    pool = pool_cls(64, version=3, deal_algo=0, max_rows=8)
    try:
        pool.reset(parity_util.default_seeds(64), game_ids=np.arange(64), n_games_total=64)
        raised = None
        try:
            pool.step()
        except MortalAmdError as e:
            raised = e
        assert raised is not None and "row capacity exceeded" in str(raised)
        obs = torch.zeros((8, pool.C, 34), dtype=torch.float32, device=pool.device)
        masks = torch.zeros((8, 46), dtype=torch.bool, device=pool.device)
        assert pool._L.mj_encode(pool.h, 0, obs.data_ptr(), masks.data_ptr(), pool._stream()) < 0
        assert "mj_rows_count" in pool._L.mj_last_error().decode()
        assert pool._L.mj_encode_oracle(pool.h, 0, obs.data_ptr(), pool._stream()) < 0
        assert not obs.any() and not masks.any()
    finally:
        pool.close()
    assert pool.h is None
    # the replay path: two copies of the example game, every seat tracked, in a pool whose row arrays hold one row
    with open(os.path.join(os.path.dirname(PLAN_PATH), "example_game.jsonl")) as f:
        script = mjai_log.encode_events([json.loads(line) for line in f])
    pool = pool_cls(2, version=3, deal_algo=0, max_rows=1)
    try:
        pool.replay_load([script, script], [15, 15])
        raised = None
        try:
            while pool.replay_step() == 0:  # (the first sample of both tables comes on the same step)
                pass
        except MortalAmdError as e:
            raised = e
        assert raised is not None and "row capacity exceeded" in str(raised)
        meta = torch.zeros((1, 8), dtype=torch.int32, device=pool.device)
        assert pool._L.mj_replay_meta(pool.h, meta.data_ptr(), pool._stream()) < 0
        assert "mj_rows_count" in pool._L.mj_last_error().decode() and not meta.any()
    finally:
        pool.close()
    st = parity_util.run_lockstep(oracle, n_clean, version=3, max_cycles=50, obs_every=10, pool_cls=pool_cls, deal_algo=0, verbose=False)
    assert st["cycles"] == 50 and st["obs_checked"] > 0


def check_error_texts(pool_cls):
    """A call the C side refuses raises MortalAmdError with the text of the library the pool runs on (the host emulation keeps
    its own last-error string, apart from the product library's): a pool of 4 tables, log off, no refill."""
    from mortal_amd.state import PlayerState

    def refused(call):
        with pytest.raises(MortalAmdError) as ex:
            call()
        return str(ex.value)

    pool = pool_cls(4, version=3, deal_algo=0)
    try:
        assert refused(lambda: pool.configure(5)) == "bad agent"
        assert refused(pool.read_logs) == "event log is not enabled"
        assert refused(pool.log_lengths) == "event log is not enabled"
        assert "needs the refill mode" in refused(lambda: pool.set_start_stagger(3))
        assert "mj_pool_stat: the event log is not enabled" in refused(pool.log_stat)
        # state.py's own calls go through the pool's library too.  A view answers from its copy and has no pool to call, so this
        # one is handed the pool it was taken from, and a seat that mj_table_query's argument check refuses
        st = PlayerState.view(pool, 0, 0)
        st._pool, st.player_id = pool, 4
        try:
            assert refused(st.real_time_shanten) == "bad table / seat"
        finally:
            st._pool = None
    finally:
        pool.close()


REFILL_VICTIMS = ((5, 10, "ryukyoku_none"), (20, 14, "id_46"), (63, 14, "discard_not_in_hand"))  # (table, first cycle, kind)


def check_refill_restart(oracle, pool_cls, n=64, stride=8, max_cycles=4000, plan=REFILL_VICTIMS):
    """mj_k_refill restarts a dead table clean.  The tsumogiri policy (its answers do not depend on the cycle number) under
    set_refill; three tables get a bad answer on their first own-turn row at or after the given cycle.  Each must be back on the
    cycle after its death as game t + n on (nonce + stride, key) with err == 0, and from there match -- rows and masks every cycle,
    the log event for event from its first word, the final scores -- a one-table oracle arena started on that seed, while the
    slot's first game keeps done == 2 under its old id.  Everybody else plays (and restarts) as in parity_util.run_lockstep."""
    seeds = parity_util.default_seeds(n)
    arena = oracle.Arena(seeds, deal_algo=0, enable_quick_eval=True, version=3, keep_log=True)
    pool = pool_cls(n, version=3, deal_algo=0)
    try:
        pool.enable_log()
        pool.reset(seeds, game_ids=np.arange(n), n_games_total=4 * n)
        pool.set_refill(stride)
        victims = {t: dict(first=c, kind=k, poisoned=None, side=None) for t, c, k in plan}
        nonce = [int(s[0]) for s in seeds]
        gen = [0] * n
        actions = None
        fired = side_rows = 0
        for cycle in range(max_cycles):
            for t, v in victims.items():
                if v["poisoned"] is not None and cycle == v["poisoned"] + 2:  # died in step poisoned + 1; this step's refill restarts it
                    v["side"] = oracle.Arena([(nonce[t] + stride, parity_util.KEY)], deal_algo=0, enable_quick_eval=True, version=3, keep_log=True)
            pool.step(actions, None)
            rows_g = pool.rows(0)
            gone = [t for t, v in victims.items() if v["poisoned"] is not None and cycle > v["poisoned"]]
            parts = []  # (arena, its rows, its masks, the rows as the device numbers them)
            rows_m = arena.poll()
            keep = ~np.isin(rows_m[:, 0], gone) if len(rows_m) else np.zeros(0, dtype=bool)
            masks_m = arena.encode(0, len(rows_m), want_obs=False)[1]
            act_m = parity_util.tsumogiri_actions(arena, masks_m, rows_m) if len(rows_m) else np.zeros(0, dtype=np.int32)
            want = [rows_m[keep]]
            want_masks = [masks_m[keep]]
            want_act = [act_m[keep]]
            for t, v in victims.items():
                if v["side"] is None:
                    continue
                r = v["side"].poll()
                m = v["side"].encode(0, len(r), want_obs=False)[1]
                a = parity_util.tsumogiri_actions(v["side"], m, r) if len(r) else np.zeros(0, dtype=np.int32)
                v["last"] = (r, a)
                r = r.copy()
                r[:, 0] = t
                want += [r]
                want_masks += [m]
                want_act += [a]
                side_rows += len(r)
            want, want_masks, want_act = np.concatenate(want), np.concatenate(want_masks), np.concatenate(want_act)
            order = np.argsort(want[:, 0], kind="stable")  # the device lists rows by table; within a table both sides go seat by seat
            want, want_masks, want_act = want[order], want_masks[order], np.ascontiguousarray(want_act[order], dtype=np.int32)
            assert len(want) == len(rows_g) and (want == rows_g).all(), (cycle, want[:6].tolist(), rows_g[:6].tolist(), pool.first_error())
            _, masks_g = pool.encode(0)
            assert (masks_g.cpu().numpy().astype(np.uint8) == want_masks).all(), cycle
            _, done = pool.results()
            for t, v in victims.items():
                if v["poisoned"] is None:
                    continue
                dbg = pool.debug_table(t)
                if cycle == v["poisoned"] + 1:
                    assert int(dbg["err"][0]) == 1 and int(dbg["pending"][0]) == 0 and int(dbg["game_id"][0]) == t
                if cycle >= v["poisoned"] + 1:
                    assert done[t] == 2, (cycle, t, done[t])  # the slot's first game, under its old id
                if cycle == v["poisoned"] + 2:
                    assert int(dbg["err"][0]) == 0 and int(dbg["game_id"][0]) == t + n and int(dbg["seed_nonce"][0]) == nonce[t] + stride
                    got = mjai_log.decode_events(pool.read_logs()[t])  # rewound: the log holds the new game from its first word
                    assert got and got[0]["type"] == "start_kyoku"
                    _assert_logs_agree(got, v["side"].log(0), f"restarted table {t}")
            # ---- answers
            for t, v in victims.items():
                if v["poisoned"] is None and cycle >= v["first"]:
                    hit = np.flatnonzero((want[:, 0] == t) & (want[:, 2] == 0) & want_masks[:, :37].any(axis=1))
                    if len(hit):
                        r = int(hit[0])
                        val = poisoned_value(v["kind"], want_masks[r], False, lambda: arena.player_state(t, int(want[r, 1])).snapshot())
                        assert val is not None
                        want_act[r] = val
                        v["poisoned"] = cycle
                        fired += 1
            arena.commit(act_m)
            for t, v in victims.items():
                if v["side"] is not None:
                    v["side"].commit(v["last"][1])
                    if v["side"].done_flags()[0]:  # the slot goes on to its next game, as every finished slot does
                        v.setdefault("result", v["side"].result(0)[0].copy())
                        v.setdefault("log", v["side"].log(0))
                        v["gens"] = v.get("gens", 1) + 1
                        v["side"].restart(0, nonce[t] + v["gens"] * stride)
            actions = torch.from_numpy(want_act).to(pool.device)
            if arena.n_live < n:  # finished slots restart on both sides (the victims' slots only on the device and their side arenas)
                for g in np.flatnonzero(arena.done_flags() != 0).tolist():
                    if g not in victims or victims[g]["poisoned"] is None:
                        gen[g] += 1
                        nonce[g] += stride
                        arena.restart(g, nonce[g])
            if fired == len(victims) and all("result" in v for v in victims.values()):
                break
        assert fired == len(victims) == len(plan) and max(victims) < n
        pool.step(actions, None)  # (the device closes a game in the step after the oracle's last commit)
        scores, done = pool.results()
        for t, v in victims.items():
            assert done[t] == 2 and done[t + n] == 1 and (scores[t + n] == v["result"]).all(), (t, done[t], done[t + n])
        return dict(fired=fired, cycles=cycle, side_rows=side_rows)
    finally:
        pool.close()


# ---------------------------------------------------------------- log overflow (MJ_ERR_LOG_OVERFLOW = 7)
OVERFLOW_CYCLES = 130
_REACTIONS = ("dahai", "chi", "pon", "daiminkan", "kakan", "ankan", "reach", "hora")
_forecast = {}


def overflow_forecast(oracle, n, cycles=OVERFLOW_CYCLES):
    """The oracle alone under the greedy policy -> per table the words the device must log (the oracle's events through
    mjai_log.encode_events; an agent's reaction that came from a policy row carries the tag bit and one tag word, whose position
    is returned and whose content is not compared), the number of words logged up to and including each cycle's poll, the index
    of each event's first word and whether the table has a policy row on each cycle.  Cached per (n, cycles)."""
    if (n, cycles) in _forecast:
        return _forecast[(n, cycles)]
    L = oracle.lib()
    arena = oracle.Arena(parity_util.default_seeds(n), deal_algo=0, enable_quick_eval=True, version=3, keep_log=True)
    n_ev = np.zeros((cycles, n), dtype=np.int64)
    row_seats = []
    for cycle in range(cycles):
        rows = arena.poll()
        n_ev[cycle] = [L.mjo_arena_log(arena.h, g, None, 0) for g in range(n)]
        row_seats.append({(int(g), int(s)) for g, s, k in rows if not k})
        obs, masks = arena.encode(0, len(rows), want_obs=True)
        arena.commit(_greedy(arena, masks, rows, cycle, obs))
    out = []
    for g in range(n):
        events = arena.log(g)[:int(n_ev[-1, g])]
        words, tag_pos, first, cum = [], [], [], np.zeros(cycles, dtype=np.int64)
        c = 0
        for i, e in enumerate(events):
            while i >= n_ev[c, g]:
                cum[c] = len(words)
                c += 1
            w = [int(x) for x in mjai_log.encode_events([e])]
            first.append(len(words))
            if e["type"] in _REACTIONS and c > 0 and (g, e["actor"]) in row_seats[c - 1]:  # the answer of a policy row of the cycle before
                tag_pos.append(len(words) + 1)
                w = [w[0] | (1 << 43), 0] + w[1:]
            words += w
        cum[c:] = len(words)
        out.append(dict(words=np.array(words, dtype=np.uint64), tag_pos=np.array(tag_pos, dtype=np.int64), first=first, events=events,
                        cum=cum, has_row=np.array([any(gg == g for gg, _ in row_seats[k]) for k in range(cycles)])))
    _forecast[(n, cycles)] = out
    return out


def overflow_profile(fc, cap):
    """Per table of a forecast: the cycle in which word `cap` is logged (None: never), whether `cap` cuts a hora / ryukyoku
    event behind its header, and whether the table still gets a policy row in that cycle's poll (it then lives one cycle more
    with its code latched)."""
    out = []
    for t in fc:
        over = np.flatnonzero(t["cum"] > cap)
        if not len(over):
            out.append(dict(cycle=None, inside=False, lingers=False))
            continue
        k = int(over[0])
        i = int(np.searchsorted(t["first"], cap, side="right")) - 1  # the event word `cap` belongs to
        out.append(dict(cycle=k, inside=t["events"][i]["type"] in ("hora", "ryukyoku") and t["first"][i] < cap,
                        lingers=bool(t["has_row"][k]) and t["events"][i]["type"] == "tsumo" and i == len([f for f in t["first"] if f < t["cum"][k]]) - 1))
    return out


def check_log_overflow(oracle, pool_cls, n, cap):
    """Every table's log overflows its `cap` words, at its own cycle.  Until the cycle the forecast names, a table's rows and
    masks are the oracle's; on that cycle it may still show its rows (the overflow fell into the last board step of the poll:
    the code is latched, the table ends in the next step) -- those rows are answered with id 46, and the table's code must stay
    the FIRST one, 7 --; afterwards it has none.  At the end: code 7 everywhere, mj_log_lengths above the capacity, read_logs
    raises, and words [0, cap) of every table are the oracle's (a table that wrote past its region would have landed in the
    first words of the next table's)."""
    fc = overflow_forecast(oracle, n)
    prof = overflow_profile(fc, cap)
    assert all(p["cycle"] is not None and p["cycle"] < OVERFLOW_CYCLES - 3 for p in prof)
    assert len({p["cycle"] for p in prof}) >= 8 and any(p["inside"] for p in prof) and any(p["lingers"] for p in prof)
    over_at = np.array([p["cycle"] for p in prof])
    seeds = parity_util.default_seeds(n)
    arena = oracle.Arena(seeds, deal_algo=0, enable_quick_eval=True, version=3, keep_log=False)
    pool = pool_cls(n, version=3, deal_algo=0)
    try:
        pool.enable_log(cap)
        pool.reset(seeds, game_ids=np.arange(n), n_games_total=n)
        actions = None
        lingered = 0
        for cycle in range(int(over_at.max()) + 3):
            pool.step(actions, None)
            rows_g = pool.rows(0)
            rows_o = arena.poll()
            obs_o, masks_o = arena.encode(0, len(rows_o), want_obs=True)
            act = _greedy(arena, masks_o, rows_o, cycle, obs_o)
            before = over_at[rows_o[:, 0]] > cycle if len(rows_o) else np.zeros(0, dtype=bool)
            on_it = over_at[rows_o[:, 0]] == cycle if len(rows_o) else np.zeros(0, dtype=bool)
            key = lambda r: (int(r[0]), int(r[1]), int(r[2]))
            got = {key(r) for r in rows_g}
            must = {key(r) for r in rows_o[before]}
            may = {key(r) for r in rows_o[on_it]}
            assert must <= got <= must | may, (cycle, sorted(got - must - may)[:4], sorted(must - got)[:4])
            for t in {k[0] for k in may}:  # a table keeps all of its rows or none
                mine = {k for k in may if k[0] == t}
                assert mine <= got or not (mine & got), (cycle, t)
            index = {key(r): i for i, r in enumerate(rows_o)}
            pick = np.array([index[key(r)] for r in rows_g], dtype=np.int64)
            _, masks_g = pool.encode(0)
            assert (masks_g.cpu().numpy().astype(np.uint8) == masks_o[pick]).all(), cycle
            act_dev = np.ascontiguousarray(act[pick], dtype=np.int32)
            late = on_it[pick] & (rows_g[:, 2] == 0) if len(pick) else np.zeros(0, dtype=bool)
            act_dev[late] = 46  # a second error on a table whose first code is already latched
            lingered += len({int(t) for t in rows_g[late, 0]})
            arena.commit(act)
            actions = torch.from_numpy(act_dev).to(pool.device)
        assert lingered >= 1
        pool.step(actions, None)
        assert len(pool.rows(0)) == 0
        cnt = pool.counters()
        assert cnt["errors"] == n and cnt["games"] == n, cnt
        assert pool.first_error() == (7, 0)
        for t in range(n):
            assert int(pool.debug_table(t)["err"][0]) == 7, (t, pool.debug_table(t)["err"])
        _, done = pool.results()
        assert (done == 2).all()
        lens = np.zeros(n, dtype=np.uint32)
        assert pool._L.mj_log_lengths(pool.h, lens.ctypes.data, pool._stream()) == 0
        assert (lens > cap).all(), lens
        raised = None
        try:
            pool.read_logs()
        except MortalAmdError as e:
            raised = e
        assert raised is not None and "event log overflow on table 0" in str(raised), raised
        buf = np.empty((n, cap), dtype=np.uint64)
        assert pool._L.mj_log_read(pool.h, 0, n, buf.ctypes.data, pool._stream()) == 0
        for t in range(n):
            want = fc[t]["words"][:cap]
            cmp = np.ones(cap, dtype=bool)
            tp = fc[t]["tag_pos"][fc[t]["tag_pos"] < cap]
            cmp[tp] = False
            bad = np.flatnonzero((buf[t] != want) & cmp)
            assert bad.size == 0, (t, bad[:6].tolist(), [hex(int(x)) for x in buf[t][bad[:3]]], [hex(int(x)) for x in want[bad[:3]]])
            assert ((buf[t][tp] >> np.uint64(63)) == 1).all(), t  # a tag word where the forecast puts one
        return dict(lingered=lingered, cycles=int(over_at.max()), distinct_cycles=len(set(over_at.tolist())))
    finally:
        pool.close()


# ---------------------------------------------------------------- the arena's Python surface: BatchRunner._fail
class OneBadAnswerEngine:
    """The reference's engine contract (agent/mortal.rs:50-159), lowest legal action id; the first row of call number `bad_call`
    (if any) is answered with id 46."""
    engine_type = "mortal"
    is_oracle = False
    version = 3
    enable_quick_eval = True
    enable_rule_based_agari_guard = False

    def __init__(self, name, bad_call=None):
        self.name, self.bad_call, self.calls = name, bad_call, 0

    def react_batch(self, obs, masks, invisible_obs):
        m = torch.as_tensor(np.stack(masks, axis=0))
        a = m.to(torch.uint8).argmax(dim=1).tolist()
        if self.calls == self.bad_call:
            a[0] = 46
        self.calls += 1
        return a, torch.zeros(m.shape, dtype=torch.float32).tolist(), m.tolist(), [True] * m.shape[0]


def check_batch_runner_fail(pool_cls=None, bad_call=7):
    """OneVsThree.py_vs_py with a challenger that answers one row with an illegal id: MortalAmdError naming error code 1, the
    table and its seed, no later than the runner's next 64-cycle poll of mj_pool_first_error (an engine is called at most once
    per cycle)."""
    import re

    from libriichi.arena import OneVsThree
    from mortal_amd import arena as A

    old = A.BatchRunner.pool_cls
    if pool_cls is not None:
        A.BatchRunner.pool_cls = pool_cls
    bad = OneBadAnswerEngine("challenger", bad_call)
    raised = None
    try:
        OneVsThree(disable_progress_bar=True, deal_algo=0).py_vs_py(bad, OneBadAnswerEngine("champion"), (10000, parity_util.KEY), 1)
    except MortalAmdError as e:
        raised = e
    finally:
        A.BatchRunner.pool_cls = old
    assert raised is not None, "the run went on over a table in error"
    m = re.search(r"table (\d+) \(seed \((\d+), (\d+)\)\)", str(raised))
    assert m and "error code 1" in str(raised), str(raised)
    assert 0 <= int(m.group(1)) < 4 and (int(m.group(2)), int(m.group(3))) == (10000, parity_util.KEY), str(raised)
    assert bad_call < bad.calls <= bad_call + 1 + 64, bad.calls
    return bad.calls


# ---------------------------------------------------------------- the dataset loader's Python surface: "not a legal game"
def _play_logs(oracle, n, start):
    """n whole game logs (text, with their seeds) from the oracle arena under the greedy policy."""
    seeds = parity_util.default_seeds(n, start)
    arena = oracle.Arena(seeds, deal_algo=0, enable_quick_eval=True, version=3, keep_log=True)
    cycle = 0
    while arena.n_live > 0:
        rows = arena.poll()
        obs, masks = arena.encode(0, len(rows), want_obs=True)
        arena.commit(_greedy(arena, masks, rows, cycle, obs))
        cycle += 1
    return [mjai_log.dump_json_log(["a", "b", "a", "c"], seeds[g], arena.log(g)) for g in range(n)]


def _edit_log(raw, pick, change):
    """The log with the first event for which pick(ev) holds changed in place by change(ev)."""
    evs = [json.loads(line) for line in raw.splitlines()]
    change(next(e for e in evs if pick(e)))
    return "\n".join(json.dumps(e, separators=(",", ":")) for e in evs) + "\n"


def _samples(games):
    return [(g.player_id, g.actions, g.at_kyoku, g.at_turns, g.shantens, np.asarray(g.take_obs()).view(np.uint32), np.asarray(g.take_masks()),
             np.asarray(g.take_invisible_obs()).view(np.uint32)) for g in games]


def _same_samples(a, b):
    return len(a) == len(b) and all(x[:5] == y[:5] and all((p == q).all() for p, q in zip(x[5:], y[5:])) for x, y in zip(a, b))


def check_loader_rejects_a_log(oracle, pool_cls=None, version=3, edit="haipai"):
    """GameplayLoader(oracle=True, trust_seed=True) over three logs, the middle one edited.  edit="haipai": its first start_kyoku
    has two tiles swapped between the haipai of seat 0 and seat 1: the wall rebuilt from the seed no longer gives those hands
    (mj_replay.hip, MJ_ERR_WALL), and load_logs raises ValueError naming log 1; the other two logs, loaded without it, give what
    each gives loaded alone (a batch does not leak between its tables).  edit="discard": its first discard names a tile the seat
    does not hold, in a well-formed event -- load_logs should refuse that too (see the test that calls this)."""
    from mortal_amd.dataset import GameplayLoader

    old = GameplayLoader.pool_cls
    if pool_cls is not None:
        GameplayLoader.pool_cls = pool_cls
    try:
        logs = _play_logs(oracle, 3, 777)

        def swap(ev):
            a, b = ev["tehais"][0], ev["tehais"][1]
            i, j = next((i, j) for i in range(13) for j in range(13) if a[i] != b[j] and a[i] not in b and b[j] not in a)
            a[i], b[j] = b[j], a[i]

        def unheld(ev):
            ev["pai"], ev["tsumogiri"] = next(t for t in mjai_log.TILE_NAMES[:34] if t not in held[ev["actor"]] and t != ev["pai"]), False

        first = next(json.loads(line) for line in logs[1].splitlines() if '"start_kyoku"' in line)
        held = first["tehais"]  # (the first discard of the game: the hand is the haipai and the draw, which is ev["pai"] or held)
        bad = dict(haipai=_edit_log(logs[1], lambda e: e["type"] == "start_kyoku", swap),
                   discard=_edit_log(logs[1], lambda e: e["type"] == "dahai", unheld))
        load = lambda ls: GameplayLoader(version, oracle=True, trust_seed=True, player_names=["a", "c"]).load_logs(ls)
        raised = None
        try:
            load([logs[0], bad[edit], logs[2]])
        except ValueError as e:
            raised = e
        assert raised is not None and str(raised).startswith("log 1: the event stream is not a legal game"), (edit, raised)
        if edit != "haipai":
            return dict(message=str(raised))
        both = load([logs[0], logs[2]])
        alone = [load([logs[0]])[0], load([logs[2]])[0]]
        n = 0
        for a, b in zip(both, alone):
            sa, sb = _samples(a), _samples(b)
            assert len(sa) == 3 and _same_samples(sa, sb)
            n += sum(len(x[1]) for x in sa)
        return dict(samples=n, message=str(raised))
    finally:
        GameplayLoader.pool_cls = old
