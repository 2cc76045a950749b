#!/usr/bin/env python3
"""Choose, with the CPU oracle alone, the decisions that tests/table_error_cases.py answers with a poisoned value, and write
tests/golden/table_error_plan.json (the fixture of tests/test_table_error_plan.py, test_emu_table_errors.py and
test_gpu_table_errors.py).

Every run plays parity_util.default_seeds under oracle_lib.random_actions.  A request names a poison kind, the tables it may
land on and the first cycle it may use; it is given the first decision row, in cycle order, at which the kind applies
(table_error_cases.poisoned_value: the row exists and the poisoned id's mask bit is clear), one victim per table.  The main
run (160 tables: two blocks of 64 and a half block) spreads its victims over lane 0 and lane 63 of a block, two victims of one
block on one cycle, the half block and its last table, and one victim whose bad answer is decoded in the very step in which
another, living table of its block is dealt a kyoku (`deal_neighbour`).  `log_overflow.words_per_table` is the smallest log
capacity from 200 words up at which, under the greedy policy, every one of the 160 tables overflows, on many different cycles, one
of them inside a hora / ryukyoku event and one in the last board step before a decision.  Two more runs: `guard` (the rule-based
agari guard with a q row of -inf and one of NaN) and `words` (explicit reaction words).  The output depends on this file only.

    python tools/find_table_error_plan.py          # a few seconds
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

R = lambda a, b: list(range(a, b))
# (kind, tables, extra): extra = "pair" (the next request shares its cycle and block) / "deal" (see above) / None
MAIN = [
    ("id_46", [0], None), ("id_1000", [63], None), ("id_minus1", R(48, 63), "pair"), ("id_int_min", R(48, 63), None),
    ("agari_none", R(32, 48), "deal"), ("discard_not_in_hand", R(1, 32), None), ("red_five_plain_only", R(1, 32), None),
    ("riichi_without_can", R(1, 32), None), ("chi_on_own_turn", R(1, 32), None), ("pon_on_own_turn", R(1, 32), None),
    ("pon_on_chi_only", R(1, 32), None), ("kan_none", R(1, 32), None), ("ryukyoku_none", R(1, 32), None),
    ("pass_own_turn", R(1, 32), None), ("pass_own_turn", R(128, 159), None), ("discard_not_in_hand", [159], None),
    ("id_46", [64], None), ("id_1000", [127], None), ("agari_none", R(65, 127), None),
]
RUNS = dict(
    main=dict(n_tables=160, quick_eval=True, first_cycle=6, spacing=5, requests=MAIN),
    kan_select=dict(n_tables=64, quick_eval=False, first_cycle=5, spacing=3,
                    requests=[("kan_select_not_candidate", R(0, 64), None), ("kan_select_34", R(0, 64), None)]),
    small=dict(n_tables=4, quick_eval=True, first_cycle=30, spacing=0, requests=[("id_46", [2], None)]),
)
MAX_CYCLES = 600


def plan_run(oracle, T, name, cfg):
    import parity_util

    n = cfg["n_tables"]
    arena = oracle.Arena(parity_util.default_seeds(n), deal_algo=0, enable_quick_eval=cfg["quick_eval"], version=3, keep_log=False)
    reqs = [dict(kind=k, tables=set(t), extra=x, first=cfg["first_cycle"] + i * cfg["spacing"]) for i, (k, t, x) in enumerate(cfg["requests"])]
    for i, r in enumerate(reqs):
        if r["extra"] == "pair":
            reqs[i + 1]["first"] = None  # placed together with request i
    entries, used = [], {}
    held = None  # a "deal" request's candidates of the previous cycle, waiting for the poll that follows
    for cycle in range(MAX_CYCLES):
        rows = arena.poll()
        if held:
            req, cands, before = held
            after = T.kyoku_ids(arena, n)
            dealt = [g for g in range(n) if after[g] != before[g] and g not in used]
            for e in cands:
                nb = [g for g in dealt if g >> 6 == e["table"] >> 6 and g != e["table"]]
                if nb and e["table"] not in used:
                    entries.append(dict(e, deal_neighbour=nb[0]))
                    used[e["table"]] = e["cycle"]
                    req["done"] = True
                    break
            held = None
        if all(r.get("done") for r in reqs):
            break
        masks = arena.encode(0, len(rows), want_obs=False)[1]
        act = oracle.random_actions(masks, rows, cycle, seed=T.POLICY_SEED)

        def candidates(req, taken):
            out = []
            for r in range(len(rows)):
                g, seat, kan = (int(x) for x in rows[r])
                if g not in req["tables"] or g in used or g in taken:
                    continue
                e = dict(kind=req["kind"], table=g, cycle=cycle, seat=seat, row="kan" if kan else "main")
                v = T.poisoned_value(req["kind"], masks[r], bool(kan), lambda: arena.player_state(g, seat).snapshot())
                if v is not None and T.applies(dict(e, value=v), arena, rows, masks, act) == r:
                    out.append(dict(e, value=v))
            return out

        for i, req in enumerate(reqs):
            if req.get("done") or req["first"] is None or cycle < req["first"]:
                continue
            if req["extra"] == "deal":
                if held is None:
                    cands = candidates(req, ())
                    if cands:
                        held = (req, cands, T.kyoku_ids(arena, n))
                continue
            cands = candidates(req, ())
            if req["extra"] == "pair":
                other = reqs[i + 1]
                for e in cands:
                    mate = [m for m in candidates(other, (e["table"],)) if m["table"] >> 6 == e["table"] >> 6]
                    if mate:
                        entries += [e, mate[0]]
                        used[e["table"]] = used[mate[0]["table"]] = cycle
                        req["done"] = other["done"] = True
                        break
            elif cands:
                entries.append(cands[0])
                used[cands[0]["table"]] = cycle
                req["done"] = True
        arena.commit(act)
    left = [r["kind"] for r in reqs if not r.get("done")]
    if left:
        raise SystemExit(f"run {name}: no decision found for {left} in {MAX_CYCLES} cycles")
    entries.sort(key=lambda e: (e["cycle"], e["table"]))
    return dict(n_tables=n, quick_eval=cfg["quick_eval"], entries=entries)


def plan_guard(oracle, T, n=16):
    """The rule-based agari guard on, greedy policy (it answers 43 wherever it may): the first row whose 43 rule_based_agari
    rejects gets a q row of -inf on both sides (no victim: the agari is played), the first such own-turn row of another table
    gets a q row of NaN on the device (its maximum is 45, which no own-turn row may answer)."""
    import parity_util

    run = dict(n_tables=n, quick_eval=True, policy="greedy", guard=True, entries=[])
    arena = oracle.Arena(parity_util.default_seeds(n), deal_algo=0, enable_quick_eval=True, version=3, keep_log=False)
    left = ["guard_q_neg_inf", "guard_q_nan"]
    for cycle in range(4000):
        rows = arena.poll()
        if not left or (len(rows) == 0 and arena.n_live == 0):
            break
        obs, masks = arena.encode(0, len(rows), want_obs=True)
        act = T.policy_actions(oracle, run, arena, rows, masks, cycle, obs)
        q = parity_util.fake_q_values(masks, rows, cycle, T.POLICY_SEED)
        for r in np.flatnonzero(act == 43).tolist():
            g, seat, _ = (int(x) for x in rows[r])
            for kind in left:
                e = dict(kind=kind, table=g, cycle=cycle, seat=seat, row="main", value=T.GUARD_KINDS[kind])
                if all(g != x["table"] for x in run["entries"]) and T.applies(e, arena, rows, masks, act) == r:
                    run["entries"].append(e)
                    left.remove(kind)
                    if kind in T.SURVIVES:
                        q[r] = -np.inf
                    break
        arena.commit(act, q)
    if left:
        raise SystemExit(f"guard run: no decision found for {left}")
    return run


def plan_words(oracle, T, n=64, table=37, first_cycle=12):
    """Every row answered with an explicit reaction word (tsumogiri policy): the first own-turn row of `table` from
    `first_cycle` on gets the word of a discard of a tile the seat does not hold."""
    import parity_util

    run = dict(n_tables=n, quick_eval=True, policy="tsumogiri", words=True, entries=[])
    arena = oracle.Arena(parity_util.default_seeds(n), deal_algo=0, enable_quick_eval=True, version=3, keep_log=False)
    for cycle in range(MAX_CYCLES):
        rows = arena.poll()
        masks = arena.encode(0, len(rows), want_obs=False)[1]
        act = T.policy_actions(oracle, run, arena, rows, masks, cycle, None)
        for r in np.flatnonzero(rows[:, 0] == table).tolist() if cycle >= first_cycle else ():
            seat = int(rows[r, 1])
            v = T.poisoned_value("reaction_word", masks[r], bool(rows[r, 2]), lambda: arena.player_state(table, seat).snapshot(), seat)
            e = dict(kind="reaction_word", table=table, cycle=cycle, seat=seat, row="main", value=v)
            if v is not None and T.applies(e, arena, rows, masks, act) == r:
                run["entries"].append(e)
                return run
        arena.commit(act)
    raise SystemExit("words run: no decision found")


def overflow_ok(T, prof, n_emu=64):
    """What the log-overflow case needs of a capacity: every table overflows, on many different cycles, and both among all
    tables and among the emulator leg's first 64 one is cut inside a hora / ryukyoku event and one outlives its overflow by a cycle."""
    if any(p["cycle"] is None or p["cycle"] >= T.OVERFLOW_CYCLES - 3 for p in prof):
        return False
    return all(len({p["cycle"] for p in part}) >= 8 and any(p["inside"] for p in part) and any(p["lingers"] for p in part)
               for part in (prof, prof[:n_emu]))


def plan_overflow(oracle, T, n=160):
    fc = T.overflow_forecast(oracle, n)
    for cap in range(200, 320):
        if overflow_ok(T, T.overflow_profile(fc, cap)):
            return dict(n_tables=n, policy="parity_util.greedy_actions", words_per_table=cap)
    raise SystemExit("no log capacity found")


def main():
    import oracle_lib
    import table_error_cases as T

    oracle_lib.lib()
    doc = dict(generator="tools/find_table_error_plan.py", policy="oracle_lib.random_actions", policy_seed=T.POLICY_SEED, deal_algo="rand08",
               runs={name: plan_run(oracle_lib, T, name, cfg) for name, cfg in RUNS.items()}, log_overflow=plan_overflow(oracle_lib, T))
    doc["runs"].update(guard=plan_guard(oracle_lib, T), words=plan_words(oracle_lib, T))
    with open(T.PLAN_PATH, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for name, run in doc["runs"].items():
        for e in run["entries"]:
            print(name, e)


if __name__ == "__main__":
    main()
