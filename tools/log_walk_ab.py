#!/usr/bin/env python3
"""A/B of the calls that read packed event logs on the device (mj_log.h: mj_k_log_stat, mj_k_log_len / _pack, mj_k_log_grp), this
tree against a built checkout of another commit (--parent-tree), inside one run on one GPU.

Child processes alternate parent, new, parent, new, ...; the first pair is the warm-up.  Every child imports the package of its
tree, plays --tables hanchan to the end (obs v3, greedy device policy, event log on) and a second pool in refill mode with
harvesting on until --harvest-games games are collected, then times, host clock around synchronised calls, one warm-up and
--repeats runs each:
  log_stat           TablePool.log_stat() over all tables                         (tools/stat_bench.py's quantity)
  pack, grp          replay_load_pool / log_grp over the first --load-tables      (the split tools/gameplay_bench.py reports)
  load_pool          GameplayLoader.load_pool over the first --whole-tables, one seat each
  harvest_stat, harvest_grp, load_harvest    Harvest.stat / Harvest.grp / load_harvest (128 games)  (tools/harvest_bench.py's costs)
A child's figure per quantity is the median of its runs.  Gate per quantity: the median of the new tree's children does not
exceed the median of the parent's by more than the spread (max - min) of the parent's own children.  Writes --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 0xD5DFAA4CEF265CD7


def child(args):
    sys.path.insert(0, args.child)
    import numpy as np
    import torch

    from mortal_amd import _lib
    from mortal_amd.dataset import GameplayLoader
    from mortal_amd.pool import TablePool

    def timed(fn):
        out = []
        for _ in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
            del r
        return out[1:]

    def run(pool, until):
        acts, cycle = None, 0
        while not until(pool, cycle):
            k, _ = pool.step(acts, None)
            acts = None
            if k:
                obs, masks = pool.encode(0)
                acts = pool.greedy_policy(0, masks, obs, 7, cycle)
            cycle += 1

    n = args.tables
    res = {}
    pool = TablePool(n, version=3, deal_algo=0, max_rows=4 * n)
    pool.enable_log(args.log_words)
    pool.reset([(10000 + t, KEY) for t in range(n)], game_ids=np.arange(n), n_games_total=n)
    run(pool, lambda p, c: c > 0 and c % 64 == 0 and p.counters()["games"] >= n)
    assert pool.first_error()[0] == 0
    counts = pool.log_stat()[2]
    assert counts == dict(reduced=n, skipped=0, malformed=0), counts
    res["log_stat"] = timed(pool.log_stat)
    k = args.load_tables
    rp = TablePool(k, version=3)
    res["pack"] = timed(lambda: rp.replay_load_pool(pool))
    rp.close()
    res["grp"] = timed(lambda: pool.log_grp(0, k))
    w = args.whole_tables
    loader = GameplayLoader(3, oracle=False)
    res["load_pool"] = timed(lambda: loader.load_pool(pool, table0=0, n_tables=w, seats=np.ones(w, dtype=np.uint8)))
    pool.close()

    pool = TablePool(n, version=3, deal_algo=0, max_rows=4 * n)
    pool.enable_log(args.log_words)
    pool.reset([(10000 + t, KEY) for t in range(n)], game_ids=np.arange(n), n_games_total=n)
    pool.set_refill(n)
    pool.enable_harvest(2 * args.harvest_games, 2 * args.harvest_games * 4096)
    run(pool, lambda p, c: c > 0 and c % 64 == 0 and p.harvest_pending()["games"] >= args.harvest_games)
    h = pool.take_harvest()
    res["harvest_stat"] = timed(h.stat)
    res["harvest_grp"] = timed(h.grp)
    g = min(128, h.n_games)
    res["load_harvest"] = timed(lambda: loader.load_harvest(h, 0, g, seats=np.ones(g, dtype=np.uint8)))
    games = h.n_games
    h.close()
    pool.close()
    props = torch.cuda.get_device_properties(0)
    assert os.path.dirname(_lib.LIB_PATH).startswith(os.path.abspath(args.child))  # the library of the tree asked for
    print(json.dumps(dict(harvest_games=games, seconds=res,
                          box=dict(device=torch.cuda.get_device_name(0), gcn_arch=getattr(props, "gcnArchName", ""),
                                   cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent-tree", default="", help="a built checkout of the commit to compare with")
    ap.add_argument("--commit", default="", help="this tree's commit, recorded as given")
    ap.add_argument("--parent-commit", default="", help="the other tree's commit, recorded as given")
    ap.add_argument("--rounds", type=int, default=5, help="pairs of children; the first pair is the warm-up")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tables", type=int, default=4096)
    ap.add_argument("--load-tables", type=int, default=1024)
    ap.add_argument("--whole-tables", type=int, default=64)
    ap.add_argument("--harvest-games", type=int, default=2048)
    ap.add_argument("--log-words", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_walk_refactor.json"))
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    trees = dict(parent=os.path.abspath(args.parent_tree), new=ROOT)
    env = {k: v for k, v in os.environ.items() if k != "MORTAL_AMD_LIB"}
    runs = []
    for r in range(args.rounds):
        for which in ("parent", "new"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", trees[which]] + [
                x for k in ("repeats", "tables", "load_tables", "whole_tables", "harvest_games", "log_words")
                for x in ("--" + k.replace("_", "-"), str(getattr(args, k)))]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            if p.returncode != 0:  # nothing more is started on the GPU after a child that failed
                raise SystemExit(f"child on the {which} tree failed ({p.returncode}):\n{p.stderr[-3000:]}")
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            runs.append(dict(round=r, which=which, warm_up=r == 0) | rec)
            print(json.dumps(dict(round=r, which=which) | {q: round(1e3 * statistics.median(v), 4) for q, v in rec["seconds"].items()}), flush=True)
    gate = {}
    for q in runs[0]["seconds"]:
        per = {w: [statistics.median(x["seconds"][q]) for x in runs if x["which"] == w and not x["warm_up"]] for w in trees}
        med = {w: statistics.median(per[w]) for w in trees}
        spread = max(per["parent"]) - min(per["parent"])
        gate[q] = dict(parent_child_medians_s=per["parent"], new_child_medians_s=per["new"], parent_median_s=med["parent"],
                       new_median_s=med["new"], parent_spread_s=spread, new_minus_parent_s=med["new"] - med["parent"],
                       passes=med["new"] - med["parent"] <= spread)
        print(json.dumps(dict(quantity=q, parent_ms=round(1e3 * med["parent"], 4), new_ms=round(1e3 * med["new"], 4),
                              parent_spread_ms=round(1e3 * spread, 4), passes=gate[q]["passes"])), flush=True)
    out = dict(tool="tools/log_walk_ab.py", commit=args.commit, parent_commit=args.parent_commit, box=runs[0]["box"],
               method=__doc__.split("\n\n", 1)[1], args={k: v for k, v in vars(args).items() if k not in ("child", "out", "parent_tree")},
               gate=gate, runs=runs)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, all_pass=all(g["passes"] for g in gate.values()))))


if __name__ == "__main__":
    main()
