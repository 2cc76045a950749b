#!/usr/bin/env python3
"""Times what collecting finished games costs a pool in refill mode (mj_k_harvest in front of mj_k_refill, mortal_amd/csrc/mj_harvest.hip)
and what the collected games cost to consume (take, Stat, Grp, load_harvest).

Pool: 65,536 tables, event log on, refill, first starts staggered over 3,072 untimed pre-roll cycles, so the timed cycles see every
phase of a hanchan and a steady stream of finishing games.  Two workloads: obs v3 with the random policy (the shortest cycle: a
per-step cost shows most) and obs v4 with the greedy policy.  After the pre-roll, legs of --steps cycles alternate between
harvesting off and on in this one process, on the same pool (enable_harvest(0) / enable_harvest(n)), the order swapped from pair to
pair (off/on, on/off, ...) so that a slow drift of the game phases or the clocks cancels in the medians.  Host clock around each
leg, device synchronised before and after.  The first pair of legs is the warm-up (reported, not in the medians).  The buffer of every on leg is taken after the leg, outside the timing; on the last one, take, stat,
grp and -- obs v3 only -- load_harvest over --load-games games with one seat each are timed per call and reported per 1,000 games.

The expectation under test: on - off lies inside the off legs' own spread.  Nothing is gated: the file records what came out.
Writes profiles/harvest_bench.json.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEY = 0xD5DFAA4CEF265CD7
POLICY_SEED = 0x9E3779B97F4A7C15


def commit_of(arg):
    if arg:
        return arg
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        return "unknown"


def sources_sha256():
    """Ties the numbers to the device and host sources they were measured on, whatever commit holds them."""
    import hashlib

    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "mortal_amd", "csrc")
    for path in sorted(os.path.join(csrc, f) for f in os.listdir(csrc)) + [os.path.join(ROOT, "include", "mortal_amd.h")]:
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def workload(args, version, policy):
    import numpy as np
    import torch

    from mortal_amd.dataset import GameplayLoader
    from mortal_amd.pool import ACTION_SPACE, OBS_ROWS, TablePool

    n = args.tables
    dev = torch.device("cuda:0")
    pool = TablePool(n, version=version, deal_algo=0, max_rows=2 * n)
    pool.enable_log(args.log_words)
    pool.reset([(10000 + t, KEY) for t in range(n)], game_ids=np.arange(n), n_games_total=n)
    pool.set_refill(n)
    pool.set_start_stagger(args.preroll)
    obs = torch.empty((2 * n, OBS_ROWS[version], 34), dtype=torch.float32, device=dev)
    obs3 = obs.view(-1)[: 2 * n * OBS_ROWS[3] * 34].view(2 * n, OBS_ROWS[3], 34)
    masks = torch.empty((2 * n, ACTION_SPACE), dtype=torch.bool, device=dev)
    act = torch.empty(2 * n, dtype=torch.int32, device=dev)
    state = dict(acts=None, i=0)

    def run(steps, ob):
        for _ in range(steps):
            nr, _ = pool.step(state["acts"], None)
            pool.encode(0, ob, masks)
            if policy == "greedy":
                pool.greedy_policy(0, masks, ob, POLICY_SEED, state["i"], act)
            else:
                pool.random_policy(0, masks, POLICY_SEED, state["i"], act)
            state["acts"] = act[:nr]
            state["i"] += 1

    # the pre-roll runs on the cheap v3 encode, as bench.py's does
    pool.configure(0, version=3)
    _, preroll_s = timed(lambda: run(args.preroll, obs3))
    pool.configure(0, version=version)
    run(args.warmup, obs)
    legs = []
    harvests = []
    for leg in range(2 * args.pairs):
        on = (leg % 2 == 1) != ((leg // 2) % 2 == 1)  # off/on, on/off, off/on, ...: a slow drift of phases or clocks cancels
        pool.enable_harvest(args.max_games if on else 0, args.max_games * args.words_per_game)
        c0 = pool.counters()
        _, dt = timed(lambda: run(args.steps, obs))
        c1 = pool.counters()
        rec = dict(harvest=on, cycle_ms=1e3 * dt / args.steps, games=c1["games"] - c0["games"], env_steps=c1["steps"] - c0["steps"])
        if on:
            pend = pool.harvest_pending()
            rec.update(collected=pend["games"], dropped=pend["dropped"], words=pend["words"])
            for h in harvests:
                h.close()
            harvests = []
            h, take_s = timed(pool.take_harvest)
            harvests.append(h)
            rec["take_s"] = take_s
            taken = rec
        legs.append(rec)
    code, tbl = pool.first_error()
    if code:
        raise SystemExit(f"table {tbl} in error {code}")
    h = harvests[0]
    per_k = 1000.0 / max(h.n_games, 1)
    consume = dict(games=h.n_games, words=h.n_words, dropped=h.dropped, take_ms_per_1000=1e3 * taken["take_s"] * per_k)
    (_, _, counts), stat_s = timed(lambda: h.stat())
    consume.update(stat_ms_per_1000=1e3 * stat_s * per_k, stat_counts=counts)
    grps, grp_s = timed(lambda: h.grp())
    consume.update(grp_ms_per_1000=1e3 * grp_s * per_k, grp_games=sum(1 for g in grps if g is not None))
    if version == 3:
        k = min(args.load_games, h.n_games)
        loader = GameplayLoader(3, oracle=False)
        seats = np.ones(k, dtype=np.uint8)
        loader.load_harvest(h, 0, min(k, 8), seats=seats[: min(k, 8)])  # warm-up
        got, load_s = timed(lambda: loader.load_harvest(h, 0, k, seats=seats))
        consume.update(load_games=k, load_samples=sum(len(g.actions) for per in got for g in per),
                       load_harvest_ms_per_1000=1e3 * load_s * 1000.0 / max(k, 1))
        del got
    h.close()
    pool.close()
    timed_legs = legs[2:]
    off = [x["cycle_ms"] for x in timed_legs if not x["harvest"]]
    on = [x["cycle_ms"] for x in timed_legs if x["harvest"]]
    out = dict(obs_version=version, policy=policy, preroll_s=round(preroll_s, 2), legs=legs,
               off_ms=dict(median=statistics.median(off), min=min(off), max=max(off)),
               on_ms=dict(median=statistics.median(on), min=min(on), max=max(on)),
               on_minus_off_ms=statistics.median(on) - statistics.median(off), off_spread_ms=max(off) - min(off),
               games_per_cycle=sum(x["games"] for x in timed_legs) / (len(timed_legs) * args.steps),
               words_per_cycle=sum(x.get("words", 0) for x in timed_legs if x["harvest"]) / max(1, len(on) * args.steps), consume=consume)
    del obs, obs3, masks, act
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tables", type=int, default=65536)
    ap.add_argument("--preroll", type=int, default=3072)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100, help="cycles per leg")
    ap.add_argument("--pairs", type=int, default=5, help="pairs of legs (off/on, on/off, ...); the first pair is the warm-up")
    ap.add_argument("--max-games", type=int, default=16384)
    ap.add_argument("--words-per-game", type=int, default=4096)
    ap.add_argument("--log-words", type=int, default=16384)
    ap.add_argument("--load-games", type=int, default=128)
    ap.add_argument("--workloads", nargs="+", default=["v3-random", "v4-greedy"], choices=["v3-random", "v4-greedy"])
    ap.add_argument("--commit", default="", help="recorded as given (for a copy of the tree without its history)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harvest_bench.json"))
    args = ap.parse_args()
    if args.pairs < 3 or args.pairs % 2 == 0:
        raise SystemExit("--pairs: an odd number >= 3 (the first pair is the warm-up, the timed pairs come in both orders equally often)")

    import torch

    results = []
    for w in args.workloads:
        version, policy = (3, "random") if w == "v3-random" else (4, "greedy")
        results.append(workload(args, version, policy))
        r = results[-1]
        print(json.dumps(dict(workload=w, off_ms=r["off_ms"], on_ms=r["on_ms"], on_minus_off_ms=r["on_minus_off_ms"],
                              off_spread_ms=r["off_spread_ms"], consume=r["consume"])), flush=True)
    props = torch.cuda.get_device_properties(0)
    out = dict(tool="tools/harvest_bench.py", commit=commit_of(args.commit), sources_sha256=sources_sha256(),
               library=os.path.basename(os.environ.get("MORTAL_AMD_LIB", "libmortal_amd.so")), tables=args.tables, preroll=args.preroll,
               steps_per_leg=args.steps, pairs=args.pairs, max_games=args.max_games, log_words=args.log_words,
               clock="host perf_counter around each leg / call, device synchronised before and after",
               box=dict(device=torch.cuda.get_device_name(0), gcn_arch=getattr(props, "gcnArchName", ""), cus=props.multi_processor_count,
                        hbm_bytes=props.total_memory, torch=torch.__version__, hip=torch.version.hip, python=platform.python_version(),
                        host=platform.platform(), cpus_usable=len(os.sched_getaffinity(0))),
               workloads=results)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, commit=out["commit"])))


if __name__ == "__main__":
    main()
