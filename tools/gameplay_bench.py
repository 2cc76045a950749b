#!/usr/bin/env python3
"""Times `GameplayLoader.load_pool` (samples replayed from the pool's device log: mj_replay_load_pool + mj_pool_grp, no JSON, no
files) against the route that gave the same samples before it: read_logs() -> mjai_log.decode_events -> dump_json_log -> load_logs.

Per pool size (default 256 and 1,024 tables): plays that many hanchan (obs v3, the device's greedy policy, event log on) to
completion, then runs both routes over the same finished pool, interleaved in this one process: --repeats pairs, the first pair
is the warm-up (reported, not in the medians).  Host clock around each route; both end in device synchronises (the copy of the
sample metadata to the host).  The new route is split by timing its calls of log_grp and replay_load_pool (pack + grp); the rest
is what both routes share: the replay loop into a sample store of the call's own, and its Gameplays, encoded once in the
reference's order (GameplayLoader._load).  The old route is split at its call of replay_load: what comes before is the host codec
(log copy, decode, JSON text, json.loads, Grp.load_events, encode_events).  One seat per table is tracked by default (--seats 1):
every obs of the range is materialised on the device, 128,570 B per obs-v3 sample, and this tool holds the results of both
routes at once to compare them -- 30 GB each for one seat of 1,024 tables.

The two routes must give the same samples (checked on the warm-up pair).  No ratio is gated: the file records what came out.
Writes profiles/pool_gameplay_bench.json.  Needs a GPU; there is no fallback.

--augment-leg instead measures what suit augmentation on the device costs (load_pool(..., augmented=True): the copy kernel swaps the
tiles on its way): per pool size, on the same finished pool, load_pool plain and augmented, interleaved in this one process, the
median of the timed pairs after a warm-up pair, with the pack step's own time per call (replay_load_pool: length pass, scan, copy)
for both.  With --parent-tree DIR (a checkout of the parent commit with its library built) it also alternates child processes of
this tool on the two trees, each playing the same pool and timing the plain load_pool: the plain path matches the parent when the
difference of the medians lies inside the spread of the parent's own runs.  Writes profiles/pool_augment_bench.json."""
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


class Clock:
    """Accumulates the time spent inside the wrapped methods, and the moment of the first call."""

    def __init__(self):
        self.total = 0.0
        self.first = None

    def wrap(self, fn):
        def timed(*a, **kw):
            t0 = time.perf_counter()
            if self.first is None:
                self.first = t0
            try:
                return fn(*a, **kw)
            finally:
                self.total += time.perf_counter() - t0
        return timed


def play(n, log_words):
    import numpy as np

    from mortal_amd.pool import TablePool

    pool = TablePool(n, version=3, deal_algo=0, max_rows=4 * n)
    pool.enable_log(log_words)
    pool.reset([(10000 + t, KEY) for t in range(n)], game_ids=np.arange(n), n_games_total=n)
    t0 = time.perf_counter()
    acts, cycle = None, 0
    while True:
        k, _ = pool.step(acts, None)
        if k == 0 and pool.counters()["games"] >= n:
            break
        obs, masks = pool.encode(0)
        acts = pool.greedy_policy(0, masks, obs, 7, cycle)
        cycle += 1
    code, tbl = pool.first_error()
    if code:
        raise SystemExit(f"table {tbl} ended with error {code}")
    return pool, cycle, time.perf_counter() - t0


def commit_of(arg):
    if arg:
        return arg
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        return "unknown"


def timed_load(loader, pool, n, mask, names, **kw):
    """One load_pool call -> (seconds, seconds inside replay_load_pool, samples)."""
    import numpy as np
    import torch

    from mortal_amd.pool import TablePool

    pack = Clock()
    real_pack = TablePool.replay_load_pool
    TablePool.replay_load_pool = pack.wrap(real_pack)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = loader.load_pool(pool, seats=np.full(n, mask, dtype=np.uint8), names=[names] * n, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        TablePool.replay_load_pool = real_pack
    n_samples = sum(len(g.actions) for per in got for g in per)
    del got
    torch.cuda.empty_cache()
    return dt, pack.total, n_samples


def plain_child(args):
    """Child of the parent A/B: imports the package of the tree given (this one or the parent's), plays each pool size and times
    the plain load_pool --repeats times after a warm-up -> one JSON line."""
    sys.path.insert(0, args.plain_child)
    from mortal_amd import _lib
    from mortal_amd.dataset import GameplayLoader

    names = ["a"] * args.seats + ["b"] * (4 - args.seats)
    loader = GameplayLoader(3, oracle=False, player_names=["a"])
    out = dict(tree=args.plain_child, library=_lib.LIB_PATH, sizes={})
    for n in args.tables:
        pool, _cycles, _play_s = play(n, args.log_words)
        runs = [timed_load(loader, pool, n, (1 << args.seats) - 1, names) for _ in range(args.repeats)]
        pool.close()
        out["sizes"][str(n)] = dict(warm_up_s=runs[0][0], load_pool_s=[r[0] for r in runs[1:]], pack_s=[r[1] for r in runs[1:]],
                                    samples=runs[0][2])
    print(json.dumps(out), flush=True)


def augment_leg(args):
    import torch

    from mortal_amd.dataset import GameplayLoader

    names = ["a"] * args.seats + ["b"] * (4 - args.seats)
    mask = (1 << args.seats) - 1
    loader = GameplayLoader(3, oracle=False, player_names=["a"])
    sizes = []
    for n in args.tables:
        pool, cycles, play_s = play(n, args.log_words)
        runs = []
        for _ in range(args.repeats):
            p = timed_load(loader, pool, n, mask, names)
            a = timed_load(loader, pool, n, mask, names, augmented=True)
            assert p[2] == a[2] > 0  # (the swap changes no sample count)
            runs.append(dict(plain_load_pool_s=p[0], plain_pack_s=p[1], augmented_load_pool_s=a[0], augmented_pack_s=a[1], samples=p[2]))
        pool.close()
        timed = runs[1:]
        med = {k: statistics.median(x[k] for x in timed) for k in runs[0] if k != "samples"}
        sizes.append(dict(tables=n, cycles=cycles, play_s=round(play_s, 3), samples=runs[0]["samples"], median=med, warm_up=runs[0],
                          timed=timed))
        print(json.dumps(med | dict(tables=n, samples=runs[0]["samples"])), flush=True)
    ab = None
    if args.parent_tree:
        # the plain path against the parent: children alternate between the two trees, new first
        trees = dict(new=ROOT, parent=os.path.abspath(args.parent_tree))
        rounds = []
        for r in range(args.ab_rounds):
            for which in ("new", "parent"):
                cmd = [sys.executable, os.path.abspath(__file__), "--plain-child", trees[which], "--repeats", str(args.repeats),
                       "--seats", str(args.seats), "--log-words", str(args.log_words), "--tables", *map(str, args.tables)]
                env = {k: v for k, v in os.environ.items() if k != "MORTAL_AMD_LIB"}
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
                if res.returncode != 0:
                    raise SystemExit(f"plain child on the {which} tree failed ({res.returncode}):\n{res.stderr[-2000:]}")
                rounds.append(dict(round=r, which=which) | json.loads(res.stdout.strip().splitlines()[-1]))
        ab = dict(method="child processes alternating new / parent, each plays the pool and times load_pool (plain) "
                         f"{args.repeats - 1} times after a warm-up; per child the median; spread = max - min of the parent's child medians",
                  rounds=rounds, sizes={})
        for n in args.tables:
            per = {w: [statistics.median(x["sizes"][str(n)]["load_pool_s"]) for x in rounds if x["which"] == w] for w in trees}
            spread = max(per["parent"]) - min(per["parent"])
            diff = statistics.median(per["new"]) - statistics.median(per["parent"])
            ab["sizes"][str(n)] = dict(new_child_medians_s=per["new"], parent_child_medians_s=per["parent"], parent_spread_s=spread,
                                       new_minus_parent_s=diff, within_parent_spread=abs(diff) <= spread)
            print(json.dumps(dict(tables=n) | ab["sizes"][str(n)]), flush=True)
    props = torch.cuda.get_device_properties(0)
    out = dict(tool="tools/gameplay_bench.py --augment-leg", commit=commit_of(args.commit), obs_version=3, seats_tracked=args.seats,
               repeats=args.repeats, clock="host perf_counter around each load_pool, device synchronised before and after; pack_s = "
               "the time inside replay_load_pool (length pass, scan, copy kernel, two synchronises)",
               box=dict(device=torch.cuda.get_device_name(0), gcn_arch=getattr(props, "gcnArchName", ""), cus=props.multi_processor_count,
                        torch=torch.__version__, hip=torch.version.hip, cpus_usable=len(os.sched_getaffinity(0))),
               sizes=sizes, plain_against_parent=ab)
    path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "pool_augment_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=path, commit=out["commit"])))


DEFAULT_OUT = os.path.join(ROOT, "profiles", "pool_gameplay_bench.json")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tables", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--repeats", type=int, default=3, help="pairs per size; the first is the warm-up")
    ap.add_argument("--seats", type=int, default=1, choices=[1, 2, 3, 4], help="tracked seats per table (seats 0..k-1)")
    ap.add_argument("--log-words", type=int, default=16384)
    ap.add_argument("--commit", default="", help="recorded as given (for a copy of the tree without its history)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--augment-leg", action="store_true", help="load_pool plain against augmented (profiles/pool_augment_bench.json)")
    ap.add_argument("--parent-tree", default="", help="--augment-leg: a built checkout of the parent commit, for the plain A/B")
    ap.add_argument("--ab-rounds", type=int, default=3, help="--parent-tree: child processes per tree")
    ap.add_argument("--plain-child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.repeats < 2:
        raise SystemExit("--repeats: at least 2 (the first pair is the warm-up)")
    if args.plain_child:
        return plain_child(args)
    if args.augment_leg:
        return augment_leg(args)

    import numpy as np
    import torch

    from mortal_amd import mjai_log
    from mortal_amd.dataset import GameplayLoader
    from mortal_amd.pool import TablePool

    names = ["a"] * args.seats + ["b"] * (4 - args.seats)
    mask = (1 << args.seats) - 1
    loader = GameplayLoader(3, oracle=False, player_names=["a"])
    sizes = []
    for n in args.tables:
        pool, cycles, play_s = play(n, args.log_words)
        lens = pool.log_lengths()
        seeds = [(10000 + t, KEY) for t in range(n)]
        runs = []
        for r in range(args.repeats):
            # ---- new route
            pack, grp = Clock(), Clock()
            real_pack, real_grp = TablePool.replay_load_pool, TablePool.log_grp
            TablePool.replay_load_pool, TablePool.log_grp = pack.wrap(real_pack), grp.wrap(real_grp)
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                new = loader.load_pool(pool, seats=np.full(n, mask, dtype=np.uint8), names=[names] * n)
                torch.cuda.synchronize()
                new_s = time.perf_counter() - t0
            finally:
                TablePool.replay_load_pool, TablePool.log_grp = real_pack, real_grp
            n_samples = sum(len(g.actions) for per in new for g in per)
            # ---- old route
            upload = Clock()
            real_load = TablePool.replay_load
            TablePool.replay_load = upload.wrap(real_load)
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                raws = [mjai_log.dump_json_log(names, seeds[t], mjai_log.decode_events(w)) for t, w in enumerate(pool.read_logs())]
                t_text = time.perf_counter()
                old = GameplayLoader(3, oracle=False, player_names=["a"], deal_algo=0).load_logs(raws)
                torch.cuda.synchronize()
                old_s = time.perf_counter() - t0
            finally:
                TablePool.replay_load = real_load
            if r == 0:  # same samples, same Grp
                assert len(new) == len(old) == n
                for a, b in zip(new, old):
                    assert [g.player_id for g in a] == [g.player_id for g in b]
                    for ga, gb in zip(a, b):
                        assert ga.actions == gb.actions and ga.at_kyoku == gb.at_kyoku and ga.at_turns == gb.at_turns
                        assert torch.equal(ga.obs_dev, gb.obs_dev) and torch.equal(ga.masks_dev, gb.masks_dev)
                        assert (ga.grp.feature == gb.grp.feature).all() and ga.grp.final_scores == gb.grp.final_scores
            runs.append(dict(load_pool_s=new_s, pack_s=pack.total, grp_s=grp.total, replay_and_slice_s=new_s - pack.total - grp.total,
                             old_route_s=old_s, old_text_s=t_text - t0, old_host_codec_s=upload.first - t0,
                             old_upload_replay_slice_s=old_s - (upload.first - t0), samples=n_samples))
            del new, old, raws
            torch.cuda.empty_cache()
        timed = runs[1:]
        med = {k: statistics.median(x[k] for x in timed) for k in runs[0] if k != "samples"}
        sizes.append(dict(tables=n, cycles=cycles, play_s=round(play_s, 3), log_words=int(lens.sum()), log_bytes=8 * int(lens.sum()),
                          samples=runs[0]["samples"], median=med, old_over_new=med["old_route_s"] / med["load_pool_s"],
                          warm_up=runs[0], timed=timed))
        pool.close()
        print(json.dumps(sizes[-1]["median"] | dict(tables=n, samples=runs[0]["samples"])), flush=True)

    props = torch.cuda.get_device_properties(0)
    out = dict(tool="tools/gameplay_bench.py", commit=commit_of(args.commit), obs_version=3, seats_tracked=args.seats,
               repeats=args.repeats, clock="host perf_counter around each route, device synchronised before and after",
               box=dict(device=torch.cuda.get_device_name(0), gcn_arch=getattr(props, "gcnArchName", ""), cus=props.multi_processor_count,
                        hbm_bytes=props.total_memory, torch=torch.__version__, hip=torch.version.hip, python=platform.python_version(),
                        host=platform.platform(), cpus_usable=len(os.sched_getaffinity(0))),
               sizes=sizes)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, commit=out["commit"], old_over_new={s["tables"]: round(s["old_over_new"], 2) for s in sizes})))


if __name__ == "__main__":
    main()
