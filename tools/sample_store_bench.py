#!/usr/bin/env python3
"""Measures the sample store (mortal_amd/samples.py: decisions kept as 2 KB records, encoded when a batch draws them) against
`GameplayLoader.load_pool`, which materialises every obs of the range on the device: the same replay into a store of its own,
then every sample encoded at once.

One pool of --tables finished hanchan (obs v3 play, the device's greedy policy, event log on; the log does not depend on the obs
version), --seats tracked seats per table.  Per obs version (default 3 and 4), in this one process:
  resident   bytes per sample of both routes (the store's from mj_samples_info; load_pool's obs + mask);
  build      store_pool against load_pool over the same range, alternated, --repeats pairs after a warm-up pair (reported apart);
  batches    per batch size (default 512 and 4,096): one fixed-seed shuffled index list, `store.encode(idx)` against
             `torch.index_select` of obs and masks on what load_pool materialised, warmed up per shape, alternated.
Every time is taken with device events around synchronised work and reported as the median of the timed runs, with the runs.
No ratio is gated: the lines record what came out.  Writes profiles/sample_store_bench.jsonl, one line per obs version.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import platform
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEY = 0xD5DFAA4CEF265CD7


def play(n, log_words):
    import numpy as np

    from mortal_amd.pool import TablePool

    pool = TablePool(n, version=3, deal_algo=0, max_rows=4 * n)
    pool.enable_log(log_words)
    pool.reset([(10000 + t, KEY) for t in range(n)], game_ids=np.arange(n), n_games_total=n)
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
    return pool


def timed(fn):
    """fn() between two device events, the device idle before and after -> (milliseconds, what fn returned)."""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def med(xs):
    return round(statistics.median(xs), 4)


def bench_version(args, pool, version):
    import numpy as np
    import torch

    from mortal_amd.dataset import GameplayLoader
    from mortal_amd.pool import OBS_ROWS

    n = pool.n_tables
    seats = np.full(n, (1 << args.seats) - 1, dtype=np.uint8)
    loader = GameplayLoader(version, oracle=False)
    build = dict(load_pool_ms=[], store_pool_ms=[])
    got = store = None
    for _ in range(args.repeats + 1):  # (the first pair is the warm-up)
        got = None
        torch.cuda.empty_cache()
        ms, got = timed(lambda: loader.load_pool(pool, seats=seats))
        build["load_pool_ms"].append(ms)
        if store is not None:
            store.close()
        ms, store = timed(lambda: loader.store_pool(pool, seats=seats, capacity=args.capacity_per_table * n, batch_rows=args.batch_rows))
        build["store_pool_ms"].append(ms)
    obs_all = torch.cat([g.obs_dev for per in got for g in per])
    masks_all = torch.cat([g.masks_dev for per in got for g in per])
    del got
    count = store.count
    assert count == len(obs_all) > 0
    out = dict(version=version, tables=n, seats=args.seats, samples=count, batch_rows=args.batch_rows,
               resident_bytes_per_sample=dict(store=store.bytes_per_sample, load_pool=OBS_ROWS[version] * 34 * 4 + 46),
               build=dict(warm_up={k: round(v[0], 3) for k, v in build.items()}, median={k: med(v[1:]) for k, v in build.items()},
                          timed={k: [round(x, 3) for x in v[1:]] for k, v in build.items()}),
               batches=[])
    # (obs_all is in the reference's order: position k of it is sample order[k] of the store)
    order = store.order
    for size in args.batches:
        size = min(size, count)
        pos = np.random.default_rng(size).permutation(count)[:size]
        idx_store = order[pos]
        idx_dev = torch.as_tensor(pos, device=obs_all.device, dtype=torch.long)
        obs_buf = torch.empty((size, OBS_ROWS[version], 34), dtype=torch.float32, device=obs_all.device)
        mask_buf = torch.empty((size, 46), dtype=torch.bool, device=obs_all.device)

        def select():
            return torch.index_select(obs_all, 0, idx_dev), torch.index_select(masks_all, 0, idx_dev)

        def encode():
            return store.encode(idx_store, obs=obs_buf, masks=mask_buf)

        runs = dict(index_select_ms=[], store_encode_ms=[])
        for r in range(args.repeats + 1):
            ms, sel = timed(select)
            runs["index_select_ms"].append(ms)
            ms, enc = timed(encode)
            runs["store_encode_ms"].append(ms)
            if r == 0:  # the two sides deliver the same batch
                assert torch.equal(sel[0].view(torch.int32), enc[0].view(torch.int32)) and torch.equal(sel[1], enc[1])
            del sel
        out["batches"].append(dict(size=size, warm_up={k: round(v[0], 3) for k, v in runs.items()},
                                   median={k: med(v[1:]) for k, v in runs.items()},
                                   timed={k: [round(x, 3) for x in v[1:]] for k, v in runs.items()}))
    store.check_overflow()
    store.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tables", type=int, default=64)
    ap.add_argument("--seats", type=int, default=1, help="tracked seats per table (seats 0 .. seats - 1)")
    ap.add_argument("--versions", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--batches", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--batch-rows", type=int, default=4096, help="the store's rows per encode launch")
    ap.add_argument("--capacity-per-table", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log-words", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_store_bench.jsonl"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("sample_store_bench needs a GPU (torch.cuda.is_available() is False)")
    pool = play(args.tables, args.log_words)
    lines = []
    for v in args.versions:
        res = bench_version(args, pool, v)
        res["device"] = torch.cuda.get_device_name(0)
        res["host"] = platform.machine()
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    pool.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
