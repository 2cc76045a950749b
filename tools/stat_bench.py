#!/usr/bin/env python3
"""Times `TablePool.log_stat()` (mj_k_log_stat: Stat counted on the device, in place on the pool's event log) against the host path
that gave the same answer before it: read_logs() -> mjai_log.decode_events -> Stat.from_game x 4 seats.

Plays --tables hanchan (obs v3, the device's uniform-random legal policy, event log on) to completion, then
  1. log_stat(): one warm-up, median of 5, host clock around the synchronous call (it ends in a stream synchronise and includes
     its launch, its small allocations and the copy of the 91 result words);
  2. the host path, once;
asserts that both give the same two Stats, and appends one JSON line to profiles/log_stat.jsonl.  The only gate: (1) is faster
than (2) on the same machine in the same run.  `log_gbps` is the bytes of log the kernel has to read (8 x the words logged)
over the time of the whole call, and `hbm_peak_share` that rate over the 8.0 TB/s HBM3E peak: an end-to-end figure of the call,
not the kernel's own share of peak.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_BYTES_PER_S = 8.0e12
KERNEL_SHAPE = "shuffle-walk: one wavefront per log, 64-word coalesced windows, events taken from registers by wave-uniform __shfl, seat lanes 0..3"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tables", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log-words", type=int, default=16384, help="log capacity per table (u64 words)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_stat.jsonl"))
    ap.add_argument("--skip-host", action="store_true", help="time the device call only (no gate, nothing is compared)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from mortal_amd import mjai_log
    from mortal_amd.pool import TablePool
    from mortal_amd.stat import Stat

    n = args.tables
    pool = TablePool(n, version=3, max_rows=4 * n)
    pool.enable_log(args.log_words)
    key = 0xD5DFAA4CEF265CD7
    pool.reset([(10000 + t, key) for t in range(n)], game_ids=np.arange(n), n_games_total=n)
    masks = torch.empty((4 * n, 46), dtype=torch.bool, device=pool.device)
    obs = torch.empty((4 * n, pool.C, 34), dtype=torch.float32, device=pool.device)
    act = torch.empty(4 * n, dtype=torch.int32, device=pool.device)
    t0 = time.perf_counter()
    a_prev, cycle = None, 0
    while True:
        k, _ = pool.step(a_prev, None)
        if k == 0 and pool.counters()["games"] >= n:
            break
        pool.encode(0, obs, masks)
        a_prev = pool.random_policy(0, masks, 7, cycle, act)
        cycle += 1
    play_s = time.perf_counter() - t0
    code, tbl = pool.first_error()
    if code:
        raise SystemExit(f"table {tbl} ended with error {code}")

    pool.log_stat()  # warm-up: code object, first allocations
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        totals, _, counts = pool.log_stat()
        times.append(time.perf_counter() - t0)
    dev_s = statistics.median(times)
    assert counts == dict(reduced=n, skipped=0, malformed=0), counts

    words = int(pool.log_lengths().sum())

    host_s = None
    if not args.skip_host:
        t0 = time.perf_counter()
        host = Stat()
        for w in pool.read_logs():
            ev = mjai_log.decode_events(w)
            for seat in range(4):
                host += Stat.from_game(ev, seat)
        host_s = time.perf_counter() - t0
        assert totals[0] == host and totals[1] == Stat(), "device and host Stat differ"
        assert dev_s < host_s, f"log_stat() {dev_s:.6f} s is not faster than the host path {host_s:.3f} s"

    line = dict(tool="tools/stat_bench.py", device=torch.cuda.get_device_name(0), tables=n, cycles=cycle, play_s=round(play_s, 3),
                log_words=words, log_bytes=8 * words, kernel_shape=KERNEL_SHAPE, log_stat_s_median=dev_s,
                log_stat_s_all=[round(t, 6) for t in times], host_path_s=host_s,
                speedup=(host_s / dev_s) if host_s else None, log_gbps=8 * words / dev_s / 1e9,
                hbm_peak_share=8 * words / dev_s / HBM_PEAK_BYTES_PER_S, games=int(totals[0].game) // 4,
                rounds=int(totals[0].round) // 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    pool.close()


if __name__ == "__main__":
    main()
