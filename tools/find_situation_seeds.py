#!/usr/bin/env python3
"""Search seeds whose games reach the rule situations of tests/situation_census.py, with the CPU oracle alone, and write
tests/golden/situation_seeds.json (the fixture of tests/test_situations_oracle.py, test_emu_situations.py, test_gpu_situations.py).

Every steering policy of tests/steering.py plays `--tables` hanchan (or their first cycles) per deal algorithm (rand 0.8 and rand 0.9) on the seeds
(start + i, parity_util.KEY); the census of the oracle's event logs says which kyoku of which table holds which situation.  One
entry per situation is written: the (policy, deal algorithm) pair with the most tables (up to --per-situation, earliest stop cycle
first; the deal algorithm alternates between situations where both have enough), and per table the kyoku, the cycle in which that
kyoku ended and the cycle at which a lock-step run may stop.  The output depends on the arguments only (they are recorded in the
file): the same arguments reproduce it byte for byte.

    python tools/find_situation_seeds.py            # the committed fixture (about a quarter of an hour on 8 cores)
"""
import argparse
import json
import os
import sys
from collections import Counter
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# what the fixture must hold; MAY_BE_MISSING are the only names allowed under "not_found"
TARGETS = (
    "ron_double", "ron_triple", "chankan_ron", "ron_on_ankan", "rinshan_tsumo", "haitei_tsumo", "houtei_ron", "first_turn_win",
    "tenhou", "double_riichi_declared", "double_riichi_win", "ippatsu_win", "abort_four_riichi", "abort_four_kans",
    "four_kans_one_seat_play_goes_on", "exhaustive_tenpai_0", "exhaustive_tenpai_3", "exhaustive_tenpai_4", "nagashi_mangan_1",
    "nagashi_mangan_2", "pao_set_daisangen", "pao_set_daisuushi", "pao_tsumo_paid", "pao_ron_split_paid", "win_32000_plus",
    "kan_dora_at_discard", "kan_dora_at_next_draw", "consecutive_kans", "hanchan_ends_negative", "west_round_kyoku", "honba_3_plus",
    "kyotaku_2_plus", "abort_four_winds", "abort_kyuushu", "four_winds_broken", "nagashi_lost_to_call", "kan_dora_at_ankan",
    "pao_ron_from_liable", "chiihou_position", "renhou_position",
)
MAY_BE_MISSING = ("ron_triple", "ron_on_ankan", "pao_set_daisuushi", "tenhou")  # at most three of them
OPTIONAL = ("nagashi_mangan_2",)  # written when the search meets two tables of one (the fixture's floor), no omission otherwise
# The policies added after the first fixture and the situations each was written for.  Such a policy is chosen for its own
# situations whenever it reaches them; for every other situation it stands behind the older policies whatever it found, so the
# entries that exist do not move when a policy is added.
WRITTEN_FOR = {
    "wind_discards": ("abort_four_winds", "abort_kyuushu", "four_winds_broken"),
    "calling_terminal_discards": ("nagashi_lost_to_call",),
    "first_go_around": ("chiihou_position", "renhou_position"),
}
CHUNK = 128
DEAL_CHUNK = 4096  # (of a policy with a steering.DEAL_FILTER: few of a chunk's tables are played)
SLACK = 3  # cycles a table runs past the end of its kyoku


def search_chunk(job):
    policy, algo, nonce0, n, max_cycles = job
    import oracle_lib
    import parity_util
    import situation_census
    import steering

    oracle_lib.lib()
    seeds = [(nonce0 + i, parity_util.KEY) for i in range(n)]
    if policy in steering.DEAL_FILTER:
        dealt = oracle_lib.Arena(seeds, deal_algo=algo, enable_quick_eval=True, version=3, keep_log=False)
        dealt.poll()
        seeds = [seeds[g] for g in range(n) if steering.DEAL_FILTER[policy](dealt, g)]
        del dealt
        if not seeds:
            return policy, algo, [], 0
    arena, ends = steering.play_oracle(oracle_lib, seeds, policy, deal_algo=algo, max_cycles=max_cycles)
    found = []
    kyoku = 0
    for g in range(len(seeds)):
        per = situation_census.census_by_kyoku(arena.log(g))
        done = arena.result(g)[1]
        kyoku += len(ends[g])
        for k, cnt in enumerate(per):
            if k >= len(ends[g]):
                break  # (the kyoku had not ended at max_cycles)
            bad = [s for s in cnt if s.startswith("mismatch:")]
            assert not bad, (policy, algo, seeds[g], k, bad)
            stop = (ends[g][-1] if done else ends[g][k]) + SLACK
            if policy in steering.NEVER_ENDING:
                stop = ends[g][k] + SLACK
            elif not done:
                continue  # (a policy whose games end is replayed to the end of the hanchan: final scores are compared)
            for s in cnt:
                if s in TARGETS:
                    found.append((s, seeds[g][0], k, ends[g][k], stop))
    return policy, algo, found, kyoku


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--start", type=int, default=20000)
    ap.add_argument("--tables", default="kan_seeking=768,closed_riichi_no_win=256,terminal_discards=1024,honour_hoarding=14336,everybody_rons=6144,"
                    "wind_discards=1024,calling_terminal_discards=512,first_go_around=2097152@8",
                    help="hanchan per policy and deal algorithm; policy=N@C plays C cycles instead of --max-cycles")
    ap.add_argument("--max-cycles", type=int, default=2500)
    ap.add_argument("--per-situation", type=int, default=8)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "situation_seeds.json"))
    args = ap.parse_args()
    import parity_util
    import steering

    # "policy=hanchan" or "policy=hanchan@cycles": a policy searched over the first cycles of its hanchan only
    tables = {k: [int(x) for x in v.split("@")] for k, v in (kv.split("=") for kv in args.tables.split(","))}
    jobs = [(pol, algo, args.start + c, min(DEAL_CHUNK if pol in steering.DEAL_FILTER else CHUNK, spec[0] - c), spec[1] if len(spec) > 1 else args.max_cycles)
            for pol, spec in tables.items() for algo in (0, 1)
            for c in range(0, spec[0], DEAL_CHUNK if pol in steering.DEAL_FILTER else CHUNK)]
    cands = {}  # situation -> (policy, algo) -> [(stop, nonce, kyoku, kyoku_end)]
    searched = Counter()
    with Pool(args.jobs) as pool:
        for pol, algo, found, kyoku in pool.imap(search_chunk, jobs):  # (imap: in job order, whatever finishes first)
            searched[f"{pol}/{'rand08' if algo == 0 else 'rand09'}"] += kyoku
            for s, nonce, k, kend, stop in found:
                cands.setdefault(s, {}).setdefault((pol, algo), []).append((stop, nonce, k, kend))
    entries, not_found = [], []
    for i, s in enumerate(TARGETS):
        by = cands.get(s)
        if not by:
            if s not in OPTIONAL:
                not_found.append(s)
            continue
        # one table once per entry (its earliest kyoku with the situation); the pair with the most tables, capped; then the
        # alternating deal algorithm; then the policy name
        def tables_of(key):
            seen, out = set(), []
            for stop, nonce, k, kend in sorted(by[key]):
                if nonce not in seen:
                    seen.add(nonce)
                    out.append((stop, nonce, k, kend))
            return out[:args.per_situation]

        def standing(key):
            return 0 if s in WRITTEN_FOR.get(key[0], ()) else 2 if key[0] in WRITTEN_FOR else 1

        best = min(by, key=lambda key: (standing(key), -len(tables_of(key)), key[1] != i % 2, key[0]))
        tabs = tables_of(best)
        if s in OPTIONAL and len(tabs) < 2:
            continue
        entries.append(dict(situation=s, policy=best[0], deal_algo="rand08" if best[1] == 0 else "rand09", count=len(tabs),
                            tables=[dict(nonce=nonce, key=parity_util.KEY, kyoku=k, kyoku_end_cycle=kend, stop_cycle=stop)
                                    for stop, nonce, k, kend in tabs]))
    missing = [s for s in not_found if s not in MAY_BE_MISSING]
    doc = dict(generator="tools/find_situation_seeds.py",
               arguments=dict(start=args.start, tables=args.tables, max_cycles=args.max_cycles, per_situation=args.per_situation),
               kyoku_searched=dict(sorted(searched.items())), not_found=not_found, entries=entries)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for e in entries:
        print(f"{e['situation']:34s} {e['policy']:22s} {e['deal_algo']} {e['count']} tables, stop cycles "
              f"{[t['stop_cycle'] for t in e['tables']]}")
    print("kyoku searched:", dict(searched), "not found:", not_found)
    if missing or len(not_found) > 3:
        raise SystemExit(f"situations that must be found are missing: {missing}")


if __name__ == "__main__":
    main()
