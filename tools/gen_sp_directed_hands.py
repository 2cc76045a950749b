#!/usr/bin/env python3
"""Writes tests/golden/sp_directed_hands.json: directed hands for mj_k_sp's hash set at its REAL capacity (1,024 buckets in LDS, the
rest in the HBM tag table).  Each hand is played as `start_kyoku` + one `tsumo` for seat 0 (as tests/test_gpu_state.py does with its
random hands); the host emulation of the kernels (tests/host, small-pool schedule off, so the kernel is mj_k_sp) encodes the v4 obs,
which must equal the oracle's, and the fixture records what the emulator counted for the row:
  states = the row's number of states (mj_sp_phase_ticks word 7), taken with the emulator's uniqueness check on (no overflow),
  lds / hbm = states placed in the LDS set / in the HBM table (mj_emu_sp_placed).
tests/test_sp_contention.py replays the fixture on the emulator, tests/test_gpu_sp_lds_set.py on the device: the device's state
count must equal `states`, which a state duplicated by a lost race would break while every obs value stayed right.

The first four hands are those of the reference's SP known-answer tests that this event stream can reach (14 tiles, the draw last:
tests/test_oracle_sp.py; the fifth has 13 tiles and no discard).  The heavy ones were picked by the counter: --search N SEED deals N
random hands and prints the ones with the most states.

  python tools/gen_sp_directed_hands.py            # rewrite the fixture
  python tools/gen_sp_directed_hands.py --search 400 7"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "host")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "sp_directed_hands.json")

# (name, kind, 13 tiles + the draw in mpsz notation (z: 1-7 = E S W N P F C), dora marker by its tile name)
HANDS = [
    ("kat_nanikiru_1", "kat", "45678m 34789p 3344z", "P"),
    ("kat_nanikiru_2", "kat", "3667m 23489p 34688s", "P"),
    ("kat_nanikiru_3", "kat", "45677m 456778p 248s", "6m"),
    ("kat_nanikiru_4", "kat", "9999m 6677p 88s 335z 1m", "1m"),
    ("heavy_6k", "heavy", "1238m 1234p 27s 113z 4m", "3m"),
    ("heavy_4k6", "heavy", "1126789m 345p 4s 45z 7p", "8s"),
    ("heavy_4k2", "heavy", "356m 134667p 47s 33z 3z", "3m"),
    ("heavy_3k8", "heavy", "169m 67p 3445678s 5z 4p", "8m"),
    ("heavy_2k9", "heavy", "5689m 146788p 67s 7z 6p", "8p"),
    ("no_graph", "no_graph", "147m 258p 369s 1234z 5z", "9m"),
    ("tenpai", "tenpai", "123m 456p 78999s 22z 5m", "E"),
    ("seven_pairs", "seven_pairs", "1133m 5577p 2244s 6z 7z", "9p"),
    ("thirteen_orphans", "thirteen_orphans", "19m 19p 19s 1234567z 5m", "2s"),
]


def parse(s):
    from oracle_lib import TILE_NAMES

    out, stack = [], []
    for ch in s:
        if ch.isdigit():
            stack.append(ch)
        elif ch in "mps":
            out += [f"5{ch}r" if d == "0" else d + ch for d in stack]
            stack = []
        elif ch == "z":
            out += [TILE_NAMES[26 + int(d)] for d in stack]
            stack = []
    assert len(out) == 14, s
    return out


def events(hand, draw, marker):
    return [{"type": "start_kyoku", "bakaze": "E", "dora_marker": marker, "kyoku": 1, "honba": 0, "kyotaku": 0, "oya": 0,
             "scores": [25000] * 4, "tehais": [list(hand)] + [["?"] * 13] * 3},
            {"type": "tsumo", "actor": 0, "pai": draw}]


def run_on_emulator(O, hand, draw, marker):
    import emu_pool
    import numpy as np

    from mortal_amd.state import PlayerState

    L = emu_pool.emu_lib()

    def placed():
        out = (ctypes.c_uint64 * 2)()
        L.mj_emu_sp_placed(out)
        return int(out[0]), int(out[1])

    old = PlayerState.pool_cls
    PlayerState.pool_cls = emu_pool.make_pool_class()
    try:
        dev, ora = PlayerState(0), O.PlayerState(0)
        for ev in events(hand, draw, marker):
            dev.update(ev)
            ora.update(ev)
        p0 = placed()
        og, mg = dev.encode_obs(4, False)
        oo, mo = ora.encode_obs(4, False)
        assert (mg == mo).all() and (og.view(np.uint32) == oo.view(np.uint32)).all(), (hand, draw)
        p1 = placed()
        tk = dev._pool.sp_phase_ticks()
        assert tk["overflow"] == 0 and dev._pool.sp_schedule_stats()["hybrid_launches"] == 0
        dev.close()
    finally:
        PlayerState.pool_cls = old
    return dict(shanten=int(ora.snapshot()["shanten"]), states=tk["states"], lds=p1[0] - p0[0], hbm=p1[1] - p0[1])


def main():
    os.environ["MJ_SP_WIDE"] = "0"  # the kernel under test is mj_k_sp
    assert not os.environ.get("EMU_EXTRA_FLAGS"), "the fixture records the DEFAULT build"
    import numpy as np
    import oracle_lib as O

    O.lib()
    if len(sys.argv) > 1 and sys.argv[1] == "--search":
        n, seed = int(sys.argv[2]), int(sys.argv[3])
        rng = np.random.default_rng(seed)
        full = np.array([t for t in range(34) for _ in range(4)])
        found = []
        for _ in range(n):
            pool = full.copy()
            rng.shuffle(pool)
            held = np.bincount(pool[:14], minlength=34)
            marker = O.TILE_NAMES[int(rng.choice(np.flatnonzero(held < 4)))]
            hand = [O.TILE_NAMES[int(t)] for t in sorted(pool[:13])]
            found.append((run_on_emulator(O, hand, O.TILE_NAMES[int(pool[13])], marker), hand, O.TILE_NAMES[int(pool[13])], marker))
        for r in sorted(found, key=lambda r: -r[0]["states"])[:10]:
            print(r)
        return
    rows = []
    for name, kind, tiles, marker in HANDS:
        t = parse(tiles)
        r = run_on_emulator(O, t[:13], t[13], marker)
        rows.append(dict(name=name, kind=kind, hand=t[:13], draw=t[13], dora_marker=marker, **r))
        print(rows[-1])
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main()
