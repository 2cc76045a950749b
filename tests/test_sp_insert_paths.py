"""The expansion's insert pass (mj_sp.hip: sp_expand_chunk, P4) runs as stages behind wavefront-uniform tests: decode from einfo (the
entries past SP_EINFO_CAP by a search), look in the LDS table, a claim loop, the HBM table with its linear probe, new states, the
child-list entry.  The emulator counts the paths taken (mj_emu_sp_insert_paths, next to the placements and the lost claims):

  [0] rounds with one entry per lane   [1] rounds with two   [2] entries decoded by the search
  [3] a lane's claim-loop turns beyond its first   [4] entries sent to the HBM table   [5] linear-probe steps there

and this file runs the 4-table greedy v4 lock-step of tests/test_sp_lds_set.py (90 cycles, SP rows f32 bit for bit against the oracle,
no overflow -- the overflow flag also carries the emulator's checks of the id <-> key bijection, of the uniqueness of a row's ids and of
the pass's branch-free red-five arithmetic against the rules as the file states them elsewhere) on builds that force every path:

  default build                          both round forms, the claim loop's later turns
  -DSP_SET_BUCKETS=16                    32 ways: most states go on to the HBM table and probe there
  -DSP_EINFO_CAP=8                       all but a round's first eight entries are decoded by the search
  -DSP_EINFO_CAP=8 -DSP_SET_BUCKETS=16   both at once
  default build, MJ_SP_WIDE_ALL_ROWS=1   the child-cache form of the pass (mj_k_sp_wide): every state through the HBM table

so that across the file no path of the pass is left unexecuted, and each build shows the paths it is meant to force.  The heavy
directed hands (tests/golden/sp_directed_hands.json, thousands of states: rounds of two entries past the default SP_EINFO_CAP, a full
LDS set handing over to the HBM table) run in the default build with their recorded state counts.

A variant build needs its own emulator library, hence one subprocess each: this file run as a script."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
for p in (ROOT, os.path.join(ROOT, "tests"), HOST):
    if p not in sys.path:
        sys.path.insert(0, p)

NAMES = ("rounds_one", "rounds_two", "searched", "later_claim_turns", "hbm_entries", "probe_steps")
# what each run must show (a count above zero) and what it cannot show (zero)
WANT = {
    "default": {"rounds_one", "rounds_two", "later_claim_turns"},
    "tiny_set": {"rounds_one", "rounds_two", "later_claim_turns", "hbm_entries", "probe_steps"},
    "einfo8": {"rounds_one", "rounds_two", "searched", "later_claim_turns"},
    "einfo8_tiny_set": {"rounds_one", "rounds_two", "searched", "later_claim_turns", "hbm_entries", "probe_steps"},
    "child_cache": {"rounds_one", "rounds_two", "hbm_entries", "probe_steps"},
    "directed": {"rounds_one", "rounds_two", "searched", "later_claim_turns", "hbm_entries", "probe_steps"},
}
ZERO = {"child_cache": {"later_claim_turns"}}  # (the claim loop belongs to the LDS set)
FLAGS = {"tiny_set": "-DSP_SET_BUCKETS=16", "einfo8": "-DSP_EINFO_CAP=8", "einfo8_tiny_set": "-DSP_EINFO_CAP=8 -DSP_SET_BUCKETS=16"}


def _paths():
    import emu_pool

    out = (ctypes.c_uint64 * 6)()
    emu_pool.emu_lib().mj_emu_sp_insert_paths(out)
    return [int(x) for x in out]


def _check(case, before):
    got = dict(zip(NAMES, (b - a for a, b in zip(before, _paths()))))
    print(f"insert paths [{case}]:", got)
    for k in WANT[case]:
        assert got[k] > 0, (case, k, got)
    for k in ZERO.get(case, ()):
        assert got[k] == 0, (case, k, got)


def run_lockstep(oracle, emu, case):
    """The 4-table greedy lock-step on mj_k_sp alone, or (child_cache) with every row taken by mj_k_sp_wide."""
    import parity_util

    os.environ.pop("MJ_SP_GRID", None)
    if case == "child_cache":
        os.environ["MJ_SP_WIDE"] = "1"
        os.environ["MJ_SP_WIDE_ALL_ROWS"] = "1"
    else:
        os.environ["MJ_SP_WIDE"] = "0"
        os.environ.pop("MJ_SP_WIDE_ALL_ROWS", None)
    before = _paths()
    try:
        st = parity_util.run_lockstep(oracle, 4, version=4, max_cycles=90, obs_every=1, pool_cls=emu, sp_rows_checked=True,
                                      policy="greedy", verbose=False)
    finally:
        os.environ.pop("MJ_SP_WIDE_ALL_ROWS", None)
        os.environ.pop("MJ_SP_WIDE", None)
    assert st["obs_checked"] > 300 and st["counters"]["sp_overflow"] == 0, st
    if case == "child_cache":
        assert st["sp_schedule"]["rows_swept"] == 0, st["sp_schedule"]
    else:
        assert st["sp_schedule"]["hybrid_launches"] == 0, st["sp_schedule"]
    _check(case, before)


def run_directed(oracle, emu):
    import test_sp_contention as T
    from mortal_amd.state import PlayerState

    os.environ["MJ_SP_WIDE"] = "0"
    old = PlayerState.pool_cls
    PlayerState.pool_cls = emu
    before = _paths()
    try:
        heavy = [h for h in T.directed_hands() if h["kind"] == "heavy"]
        assert len(heavy) >= 3
        for h in heavy:
            n = T.check_directed_hand(oracle, PlayerState, h)  # whole v4 obs against the oracle, the fixture's state count
            print(f"{h['name']}: {n} states")
    finally:
        PlayerState.pool_cls = old
        os.environ.pop("MJ_SP_WIDE", None)
    _check("directed", before)


@pytest.fixture(scope="module")
def emu():
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    import emu_pool

    return emu_pool.make_pool_class()


def _variant(case):
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    env = dict(os.environ, EMU_EXTRA_FLAGS=FLAGS[case])
    out = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "insert paths run ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_default_build(oracle, emu):
    run_lockstep(oracle, emu, "default")


def test_child_cache_form(oracle, emu):
    run_lockstep(oracle, emu, "child_cache")


def test_heavy_directed_hands(oracle, emu):
    run_directed(oracle, emu)


@pytest.mark.parametrize("case", sorted(FLAGS))
def test_variant_build(case):
    _variant(case)


if __name__ == "__main__":
    import emu_pool
    import oracle_lib

    oracle_lib.lib()
    run_lockstep(oracle_lib, emu_pool.make_pool_class(), sys.argv[1])
    print("insert paths run ok")
