"""mj_k_sp keeps the first states of a row in a two-choice hash set in LDS (mj_sp.hip: sp_set_find_or_claim, SP_SET_BUCKETS buckets
of two ways) and the states that find their four ways taken in the HBM tag table.  The emulator runs the unchanged kernel against the
oracle: SP rows f32 bit for bit, no overflow, and the id <-> key bijection checked on every hit (sp_emu_check_hit raises the overflow
flag), for
  (a) the default set (1,024 buckets: every state of these small rows lives in LDS),
  (b) a tiny set (-DSP_SET_BUCKETS=16: 32 ways, so most states overflow to the HBM table and both paths and the hand-over between
      them carry every row),
  (c) the tiny set with the tag epoch wrapping after three rows (-DSP_EPOCH_WRAP=3: the set's ways carry the same epoch as the tags
      and are wiped with them).
A small pool would run the small-pool schedule (mj_k_sp_promo + mj_k_sp_wide, which keep the child cache: a parked row changes
workgroups and LDS does not travel), so the runs switch it off (MJ_SP_WIDE=0): the kernel under test is mj_k_sp.
(b) and (c) need their own emulator library, hence a subprocess each (as test_emu_tag_epoch_wrap_in_a_variant_build)."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
if HOST not in sys.path:
    sys.path.insert(0, HOST)

import parity_util  # noqa: E402

CASE_ENV = "SP_LDS_SET_CASE"  # set by the outer tests: the inner run expects this split of the placements


@pytest.fixture(scope="module")
def emu():
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    import emu_pool

    return emu_pool.make_pool_class()


def _placed():
    """States placed in the LDS set / in the HBM table by this process's emulator library so far."""
    import emu_pool

    out = (ctypes.c_uint64 * 2)()
    emu_pool.emu_lib().mj_emu_sp_placed(out)
    return int(out[0]), int(out[1])


def _lockstep_cases(oracle, emu, monkeypatch):
    """The two lock-step cases of test_emu_device_code.py (v4_sp_rows_greedy, one_workgroup_takes_every_row) on mj_k_sp alone."""
    monkeypatch.setenv("MJ_SP_WIDE", "0")
    l0, h0 = _placed()
    st = parity_util.run_lockstep(oracle, 4, version=4, max_cycles=90, obs_every=1, pool_cls=emu, sp_rows_checked=True,
                                  policy="greedy", verbose=False)
    assert st["obs_checked"] > 300 and st["counters"]["sp_overflow"] == 0
    assert st["sp_schedule"]["hybrid_launches"] == 0, st["sp_schedule"]
    monkeypatch.setenv("MJ_SP_GRID", "1")
    st = parity_util.run_lockstep(oracle, 4, version=4, max_cycles=60, obs_every=1, pool_cls=emu, sp_rows_checked=True,
                                  policy="greedy", verbose=False)
    assert st["obs_checked"] > 200 and st["counters"]["sp_overflow"] == 0
    assert st["sp_schedule"]["hybrid_launches"] == 0, st["sp_schedule"]
    l1, h1 = _placed()
    return l1 - l0, h1 - h0


def test_lds_set_default_size(oracle, emu, monkeypatch):
    """(a), and the inner run of (b) / (c) in their variant builds."""
    in_lds, in_hbm = _lockstep_cases(oracle, emu, monkeypatch)
    print("states placed in LDS / HBM:", in_lds, in_hbm)
    if os.environ.get(CASE_ENV) == "tiny":
        # 32 ways against rows of hundreds of states: the pool sends states both ways, and most of them to HBM
        assert in_lds > 0 and in_hbm > in_lds, (in_lds, in_hbm)
    else:
        assert in_lds > 0, (in_lds, in_hbm)


def _variant(flags):
    env = dict(os.environ, EMU_EXTRA_FLAGS=flags)
    env[CASE_ENV] = "tiny"
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k", "default_size", "-p",
                          "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "1 passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_lds_set_tiny_most_states_overflow_to_hbm():
    """(b)"""
    _variant("-DSP_SET_BUCKETS=16")


def test_lds_set_tiny_with_epoch_wrap():
    """(c)"""
    _variant("-DSP_SET_BUCKETS=16 -DSP_EPOCH_WRAP=3")
