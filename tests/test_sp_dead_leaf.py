"""mj_k_sp skips the tenpai level of a row that has as many draws left as its shanten number (mj_sp.hip: leaf_dead,
sp_expand_dead_chunk): the emulator runs the unchanged kernels in lock-step with the oracle -- 64 tables, the benchmark's protocol
(refill, first starts staggered over the pre-roll, rand 0.9.1 deals), pre-rolled in obs v3, then 20 cycles of obs v4 with every row's
SP block compared f32 bit for bit (tests/sp_dead_leaf_cases.py).  The oracle alone gives this window 120 such rows (28 / 50 / 42 at
1 / 2 / 3 shanten, 16 of them without a discard), 99 rows with one draw more and 86 with one draw less; the test asks for 30 / 8 at
3 shanten / 3 without a discard / one each at 1 and 2 shanten, for both neighbours of the boundary, for the kernel's own count of
the rows that took the path to equal the oracle's, and for no overflow -- which in the emulator includes the uniqueness check of the
finished graphs, the id <-> key check of every hit and the check that every required draw of a 1-shanten state has a keeping discard
(what the shortened child list rests on).
  (a) mj_k_sp alone (MJ_SP_WIDE=0);
  (b) the small-pool schedule with every eligible row parked (thresholds of 1: mj_k_sp_promo parks a 2- or 3-shanten row before
      level 1, mj_k_sp_wide expands the dead level from the hand-off block);
  (c) (a) in a variant build with a tiny LDS set (-DSP_SET_BUCKETS=16: most states live in the HBM table), in a subprocess."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
if HOST not in sys.path:
    sys.path.insert(0, HOST)

import sp_dead_leaf_cases as cases  # noqa: E402

N_TABLES, PRE, WINDOW = 64, 400, 20


@pytest.fixture(scope="module")
def emu():
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    import emu_pool

    return emu_pool.make_pool_class()


def test_dead_leaf_rows_mj_k_sp_alone(oracle, emu, monkeypatch):
    """(a), and the inner run of (c)."""
    monkeypatch.setenv("MJ_SP_WIDE", "0")
    st, c, ticks = cases.run(oracle, emu, N_TABLES, PRE, WINDOW)
    cases.check(st, c, ticks, 1)
    assert st["sp_schedule"]["hybrid_launches"] == 0, st["sp_schedule"]


def test_dead_leaf_rows_parked_and_finished_by_the_wide_kernel(oracle, emu, monkeypatch):
    """(b)"""
    monkeypatch.setenv("MJ_SP_WIDE", "1")
    monkeypatch.setenv("MJ_SP_PROMO_MIN1", "1")
    monkeypatch.setenv("MJ_SP_PROMO_MIN2", "1")
    st, c, ticks = cases.run(oracle, emu, N_TABLES, PRE, WINDOW)
    cases.check(st, c, ticks, 1)
    sc = st["sp_schedule"]
    # every 2- and 3-shanten row with a graph changes workgroups before its level 1 (the emulator runs the launches one after the
    # other: the sweep takes them)
    assert sc["hybrid_launches"] == WINDOW and sc["rows_promoted"] + sc["rows_swept"] >= c["dead_by_s"][2] + c["dead_by_s"][3], sc


def test_dead_leaf_rows_with_a_tiny_lds_set():
    """(c)"""
    env = dict(os.environ, EMU_EXTRA_FLAGS="-DSP_SET_BUCKETS=16")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k", "mj_k_sp_alone", "-p",
                          "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "1 passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
