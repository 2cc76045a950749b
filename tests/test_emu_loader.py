"""GameplayLoader.load_logs / load_pool / load_harvest and the store they fill behind the scenes (mortal_amd/dataset.py _load,
sample_bound, load_batch_rows), run on the host emulation of the device code.  The cases live in tests/loader_cases.py, shared with
the `-m gpu` leg (tests/test_gpu_loader.py)."""
import os
import shutil
import sys

import pytest

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
if HOST not in sys.path:
    sys.path.insert(0, HOST)

import harvest_cases as H  # noqa: E402
import loader_cases as LC  # noqa: E402
import pool_gameplay_cases as G  # noqa: E402
import sample_store_cases as SC  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    import emu_pool

    return emu_pool.make_pool_class()


@pytest.fixture(scope="module")
def played(oracle, emu):
    """Three finished games, their logs and the reference's reading of them, shared and left unchanged."""
    P = SC.Played(oracle, emu, 3)
    yield P
    P.close()


def test_rows_per_event_and_per_log_stay_within_the_bound(oracle, played):
    """The golden log and the parity range of tests/sample_store_cases.py (tables 1 and 2: kan labels with their select rows,
    events that give rows to two seats), under the seat masks 15, 6 and 1."""
    most, kan = LC.check_bound(oracle, [G.golden_events()] + [played.events(SC.TABLE0 + g) for g in range(len(SC.SEATS))])
    assert most >= 2 and kan >= 7


def test_a_load_leaves_nothing_behind(emu, played, monkeypatch):
    run = H.Run(emu, 2)
    try:
        run.play_until(run.every_table(1), 8000)
        h = run.pool.take_harvest()
        try:
            assert h.n_games >= 2 and h.n_errors == 0
            LC.check_nothing_left(emu, played.pool, played.logs, h, monkeypatch)
        finally:
            h.close()
    finally:
        run.close()


def test_more_samples_than_one_encode_launch_takes(oracle, played):
    assert LC.check_chunked(oracle, played.pool, played.logs, 3) > 4 * LC.load_batch_rows(2)  # (at least four full launches)
