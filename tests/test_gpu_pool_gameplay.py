"""Training samples and Grp from a pool's device log on the MI355X (mortal_amd/csrc/mj_gameplay.hip behind mj_replay_load_pool /
mj_pool_grp / mj_grp_logs; GameplayLoader.load_pool, TablePool.log_grp, Grp.from_packed).  The cases and their yardsticks live in
tests/pool_gameplay_cases.py, shared with the host-emulation leg (tests/test_emu_pool_gameplay.py)."""
import pytest

import pool_gameplay_cases as G

pytestmark = pytest.mark.gpu

# 70 tables = two blocks with six padding lanes; the first range crosses the block boundary at 60, no multiple of 64
N_TABLES = 70
RANGE_A = dict(table0=60, seats=[15, 0, 5, 10, 1, 15, 8, 3, 15, 6])
RANGE_B = dict(table0=0, seats=[15, 3, 0, 12, 15, 9])


@pytest.fixture(scope="module")
def pool_cls():
    from mortal_amd.pool import TablePool

    return TablePool


@pytest.fixture(scope="module")
def lib():
    from mortal_amd._lib import lib

    return lib


@pytest.fixture(scope="module")
def played(pool_cls):
    """The 70 finished games and their logs as the host reads them, shared and left unchanged."""
    pool = G.play(pool_cls, N_TABLES)
    yield pool, pool.read_logs()
    pool.close()


def test_pool_route_equals_the_reference_loader_v3(oracle, played):
    pool, logs = played
    assert G.check_range(oracle, pool, logs, 3, RANGE_A["table0"], RANGE_A["seats"], True, want_census=True) > 1000


def test_pool_route_equals_the_reference_loader_v4_no_forced_kan_select(oracle, played):
    pool, logs = played
    assert G.check_range(oracle, pool, logs, 4, RANGE_B["table0"], RANGE_B["seats"], False) > 700


def test_invisible_obs_from_the_seed(oracle, pool_cls):
    assert G.check_invisible(oracle, pool_cls, n=5, version=1) > 1000


def test_skipped_in_mid_run_and_a_table_in_error(oracle, pool_cls):
    G.check_skipped_and_error(oracle, pool_cls, n=4, victim=1)


def test_refused_calls_leave_the_destination_usable(pool_cls, played):
    G.check_refusals(pool_cls, played[0])


def test_grp_golden_game(lib):
    G.check_grp_golden(lib)


def test_grp_truncated_and_empty_logs(lib):
    G.check_grp_truncated(lib)


def test_grp_batch_of_130_cuts(lib, monkeypatch):
    G.check_grp_batch(lib)
    monkeypatch.setenv("MJ_LOG_GRID", "2")  # two workgroups: every wavefront takes 16 or 17 logs, one after the other
    G.check_grp_batch(lib)


def test_grp_tagged_log(lib):
    G.check_grp_tagged(lib)
