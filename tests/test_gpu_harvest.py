"""Finished games collected from a pool in refill mode on the MI355X (mortal_amd/csrc/mj_harvest.hip behind
mj_pool_enable_harvest / mj_harvest_take / mj_harvest_stat / mj_harvest_grp / mj_replay_load_harvest; TablePool.take_harvest,
Harvest, GameplayLoader.load_harvest, arena.SelfPlayRunner).  The cases and their yardsticks live in tests/harvest_cases.py,
shared with the host-emulation leg (tests/test_emu_harvest.py)."""
import pytest

import harvest_cases as H

pytestmark = pytest.mark.gpu

# 70 tables = two blocks with six padding lanes; in the sorted order of a take games 0..69 are generation 0, so the ten-game range
# from 60 crosses game 64 and ends at the last game of the generation
N_TABLES = 70
RANGE = dict(game0=60, seats=[15, 0, 5, 10, 1, 15, 8, 3, 15, 6])
# eight tables of block 0 and three of block 1
SAME = {0, 1, 2, 3, 4, 5, 6, 7, 64, 65, 66}


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
    """70 tables, two generations each, one take at the end: shared and left unchanged."""
    run, h, want = H.two_generations(pool_cls, N_TABLES)
    yield run, h, want
    h.close()
    run.close()


def test_two_generations_records_stat_grp(played, lib):
    H.check_two_generations(*played, lib)


def test_two_generations_samples_equal_the_reference_loader_v3(oracle, played):
    run, h, _ = played
    assert H.check_samples(oracle, run, h, RANGE["game0"], RANGE["seats"]) > 1000


def test_two_generations_samples_equal_the_reference_loader_v4_no_forced_kan_select(oracle, played):
    run, h, _ = played
    assert H.check_samples(oracle, run, h, RANGE["game0"], RANGE["seats"], version=4, always_kan=False) > 1000


def test_many_games_ending_in_one_step(pool_cls, lib):
    H.check_many_in_one_step(pool_cls, 67, SAME, lib)


def test_taking_while_playing(pool_cls):
    H.check_take_while_playing(pool_cls, 8)


def test_full_buffer_drops_and_counts(pool_cls):
    H.check_full_buffer(pool_cls, 8)


def test_a_table_in_error(oracle, pool_cls, lib):
    H.check_table_in_error(oracle, pool_cls, 4, 1, lib)


def test_staggered_start(pool_cls, lib):
    H.check_staggered_start(pool_cls, N_TABLES, 40, lib)


def test_invisible_obs_from_the_recorded_seed(oracle, played):
    run, h, _ = played
    assert H.check_invisible(oracle, run, h, N_TABLES + 3, 5) > 1000


def test_refusals(pool_cls, played):
    run, h, _ = played
    H.check_refusals(pool_cls, run, h)


def test_self_play_runner(oracle, pool_cls):
    H.check_self_play_runner(oracle, pool_cls, 8)
