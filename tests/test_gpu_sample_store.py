"""The sample store on the MI355X (mortal_amd/csrc/mj_samples.hip behind mj_samples_*; SampleStore, GameplayLoader.store_pool /
store_harvest, the runners' sample_store).  The cases and their yardsticks live in tests/sample_store_cases.py, shared with the
host-emulation leg (tests/test_emu_sample_store.py).  Every case runs the kernels once."""
import pytest

import sample_store_cases as SC

pytestmark = pytest.mark.gpu

N_TABLES = 6


@pytest.fixture(scope="module")
def pool_cls():
    from mortal_amd.pool import TablePool

    return TablePool


@pytest.fixture(scope="module")
def played(oracle, pool_cls):
    """Six finished games, their logs and the reference's reading of them, shared and left unchanged."""
    P = SC.Played(oracle, pool_cls, N_TABLES)
    yield P
    P.close()


def test_store_equals_the_reference_loader_v3(played):
    assert SC.check_parity(played, 3, SC.TABLE0, SC.SEATS, 24, want_census=True) > 1000


def test_store_equals_the_reference_loader_v4(played):
    assert SC.check_parity(played, 4, 4, [2, 4], 16) > 200


def test_shuffled_batches_v3(played):
    assert SC.check_shuffled(played, 3, SC.TABLE0, SC.SEATS, 24) == 1 + 24 + 25 + 67 + 3 + 2


def test_shuffled_batches_v4(played):
    assert SC.check_shuffled(played, 4, 4, [2, 4], 16) == 1 + 16 + 17 + 43 + 3 + 2


@pytest.mark.parametrize("version", [1, 3])
def test_invisible_obs(played, version):
    assert SC.check_invisible(played, version, 3, 5) > 200


def test_augmented(played):
    assert SC.check_augmented(played, 5, 10) > 200


def test_two_harvests_into_one_store(oracle, pool_cls):
    assert SC.check_harvest(oracle, pool_cls) > 200


def test_capacity_and_refusals(played):
    SC.check_capacity_and_refusals(played)


def test_bytes_per_sample(pool_cls):
    SC.check_size(pool_cls._L)


def test_batch_runner_sample_store(oracle, pool_cls):
    SC.check_batch_runner(oracle, pool_cls)


def test_self_play_runner_sample_store(oracle, pool_cls):
    SC.check_self_play_runner(oracle, pool_cls)
