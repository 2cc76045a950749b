"""Suit augmentation on the device, on the MI355X (mj_k_log_pack<true> behind MJ_LOAD_AUGMENT and mj_augment_logs;
GameplayLoader.load_pool / load_harvest(..., augmented=True), mjai_log.augment_logs).  The cases and their yardsticks live in
tests/pool_augment_cases.py, shared with the host-emulation leg (tests/test_emu_pool_augment.py)."""
import pytest

import pool_augment_cases as A
import pool_gameplay_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool_cls():
    from mortal_amd.pool import TablePool

    return TablePool


@pytest.fixture(scope="module")
def played(pool_cls):
    """Three finished games and their logs as the host reads them, shared and left unchanged."""
    pool = G.play(pool_cls, 3)
    yield pool, pool.read_logs()
    pool.close()


def test_directed_words_at_every_window_offset(pool_cls, monkeypatch):
    A.check_directed(pool_cls._L, py_kw={})  # (mjai_log.augment_logs on its default: the library, the current stream)
    monkeypatch.setenv("MJ_LOG_GRID", "2")  # two workgroups: every wavefront takes eight or nine logs, one after the other
    A.check_directed(pool_cls._L)


def test_pool_route_equals_the_reference_loader_on_swapped_events(oracle, pool_cls, played):
    pool, logs = played
    assert A.check_pool_route(oracle, pool_cls, pool, logs, 3, 3) > 1000


def test_pool_route_obs_v4_sp_rows_follow_the_swapped_hand(oracle, pool_cls):
    pool = G.play(pool_cls, 2, version=4)
    try:
        assert A.check_pool_route(oracle, pool_cls, pool, pool.read_logs(), 4, 2, want_conditions=False) > 500
    finally:
        pool.close()


@pytest.mark.parametrize("deal_algo", [0, 1])
def test_invisible_obs_swapped_events_wall_as_dealt(pool_cls, deal_algo):
    assert A.check_invisible(pool_cls, 2, 1, deal_algo) > 400


def test_harvest_route_and_a_record_in_error(oracle, pool_cls):
    assert A.check_harvest_route(oracle, pool_cls) > 500


def test_runners_pass_the_keyword_on(pool_cls):
    A.check_runners(pool_cls)


def test_refusals_leave_the_destination_usable(pool_cls, played):
    A.check_refusals(pool_cls, played[0])
