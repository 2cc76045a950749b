"""`-m gpu`: tables in error on the HIP pool (tests/table_error_cases.py has the cases and what they assert; every one of them has
run clean on the emulated device code first, tests/test_emu_table_errors.py).  The whole plan of
tests/golden/table_error_plan.json: 160 tables -- two full wavefronts and a half one --, 19 victims, ~300 cycles past the last; the log overflow of all 160
tables, the refill restart of three dead tables, the guard's NaN / -inf q rows, explicit reaction words, and the error reports of
the arena and of the dataset loader."""
import pytest
import table_error_cases as T

from mortal_amd.pool import TablePool

pytestmark = pytest.mark.gpu


def test_gpu_poisoned_lockstep_v3(oracle):
    run = T.plan()["runs"]["main"]
    st = T.run_poisoned(oracle, TablePool, run, tail=300, obs_cycles=(17, 47, 82, 97, 110, 200, 390))
    print("poisoned lock-step", {k: v for k, v in st.items()})
    assert st["fired"] == len(run["entries"]) == 19 and st["obs_checked"] > 0 and st["log_events"] > 50000
    assert st["neighbour_rows"] > 10000


def test_gpu_poisoned_lockstep_v4_sp_rows(oracle):
    """Obs v4 with the SP rows compared: the SP row queue and its persistent workgroups see batches whose row count drops as
    tables die.  The first 64 tables of the main run."""
    run = T.plan()["runs"]["main"]
    st = T.run_poisoned(oracle, TablePool, run, n_tables=64, version=4, tail=120, sp_rows_checked=True,
                        obs_cycles=(7, 17, 32, 47, 62, 72, 81, 82, 110, 150, 200))
    assert st["fired"] == 14 and st["obs_checked"] > 0 and st["counters"]["sp_overflow"] == 0


def test_gpu_poisoned_lockstep_kan_select_rows(oracle):
    run = T.plan()["runs"]["kan_select"]
    st = T.run_poisoned(oracle, TablePool, run, tail=300, obs_cycles=(19, 30, 100))
    assert st["fired"] == 2 and st["obs_checked"] > 0


def test_gpu_errored_table_among_finished_ones(oracle):
    st = T.run_poisoned(oracle, TablePool, T.plan()["runs"]["small"], to_completion=True, check_log_stat=True)
    assert st["fired"] == 1 and st["scores_checked"] == 3 and st["log_stat"] == dict(reduced=3, skipped=1, malformed=0)
    assert st["counters"]["games"] == 4 and st["counters"]["errors"] == 1


def test_gpu_row_capacity(oracle):
    T.check_row_capacity(oracle, TablePool)


def test_gpu_error_texts_are_the_pools_own_librarys():
    T.check_error_texts(TablePool)


def test_gpu_refill_restarts_a_dead_table_clean(oracle):
    st = T.check_refill_restart(oracle, TablePool, n=64)
    assert st["fired"] == 3 and st["side_rows"] > 1000


def test_gpu_log_overflow(oracle):
    lo = T.plan()["log_overflow"]
    st = T.check_log_overflow(oracle, TablePool, lo["n_tables"], lo["words_per_table"])
    assert st["lingered"] >= 1 and st["distinct_cycles"] >= 8


def test_gpu_batch_runner_reports_the_table_in_error():
    T.check_batch_runner_fail()


def test_gpu_poisoned_lockstep_guard_q_rows(oracle):
    run = T.plan()["runs"]["guard"]
    st = T.run_poisoned(oracle, TablePool, run, tail=60, obs_cycles=(760, 1015, 1040))
    assert st["fired"] == 2 and len(st["dead"]) == 1 and st["obs_checked"] > 0


def test_gpu_poisoned_lockstep_reaction_words(oracle):
    run = T.plan()["runs"]["words"]
    st = T.run_poisoned(oracle, TablePool, run, tail=300, obs_cycles=(11, 14, 40, 200))
    assert st["fired"] == 1 and len(st["dead"]) == 1 and st["obs_checked"] > 0 and st["neighbour_rows"] > 1000


def test_gpu_loader_names_the_log_that_is_no_legal_game(oracle):
    st = T.check_loader_rejects_a_log(oracle)
    assert st["samples"] > 300 and "error code" in st["message"]
