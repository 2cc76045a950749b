"""Shared by tests/test_emu_loader.py (host emulation of the device code) and tests/test_gpu_loader.py (`-m gpu`): what
GameplayLoader.load_logs / load_pool / load_harvest owe to the store they fill behind the scenes (mortal_amd/dataset.py _load):
its capacity (sample_bound), its rows per encode launch (load_batch_rows), and that nothing of it outlives the call.

The samples themselves are compared with the reference loader restated on the oracle by the cases these build on
(pool_gameplay_cases.check_range); the rows an event gives are counted on the reference's side (dataset_ref.entry_event_indices)."""
import gc
import json

import pytest

import dataset_ref
import pool_gameplay_cases as G
import sample_store_cases as SC
from emu_alloc import stats

from mortal_amd import mjai_log as ML
from mortal_amd.dataset import GameplayLoader, load_batch_rows, sample_bound


# ---- case 1
def check_bound(oracle, events_list, masks=(15, 6, 1)):
    """No event of a legal game gives more than min(4, tracked seats + 1) rows, and a log's rows stay under the capacity the
    loader computes for it.  -> (the most rows one event gave, kan-select rows seen)."""
    most = kan = 0
    for ev in events_list:
        words = len(ML.encode_events(ev))
        for mask in masks:
            seats = SC.seats_of(mask)
            rows_at = {}
            for p in seats:
                for i, k in dataset_ref.entry_event_indices(oracle, ev, p, True):
                    rows_at[i] = rows_at.get(i, 0) + k
                    kan += k == 2
            assert max(rows_at.values()) <= min(4, len(seats) + 1), (mask, max(rows_at.values()))
            assert 0 < sum(rows_at.values()) < sample_bound([mask], [words]), (mask, sum(rows_at.values()), words)
            most = max(most, max(rows_at.values()))
    return most, kan


# ---- case 2
def bad_haipai(raw):
    """The log with two tiles swapped between the first haipai of seat 0 and seat 1: the seed no longer deals those hands."""
    evs = [json.loads(line) for line in raw.splitlines()]
    a, b = next(e for e in evs if e["type"] == "start_kyoku")["tehais"][:2]
    i, j = next((i, j) for i in range(13) for j in range(13) if a[i] not in b and b[j] not in a)
    a[i], b[j] = b[j], a[i]
    return "\n".join(json.dumps(e, separators=(",", ":")) for e in evs) + "\n"


def check_nothing_left(pool_cls, pool, logs, harvest, monkeypatch):
    """load_logs, load_pool and load_harvest of two games, succeeding and raising "not a legal game": the library's live
    buffers, events and streams after the call are those before it, and nothing was freed twice.  load_logs raises over a log
    with an edited haipai; a device log cannot be edited from outside, so for the other two the replay pool reports an error
    of table 1 when it is asked (TablePool.first_error) -- the store and the replay pool exist by then like in a real refusal."""
    L = pool_cls._L
    raws = [ML.dump_json_log(G.NAMES, G.seeds(pool.n_tables)[t], ML.decode_events(logs[t])) for t in (0, 1)]
    monkeypatch.setattr(GameplayLoader, "pool_cls", pool_cls)
    loader = GameplayLoader(3, oracle=True, trust_seed=True, deal_algo=0)
    calls = dict(load_logs=lambda bad: loader.load_logs([raws[0], bad_haipai(raws[1]) if bad else raws[1]]),
                 load_pool=lambda bad: loader.load_pool(pool, 0, 2, seats=[5, 15]),
                 load_harvest=lambda bad: loader.load_harvest(harvest, 0, 2, seats=[15, 10]))
    for name, call in calls.items():
        for bad in (False, True):
            gc.collect()
            before = stats(L)
            assert before["bad_frees"] == 0
            with monkeypatch.context() as m:
                if bad and name != "load_logs":
                    m.setattr(pool_cls, "first_error", lambda self: (9, 1))
                if bad:
                    with pytest.raises(ValueError, match=r"^log 1: the event stream is not a legal game \(error code \d+\)$"):
                        call(True)
                else:
                    got = call(False)
                    assert len(got) == 2 and all(len(g.actions) > 50 and len(g.invisible_obs) == len(g.actions) for per in got for g in per)
                    del got
            gc.collect()
            after = stats(L)
            assert after["live"] == before["live"] and after["bad_frees"] == 0, (name, bad, before, after)
            assert after["alloc"] > before["alloc"]  # (the call did go through the library)


# ---- case 3
def check_chunked(oracle, pool, logs, version, seats=(15, 15)):
    """load_pool of two tables (all seats, unless told otherwise): more samples than the rows of one encode launch and no multiple
    of them, so the store encodes several full chunks and a partial one -- against the reference loader, Gameplay by Gameplay."""
    total = G.check_range(oracle, pool, logs, version, 0, list(seats), True)
    rows = load_batch_rows(2)
    print("samples", total, "rows per launch", rows)
    assert total > 2 * rows and total % rows != 0, (total, rows)
    return total
