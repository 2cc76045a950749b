"""`-m gpu`: every table of tests/golden/situation_seeds.json on the HIP pool in lock-step with the oracle, one run per (steering
policy, deal algorithm) group: rows, masks and obs v3 on every cycle, every event of the logs, final scores of the finished tables.
The group of the kan-seeking policy on the rand 0.9 deal runs with obs v4 and the single-player rows checked instead.  After the
run the census of the DEVICE's own decoded logs (tests/situation_census.py) must show every situation of the group, in the recorded
kyoku, in at least the recorded number of tables.  Under the policies whose games end, every table must have finished and had its
final scores compared; under the no-win policies (steering.NEVER_ENDING) the run must have covered every table's stop cycle, and
the logs of the stopped tables are compared as prefixes of equal length (parity_util.run_lockstep)."""
import pytest
import situation_fixture as F
import steering

import parity_util

pytestmark = pytest.mark.gpu
V4_GROUP = ("kan_seeking", "rand09")


@pytest.mark.parametrize("group", sorted(F.groups()), ids=lambda g: f"{g[0]}-{g[1]}")
def test_gpu_lockstep_reaches_situations(oracle, group):
    tables, wanted = F.groups()[group]
    v4 = group == V4_GROUP
    last = max(stop for _, _, stop in tables)
    st = parity_util.run_lockstep(oracle, len(tables), version=4 if v4 else 3, max_cycles=last, seeds=[(n, k) for n, k, _ in tables],
                                  obs_every=1, compare_logs=True, deal_algo=F.ALGO[group[1]], policy=steering.POLICIES[group[0]],
                                  sp_rows_checked=v4, threads=8, verbose=False)
    if group[0] in steering.NEVER_ENDING:
        # (every table plays on to the group's last stop cycle; the run ends earlier only when every hanchan has ended, by a seat
        # below zero or in the West round, and then all final scores were compared)
        assert st["cycles"] == last or st["scores_checked"] == len(tables), (st["cycles"], last, st["scores_checked"])
    else:
        assert st["scores_checked"] == len(tables)
    if v4:
        assert st["counters"]["sp_overflow"] == 0
    assert st["obs_checked"] > 0 and st["log_events_checked"] > 0
    census = {s: F.tables_showing(st["device_logs"], where, s) for s, _, where in wanted}
    print("situation census", group, len(tables), "tables", st["cycles"], "cycles", census)
    for situation, count, _ in wanted:
        assert census[situation] >= count, (situation, census)
