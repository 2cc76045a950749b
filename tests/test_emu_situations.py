"""The emulated DEVICE code in lock-step with the oracle through the rule branches that only the steering policies reach
(tests/steering.py; seeds from tests/golden/situation_seeds.json): nagashi mangan, the pao payments, the four-riichi and four-kan
aborts, four kans in one hand, multiple ron, chankan, rinshan, the first go-around, large kyotaku and honba, the West round.

Per situation the one fixture table whose kyoku ends earliest runs alone, up to a few cycles past the end of that kyoku (the games of
the no-win policies never end; a stopped table's logs are compared as prefixes of equal length, parity_util.run_lockstep): rows and
masks every cycle, obs every 7th cycle, every event.  Then the census of the DEVICE's own decoded log must show the situation in the
recorded kyoku.  Tables that serve several situations run once.  No situation of the fixture is left out of this leg."""
import os
import shutil
import sys

import pytest

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
if HOST not in sys.path:
    sys.path.insert(0, HOST)

import parity_util  # noqa: E402
import situation_fixture as F  # noqa: E402
import steering  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    import emu_pool

    return emu_pool.make_pool_class()


def _runs():
    """{(policy, algo, nonce, key): (cycles, [(situation, kyoku)])}: per situation its table with the earliest end of kyoku."""
    runs = {}
    for e in F.entries():
        t = min(e["tables"], key=lambda t: (t["kyoku_end_cycle"], t["nonce"]))
        key = (e["policy"], e["deal_algo"], t["nonce"], t["key"])
        cycles, sits = runs.get(key, (0, []))
        runs[key] = (max(cycles, t["kyoku_end_cycle"] + 3), sits + [(e["situation"], t["kyoku"])])
    return runs


RUNS = _runs()


def test_every_fixture_situation_has_an_emulator_table():
    assert {s for _, sits in RUNS.values() for s, _ in sits} == {e["situation"] for e in F.entries()}


@pytest.mark.parametrize("run", sorted(RUNS), ids=lambda r: f"{r[0]}-{r[1]}-{r[2]}")
def test_emu_lockstep_reaches_situation(oracle, emu, run):
    policy, algo, nonce, key = run
    cycles, sits = RUNS[run]
    st = parity_util.run_lockstep(oracle, 1, version=3, max_cycles=cycles, seeds=[(nonce, key)], obs_every=7, pool_cls=emu,
                                  compare_logs=True, deal_algo=F.ALGO[algo], policy=steering.POLICIES[policy], verbose=False)
    assert st["log_events_checked"] > 0 and st["obs_checked"] > 0
    for situation, kyoku in sits:
        assert F.tables_showing(st["device_logs"], [(0, kyoku)], situation) == 1, situation
