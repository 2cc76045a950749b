"""The fixture tests/golden/situation_seeds.json cannot go stale silently: for every entry the oracle alone replays the entry's seeds
under the entry's steering policy, and the census of its event logs must show the entry's situation, in the recorded kyoku, in at
least the recorded number of tables.  If the oracle, a policy or the census changes what these games do, this fails: run
tools/find_situation_seeds.py again (tools/README.md) and commit the regenerated file."""
import pytest
import situation_fixture as F
import steering

import tools.find_situation_seeds as finder


def test_fixture_covers_every_target_and_both_deal_algorithms():
    doc = F.load()
    have = {e["situation"] for e in doc["entries"]}
    assert set(doc["not_found"]) <= set(finder.MAY_BE_MISSING) and len(doc["not_found"]) <= 3
    assert have | set(doc["not_found"]) | set(finder.OPTIONAL) >= set(finder.TARGETS)
    assert {e["deal_algo"] for e in doc["entries"]} == {"rand08", "rand09"}
    # (rare even under steering: the search of `kyoku_searched` kyoku holds fewer than eight tables of them)
    rare = ("pao_ron_split_paid", "pao_tsumo_paid", "pao_set_daisuushi", "ron_triple", "ron_on_ankan", "tenhou", "first_turn_win",
            "four_kans_one_seat_play_goes_on", "nagashi_mangan_2", "pao_ron_from_liable")
    for e in doc["entries"]:
        assert e["count"] == len(e["tables"]) >= (2 if e["situation"] in rare else 8), e["situation"]
        assert e["policy"] in steering.POLICIES


@pytest.mark.parametrize("group", sorted(F.groups()), ids=lambda g: f"{g[0]}-{g[1]}")
def test_oracle_replay_reaches_the_recorded_situations(oracle, group):
    tables, wanted = F.groups()[group]
    arena, _ = steering.play_oracle(oracle, [(n, k) for n, k, _ in tables], group[0], deal_algo=F.ALGO[group[1]],
                                    max_cycles=max(stop for _, _, stop in tables))
    logs = [arena.log(g) for g in range(len(tables))]
    for situation, count, where in wanted:
        assert F.tables_showing(logs, where, situation) >= count, situation
