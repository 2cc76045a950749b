"""tests/golden/table_error_plan.json against the oracle alone (the staleness check of the fixture; tools/find_table_error_plan.py
writes it): every entry still applies -- the row exists on its cycle and the poisoned value is no legal answer of it --, the
victims sit where the plan promises, and the generator still produces the committed file."""
import table_error_cases as T


def test_every_plan_entry_applies_on_the_oracle(oracle):
    for name, run in T.plan()["runs"].items():
        fired, deals = T.replay_oracle_alone(oracle, run)
        assert fired == len(run["entries"]) > 0, (name, fired)  # zero skipped entries
        assert deals == sum(1 for e in run["entries"] if "deal_neighbour" in e), name


def test_plan_covers_the_kinds_and_the_places():
    runs = T.plan()["runs"]
    main = runs["main"]["entries"]
    assert runs["main"]["n_tables"] == 160  # two blocks of 64 and a half block: the last wavefront has padding lanes
    kinds = {e["kind"] for r in runs.values() for e in r["entries"]}
    assert kinds == set(T.KINDS)
    for r in runs.values():
        tables = [e["table"] for e in r["entries"]]
        assert len(set(tables)) == len(tables) and max(tables) < r["n_tables"]  # a table dies once
        for e in r["entries"]:
            assert e["row"] == ("kan" if e["kind"] in T.KAN_KINDS else "main")
            assert e["kind"] not in T.FIXED or e["value"] == T.FIXED[e["kind"]]
    values = {e["value"] for e in main}
    assert {45, 46, 1000, -1, T.INT32_MIN} <= values
    lanes = {(e["table"] >> 6, e["table"] & 63) for e in main}
    assert any(l == 0 for _, l in lanes) and any(l == 63 for _, l in lanes)
    assert any(b == 2 for b, _ in lanes) and (2, 31) in lanes  # the half block, and its last real lane beside the padding
    same = {}
    for e in main:
        same.setdefault((e["cycle"], e["table"] >> 6), []).append(e)
    assert any(len(v) >= 2 for v in same.values())  # two victims of one wavefront on one cycle
    deal = [e for e in main if "deal_neighbour" in e]
    dead_by = {e["table"]: e["cycle"] for e in main}
    assert deal and all(e["deal_neighbour"] >> 6 == e["table"] >> 6 and dead_by.get(e["deal_neighbour"], 1 << 30) > e["cycle"] for e in deal)
    pass45 = [e for e in main if e["kind"] == "pass_own_turn"]
    assert pass45 and all(e["value"] == 45 for e in pass45)
    assert not runs["kan_select"]["quick_eval"] and runs["main"]["quick_eval"]


def test_log_capacity_still_overflows_every_table(oracle):
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "find_table_error_plan.py")
    spec = importlib.util.spec_from_file_location("find_table_error_plan", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    lo = T.plan()["log_overflow"]
    assert lo["n_tables"] == 160
    assert gen.overflow_ok(T, T.overflow_profile(T.overflow_forecast(oracle, 160), lo["words_per_table"]))


def test_generator_reproduces_the_committed_plan(oracle, tmp_path, monkeypatch):
    import importlib.util
    import json
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "find_table_error_plan.py")
    spec = importlib.util.spec_from_file_location("find_table_error_plan", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = tmp_path / "plan.json"
    monkeypatch.setattr(T, "PLAN_PATH", str(out))
    gen.main()
    committed = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_error_plan.json")
    with open(committed) as f:
        assert json.loads(out.read_text()) == json.load(f)
