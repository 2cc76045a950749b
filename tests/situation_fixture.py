"""Reader of tests/golden/situation_seeds.json (written by tools/find_situation_seeds.py) for the three situation test modules."""
import json
import os

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "situation_seeds.json")
ALGO = {"rand08": 0, "rand09": 1}


def load():
    with open(PATH) as f:
        return json.load(f)


def entries():
    return load()["entries"]


def groups():
    """-> {(policy, deal_algo name): (tables, wanted)}: every fixture table of the pair once, in nonce order, as
    (nonce, key, stop_cycle), and per entry of the pair (situation, count, [(index into tables, kyoku)])."""
    out = {}
    for e in entries():
        tables, wanted = out.setdefault((e["policy"], e["deal_algo"]), ({}, []))
        for t in e["tables"]:
            old = tables.get(t["nonce"])
            tables[t["nonce"]] = (t["nonce"], t["key"], max(t["stop_cycle"], old[2] if old else 0))
        wanted.append((e["situation"], e["count"], [(t["nonce"], t["kyoku"]) for t in e["tables"]]))
    for key, (tables, wanted) in out.items():
        order = sorted(tables)
        index = {nonce: i for i, nonce in enumerate(order)}
        out[key] = ([tables[n] for n in order], [(s, c, [(index[n], k) for n, k in where]) for s, c, where in wanted])
    return out


def tables_showing(logs, where, situation):
    """How many of the (table index, kyoku) places hold `situation` according to the census of `logs[table]`."""
    import situation_census

    n = 0
    for t, k in where:
        per = situation_census.census_by_kyoku(logs[t])
        bad = [s for c in per for s in c if s.startswith("mismatch:")]
        assert not bad, (t, bad)
        n += k < len(per) and per[k][situation] > 0
    return n
