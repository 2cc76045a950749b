#!/usr/bin/env python3
"""Record what the reference's Python engines (mortal/engine.py, mortal/model.py) do, as the fixtures
tests/golden/reference_{engines.json,decisions.npy,top_p_freq.npy} (layout: tests/recorded_engine.py).  Runs where the
reference tree exists; the tests only read the fixtures.

usage: python tests/golden/record_reference_engines.py <the reference's mortal/ directory>

Recorded (data only, no reference code):
  top_p_freq      sample_top_p (engine.py:83-94) action frequencies on tests/test_policy_sampling.py's fixture, per top_p
  example_engine  ExampleMjaiLogEngine (engine.py:96-140): engine_type, player ids, reactions on synthetic game states
  one_vs_three    per case, the decisions (sha1 of obs + mask -> action) of the two MortalEngine instances of
                  tests/test_reference_engine.py / tests/test_one_vs_three_script.py on the oracle loop, and its rankings
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)


def _tiny(ref_model, version, seed):
    """A random-init tiny model pair (Brain 16 channels x 1 block, DQN) after torch.manual_seed(seed)."""
    import torch

    torch.manual_seed(seed)
    return ref_model.Brain(version=version, conv_channels=16, num_blocks=1), ref_model.DQN(version=version)


def main(ref):
    for p in (ROOT, TESTS, os.path.join(ROOT, "compat"), os.path.join(TESTS, "host")):
        if p not in sys.path:
            sys.path.insert(0, p)
    sys.path.append(ref)  # the repository's `libriichi` must win over anything in the reference tree
    import torch

    import engine as ref_engine
    import model as ref_model
    import oracle_lib
    import recorded_engine as R
    import test_one_vs_three_script as T3
    import test_policy_sampling as TP
    import test_reference_engine as TR
    from mortal_amd.pool import default_deal_algo

    oracle_lib.lib()
    out = {"source": "the reference's mortal/engine.py + mortal/model.py, recorded by tests/golden/record_reference_engines.py"}

    # sample_top_p: the frequencies test_nucleus_frequencies_match_reference compares with (same fixture, seed, draws)
    q, masks = TP._fixture()
    logits = (q / 0.7).masked_fill(~masks, -torch.inf)
    freq = []
    for top_p in TP.TOP_PS:
        torch.manual_seed(12)
        theirs = ref_engine.sample_top_p(logits.repeat_interleave(TP.N_DRAWS, 0).clone(), top_p).view(-1, TP.N_DRAWS)
        freq.append([np.bincount(theirs[r].numpy(), minlength=46) / TP.N_DRAWS for r in range(len(q))])
    np.save(R.TOP_P_FREQ, np.asarray(freq, dtype=np.float64))
    out["top_p"] = {"values": TP.TOP_PS, "draws": TP.N_DRAWS}

    # ExampleMjaiLogEngine on synthetic game states
    eng = ref_engine.ExampleMjaiLogEngine("logger")
    ex = {"engine_type": eng.engine_type, "name": eng.name, "player_ids_before": eng.player_ids}
    eng.set_player_ids([0, 2, 1, 3])
    ex["player_ids"] = eng.player_ids
    ex["reactions"] = eng.react_batch(R.example_engine_states())
    ex["callbacks"] = [eng.start_game(0), eng.end_kyoku(0), eng.end_game(0, [25000] * 4)]
    bad = R.example_engine_states()[:1]
    bad[0].events_json = json.dumps([{"type": "tsumo"}])
    try:
        eng.react_batch(bad)
        ex["not_start_kyoku_raises"] = None
    except AssertionError:
        ex["not_start_kyoku_raises"] = "AssertionError"
    out["example_engine"] = ex

    # MortalEngine pairs on the oracle loop (arena/game.rs:286-304)
    class Recorder:
        def __init__(self, eng):
            self.eng, self.decisions = eng, {}

        def react_batch(self, obs, masks, invisible_obs):
            res = self.eng.react_batch(obs, masks, invisible_obs)
            for o, m, a in zip(obs, masks, res[0]):
                k = R.decision_key(o, m)
                assert self.decisions.setdefault(k, int(a)) == int(a)
            return res

    cases = {}
    for case, version, key, seed_count in (("v4", 4, TR.KEY, 1), ("v2", 2, TR.KEY, 1), ("cfg0", T3.VERSION, T3.KEY, 2)):
        chal, cham = (Recorder(ref_engine.MortalEngine(*_tiny(ref_model, version, seed), is_oracle=False, version=version,
                                                       device=torch.device("cpu"), name=name, enable_amp=False, enable_quick_eval=True,
                                                       enable_rule_based_agari_guard=False))
                      for seed, name in ((1, "challenger"), (2, "champion")))
        rk = TR._oracle_rankings(oracle_lib, chal, cham, (10000, key), seed_count, version, default_deal_algo())
        cases[case] = {"version": version, "seed_start": [10000, key], "seed_count": seed_count, "rankings": rk,
                       "decisions": (chal.decisions, cham.decisions)}
    rows = [k << 9 | (2 * R.CASES.index(c) + e) << 6 | a for c in R.CASES for e, dec in enumerate(cases[c].pop("decisions"))
            for k, a in dec.items()]
    np.save(R.DECISIONS, np.asarray(rows, dtype=np.uint64))
    out["one_vs_three"] = cases
    with open(R.FIXTURE, "w") as f:  # one line per entry
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print({p: os.path.getsize(p) for p in (R.FIXTURE, R.DECISIONS, R.TOP_P_FREQ)}, {k: v["rankings"] for k, v in cases.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
