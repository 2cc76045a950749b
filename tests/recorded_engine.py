"""Recorded reference engines: what the reference's Python engines (mortal/engine.py) answered, replayed from fixtures under
tests/golden/ (made by tests/golden/record_reference_engines.py where the reference tree exists), so that the tests which play
them need nothing outside this repository.

  reference_engines.json      rankings and seeds of each case, the example mjai-log engine's record
  reference_decisions.npy     uint64 [n]: decision key << 9 | (case * 2 + engine) << 6 | action; engine 0 = challenger, 1 = champion
  reference_top_p_freq.npy    float64 [top_p, row, 46]: sample_top_p's action frequencies"""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "reference_engines.json")
DECISIONS = os.path.join(GOLDEN, "reference_decisions.npy")
TOP_P_FREQ = os.path.join(GOLDEN, "reference_top_p_freq.npy")
CASES = ("v4", "v2", "cfg0")
ENGINES = ("challenger", "champion")


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def decisions(case, engine):
    """{decision key: action} of one recorded engine."""
    d = np.load(DECISIONS)
    d = d[(d >> 6) & 7 == 2 * CASES.index(case) + ENGINES.index(engine)]
    return dict(zip((d >> 9).tolist(), (d & 63).tolist()))


def decision_key(obs, mask):
    """One decision of a 'mortal'-type engine: its obs tensor (f32) and legal-action mask, bit for bit (55 bits of a sha1)."""
    h = hashlib.sha1(np.ascontiguousarray(obs, dtype=np.float32).tobytes())
    h.update(np.ascontiguousarray(mask, dtype=bool).tobytes())
    return int.from_bytes(h.digest()[:8], "little") >> 9


def _stacked(batch):
    """The engine contract's batch (a list of per-row arrays, or the arena's stacked proxy) as a host numpy array."""
    import torch

    return torch.as_tensor(np.stack(batch, axis=0)).cpu().numpy()


class RecordedEngine:
    """A 'mortal'-type engine (agent/py_agent.rs:24-37) that answers every decision with the action the reference's
    MortalEngine chose for the same obs + mask.  A decision the reference engine never saw is an error: the obs this engine
    receives must equal, bit for bit, what the reference engine received on the oracle loop."""

    engine_type = "mortal"
    is_oracle = False
    enable_quick_eval = True
    enable_rule_based_agari_guard = False

    def __init__(self, decisions, version, name):
        self.decisions = decisions
        self.version = version
        self.name = name
        self.calls = 0

    def react_batch(self, obs, masks, invisible_obs):
        obs, masks = _stacked(obs), _stacked(masks).astype(bool)
        actions = []
        for o, m in zip(obs, masks):
            k = decision_key(o, m)
            if k not in self.decisions:
                raise AssertionError(f"{self.name}: a decision the reference engine never met (obs / mask differ from the oracle loop's)")
            actions.append(int(self.decisions[k]))
        self.calls += 1
        n = len(actions)
        return actions, np.zeros((n, masks.shape[1]), np.float32).tolist(), masks.tolist(), [True] * n


def example_engine_states():
    """Synthetic GameState inputs of ExampleMjaiLogEngine.react_batch: the two PlayerState members it reads (last_cans.can_discard,
    last_self_tsumo()) and a kyoku log whose first event is start_kyoku."""
    from types import SimpleNamespace as NS

    from mortal_amd.arena import GameState

    cases = [(0, True, "5mr"), (1, False, "E"), (2, True, "9s"), (3, True, "C"), (1, True, "1p"), (3, False, "?")]
    return [GameState(g, NS(last_cans=NS(can_discard=d), last_self_tsumo=lambda t=t: t),
                      json.dumps([{"type": "start_kyoku"}, {"type": "tsumo", "actor": 0, "pai": t}])) for g, d, t in cases]
