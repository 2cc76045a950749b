"""Shared by tests/test_gpu_sp_eval_packed.py and the seed search behind it: a staggered, refilling 64-table pool under the greedy policy,
obs v4 all along, in lock-step with the oracle; in a window after the stagger EVERY row's whole obs (SP rows 889..1011 included) is
compared f32 bit for bit.

What the window is for: the triangular sums of mj_k_sp's evaluation (mj_sp.hip: sp_eval_wave0 / sp_eval_wave) run on pairs of terms,
and a team is T - off lanes wide (T = the row's draws left, off = the state's depth below the row's roots), so a lane's term count is
odd or even with T, the three instantiations split at T <= 8 / <= 16 / 17, and the parked rows' zero fill pads every count to a
multiple of four.  A row of shanten s with T >= s runs sp_eval_wave0 at off = s, sp_eval_wave<.., 1> at off = s - 1 and
sp_eval_wave<.., 2> at the offsets above: rows of every shanten 0..3 in each of the three T ranges cover off 0..3 of every
instantiation.  `census` counts them from the oracle's own snapshots of the compared rows (sp_dead_leaf_cases.classify)."""
import parity_util
import sp_dead_leaf_cases

N_TABLES, PRE, WINDOW = 64, 160, 48
REFILL = 16


def tn_of(T):
    return 8 if T <= 8 else 16 if T <= 16 else 17


def census(seen):
    """seen: (s, T, can_discard, graph) of every compared row -> the rows with a graph by (instantiation, shanten), and by T."""
    by_case, by_T = {}, {}
    for s, T, _, graph in seen:
        if graph:
            T = min(T, 17)
            by_case[(tn_of(T), s)] = by_case.get((tn_of(T), s), 0) + 1
            if T > s or s == 0:  # (T == s >= 1: the tenpai level is skipped, sp_expand_dead_chunk)
                by_T[T] = by_T.get(T, 0) + 1
    return by_case, by_T


class RecordingOracle:
    """The oracle module with a hold on the arena run_lockstep creates, for the pool below."""
    def __init__(self, oracle):
        self._oracle, self.arena = oracle, None

    def __getattr__(self, name):
        return getattr(self._oracle, name)

    def Arena(self, *a, **k):
        self.arena = self._oracle.Arena(*a, **k)
        return self.arena


def recording_pool(base_cls, rec, seen, first_cycle):
    """`base_cls` that notes, from `first_cycle` on, the census class of every row it encodes -- from the oracle's state of that row."""
    class RecordingPool(base_cls):
        _cycle = 0

        def step(self, *a, **k):
            self._cycle += 1
            return base_cls.step(self, *a, **k)

        def encode(self, agent, obs=None, masks=None):
            if agent == 0 and self._cycle > first_cycle:
                for g, seat, _ in self.rows(0).tolist():
                    c = sp_dead_leaf_cases.classify(rec.arena.player_state(int(g), int(seat)).snapshot(), int(seat))
                    if c is not None:
                        seen.append(c)
            return base_cls.encode(self, agent, obs, masks)

    return RecordingPool


def run(oracle, base_cls, threads=0):
    """-> (run_lockstep's stats, (by_case, by_T) of the compared rows)."""
    seen = []
    rec = RecordingOracle(oracle)
    st = parity_util.run_lockstep(rec, N_TABLES, version=4, max_cycles=PRE + WINDOW, obs_cycles=set(range(PRE, PRE + WINDOW)),
                                  sp_rows_checked=True, refill=REFILL, stagger=PRE, min_games=99, verbose=False, threads=threads,
                                  policy="greedy", pool_cls=recording_pool(base_cls, rec, seen, PRE))
    assert st["cycles"] == PRE + WINDOW and st["counters"]["steps"] == st["oracle_steps"]
    return st, census(seen)


def check(st, c):
    by_case, by_T = c
    print("compared rows with a graph by (instantiation, shanten):", sorted(by_case.items()), "| by T:", sorted(by_T.items()), "|",
          st["sp_schedule"])
    assert st["obs_checked"] >= sum(by_case.values()) > 0
    # every (instantiation, off): a row of shanten s evaluates at off 0..s
    missing = [(tn, off) for tn in (8, 16, 17) for off in (0, 1, 2, 3) if not any(by_case.get((tn, s)) for s in range(off, 4))]
    assert not missing, (missing, by_case)
    # and function by function (sp_eval_wave0 at off = s, sp_eval_wave<.., 1> at s - 1, <.., 2> above) -- but for a tenpai hand with
    # all 17 draws left (sp_eval_wave0<17> at off 0: a hand dealt tenpai), which the window does not hold: the oracle gives it
    # 169 / 359 / 180 / 27 rows of shanten 0..3 at T <= 8, 82 / 414 / 743 / 593 at T <= 16, 0 / 1 / 17 / 43 at T = 17
    missing = [(tn, s) for tn in (8, 16, 17) for s in (0, 1, 2, 3) if not by_case.get((tn, s)) and (tn, s) != (17, 0)]
    assert not missing, (missing, by_case)
    assert sorted(by_T) == list(range(1, 18)), by_T  # odd and even term counts of every width
    assert st["counters"]["sp_overflow"] == 0
