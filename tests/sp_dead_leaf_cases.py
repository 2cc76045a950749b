"""Shared by tests/test_sp_dead_leaf.py (emulator) and tests/test_gpu_sp_dead_leaf.py (device): a staggered, refilling pool in lock-step
with the oracle (parity_util.run_lockstep), pre-rolled in obs v3 -- no SP kernel, the oracle follows with masks and row lists -- and
then switched to obs v4 for a window in which EVERY row's whole obs (SP rows 889..1011 included) is compared f32 bit for bit.

What the window is for: rows with as many draws left as their shanten number (mj_sp.hip: leaf_dead).  Their last draw only reaches
tenpai, so mj_k_sp writes their level-1 child lists without looking for the children (sp_expand_dead_chunk) and neither builds nor
evaluates level 0.  From the oracle's own snapshots of the compared rows (real_time_shanten, tiles_left, can_discard, target_actor:
agent_helper.rs:467-530) `census` counts those rows, their shanten numbers and their neighbours on both sides of the boundary; the
kernel's own count of the rows that took the path (sp_phase_ticks: dead_leaf_rows) must equal the oracle's."""
import numpy as np

import parity_util


def classify(sn, seat):
    """(s, T, can_discard, graph) of a decision row from the oracle's PlayerState snapshot, as sp_row_front derives them; None: the row
    has no single-player tables at all (the Err path of obs_repr.rs:612-623)."""
    s, tiles_left = sn["real_time_shanten"], sn["tiles_left"]
    can_discard = bool(sn["cans"]["can_discard"])
    if can_discard:
        T = tiles_left // 4
    else:
        target = (sn["cans"]["target_actor"] + 4 - seat) & 3
        T = max(tiles_left - (4 - target), 0) // 4
    if not (tiles_left >= 4 and s >= 0 and T >= 1):
        return None
    return s, T, can_discard, (s <= 3 and T >= s)


def census(rows):
    """rows: the (s, T, can_discard, graph) of every compared row."""
    dead = [r for r in rows if r[3] and r[0] >= 1 and r[1] == r[0]]
    return dict(rows=len(rows), graph=sum(1 for r in rows if r[3]), dead=len(dead),
                dead_by_s={s: sum(1 for r in dead if r[0] == s) for s in (1, 2, 3)},
                dead_no_discard=sum(1 for r in dead if not r[2]),
                one_more_draw=sum(1 for r in rows if r[3] and r[0] >= 1 and r[1] == r[0] + 1),   # T == s + 1: level 0 alive, one turn wide
                one_draw_short=sum(1 for r in rows if 1 <= r[0] <= 3 and r[1] == r[0] - 1))      # T == s - 1: no graph at all


def recording_policy(oracle, seen, first_cycle):
    """The uniform-random legal policy of run_lockstep, which also notes the census class of every row from `first_cycle` on."""
    def policy(arena, masks, rows, cycle):
        if cycle >= first_cycle:
            for g, seat, _ in rows.tolist():
                c = classify(arena.player_state(int(g), int(seat)).snapshot(), int(seat))
                if c is not None:
                    seen.append(c)
        return oracle.random_actions(masks, rows, cycle)
    return policy


def switching_pool(base_cls, pre, ticks_out):
    """`base_cls` encoding obs v3 for the first `pre` cycles and obs v4 from then on.  run_lockstep sizes its obs buffer for v4 all
    along (`versions` keeps saying 4), the pre-roll's encode writes its v3 rows into the front of that buffer; nobody reads them (the
    policy reads the oracle side, obs are compared from cycle `pre` on).  close() leaves the pool's sp_phase_ticks in `ticks_out`."""
    from mortal_amd.pool import OBS_ROWS

    class SwitchingPool(base_cls):
        _cycle = 0

        def step(self, *a, **k):
            want = 3 if self._cycle < pre else 4
            if self._cycle in (0, pre):
                base_cls.configure(self, 0, version=want)
                self._encodes_v3 = want == 3
                self.versions[0] = 4
            self._cycle += 1
            return base_cls.step(self, *a, **k)

        def encode(self, agent, obs=None, masks=None):
            if agent == 0 and self._encodes_v3 and obs is not None:
                n = self.n_rows[0]
                assert obs.is_contiguous() and obs.shape[1] >= OBS_ROWS[3]
                self.versions[0] = 3
                try:
                    base_cls.encode(self, 0, obs.view(-1)[: n * OBS_ROWS[3] * 34].view(n, OBS_ROWS[3], 34), masks)
                finally:
                    self.versions[0] = 4
                return obs[:n], masks[:n]
            return base_cls.encode(self, agent, obs, masks)

        def close(self):
            if getattr(self, "h", None):
                ticks_out.update(self.sp_phase_ticks())
            base_cls.close(self)

    return SwitchingPool


def run(oracle, base_cls, n_tables, pre, window, threads=0):
    """-> (run_lockstep's stats, census of the compared rows, the pool's sp_phase_ticks at the end)."""
    seen, ticks = [], {}
    st = parity_util.run_lockstep(oracle, n_tables, version=4, max_cycles=pre + window, obs_cycles=set(range(pre, pre + window)),
                                  sp_rows_checked=True, refill=n_tables // 4, stagger=pre, min_games=99, deal_algo=1, verbose=False, threads=threads,
                                  policy=recording_policy(oracle, seen, pre), pool_cls=switching_pool(base_cls, pre, ticks))
    assert st["cycles"] == pre + window and st["counters"]["steps"] == st["oracle_steps"]
    return st, census(seen), ticks


def check(st, c, ticks, scale):
    """The conditions of a 64-table window, times `scale`."""
    print("dead-leaf census of the compared rows:", c, "| kernel:", {k: ticks[k] for k in ("rows", "states", "dead_leaf_rows", "overflow")},
          "|", st["sp_schedule"])
    assert st["obs_checked"] >= c["rows"] > 0  # (every row of the window was compared; the census leaves out the rows without SP tables)
    assert c["dead"] >= 30 * scale and c["dead_by_s"][3] >= 8 * scale and c["dead_no_discard"] >= 3 * scale, c
    assert c["dead_by_s"][1] >= scale and c["dead_by_s"][2] >= scale, c
    assert c["one_more_draw"] >= scale and c["one_draw_short"] >= scale, c
    assert ticks["dead_leaf_rows"] == c["dead"], (ticks["dead_leaf_rows"], c)
    assert st["counters"]["sp_overflow"] == 0 and ticks["overflow"] == 0  # (emulator: + its uniqueness, hit and keep-set checks)
