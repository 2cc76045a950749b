"""Action policies that steer lock-step games into rule branches which random and tenpai-seeking play do not reach.

Each policy is a callable `(arena, masks, rows, cycle) -> int32 actions` for `parity_util.run_lockstep(policy=...)`.  It reads the
oracle side only (the masks, the row list, `arena.player_state(g, s).snapshot()`, `arena.game_view(g)` and the oracle's own event
log), so seeds can be searched with the oracle alone and the device has no say in its own action stream.  No policy looks at the
table index or at anything that differs between batches: a table plays the same game wherever it sits in a pool, which is what lets
tools/find_situation_seeds.py search in big batches and the tests replay any subset.  Every action is legal (asserted).

Actions: 0..36 discard (34..36 the red fives), 37 riichi, 38..40 chi, 41 pon, 42 kan, 43 agari, 44 kyuushu kyuuhai, 45 pass; on a
kan-select row the mask is over the tile kinds that can be declared."""
import numpy as np

_AKA = {4: 34, 13: 35, 22: 36}
_YAOKYUU = (0, 8, 9, 17, 18, 26, 27, 28, 29, 30, 31, 32, 33)
_WINDS = (27, 28, 29, 30)


def _legal_discards(m):
    """-> {tile kind 0..33: action} of the discards the mask allows (the plain five before the red one)."""
    out = {}
    for t in range(34):
        if m[t]:
            out[t] = t
        elif t in _AKA and m[_AKA[t]]:
            out[t] = _AKA[t]
    return out


def _pick(cands, salt):
    cands = sorted(cands)
    return cands[salt % len(cands)]


def _shanten_discard(m, sn, salt, avoid=()):
    """A discard that lowers the shanten number, else one that keeps it, else any; tiles in `avoid` only when nothing else is legal."""
    legal = _legal_discards(m)
    pool = [t for t in legal if t not in avoid] or list(legal)
    for pref in (sn["next_shanten_discards"], sn["keep_shanten_discards"]):
        c = [t for t in pool if pref[t]]
        if c:
            return legal[_pick(c, salt)]
    return legal[_pick(pool, salt)]


def _last_event(arena, g):
    """The newest event of the table's log, a kan's `dora` skipped."""
    log = arena.log(g)
    k = len(log) - 1
    while log[k]["type"] == "dora":
        k -= 1
    return log[k]


def _drive(decide):
    """Wrap a per-row rule `decide(arena, m, g, seat, sn, cycle) -> action` into a batch policy."""

    def policy(arena, masks, rows, cycle):
        masks = np.asarray(masks, dtype=bool)
        act = np.full(len(masks), 45, dtype=np.int32)
        for r in range(len(masks)):
            m = masks[r]
            g, seat = int(rows[r][0]), int(rows[r][1])
            if rows[r][2]:  # kan-select row: the lowest tile kind that can be declared
                act[r] = int(np.flatnonzero(m)[0])
            else:
                act[r] = decide(arena, m, g, seat, arena.player_state(g, seat).snapshot(), cycle)
            assert m[act[r]], (cycle, rows[r].tolist(), int(act[r]), np.flatnonzero(m).tolist())
        return act

    return policy


def _fallback(m):
    """No preferred action applies: pass if that is legal, else the lowest legal action (a forced agari included)."""
    return 45 if m[45] else int(np.flatnonzero(m)[0])


def _kan_seeking(arena, m, g, seat, sn, cycle):
    """Always kan and pon; keep pairs and triplets; win only from a kan (rinshan tsumo, ron on a kakan / ankan).  In every other
    kyoku (kyoku + honba odd) only the seat opposite the dealer calls, kans alone, and the others discard what it holds three of
    (they look at its hand in the oracle) and keep what it holds two of: four kans in one hand, after which play goes on."""
    if m[43]:
        if sn["cans"]["can_tsumo_agari"]:
            if sn["at_rinshan"]:
                return 43
        elif _last_event(arena, g)["type"] in ("kakan", "ankan"):
            return 43
    v = arena.game_view(g)
    solo = ((int(v[10]) + 2) & 3) if (int(v[1]) + int(v[2])) & 1 else None
    if solo is None or seat == solo:
        if m[42]:
            return 42
        if m[41] and solo is None:
            return 41
    legal = _legal_discards(m)
    if legal:
        tehai = sn["tehai"]
        if solo is None or seat == solo:
            key = lambda t: (tehai[t] >= 2, not sn["next_shanten_discards"][t], not sn["keep_shanten_discards"][t])
        else:
            held = arena.player_state(g, solo).snapshot()["tehai"]
            key = lambda t: (held[t] != 3, held[t] == 2, tehai[t])
        best = min(key(t) for t in legal)
        return legal[_pick([t for t in legal if key(t) == best], cycle + seat)]
    return _fallback(m)


def _closed_riichi_no_win(arena, m, g, seat, sn, cycle):
    """No calls, always riichi, shanten-lowering discards, never agari while anything else is legal."""
    if m[37]:
        return 37
    if _legal_discards(m):
        return _shanten_discard(m, sn, cycle + seat)
    return _fallback(m)


def _terminal_discards(arena, m, g, seat, sn, cycle):
    """No calls, no riichi, no win: terminals and honours go first, for as long as the seat holds one."""
    legal = _legal_discards(m)
    if legal:
        yao = [t for t in legal if t in _YAOKYUU]
        if yao:
            return legal[_pick(yao, cycle + seat)]
        tehai = sn["tehai"]
        fewest = min(tehai[t] for t in legal)
        return legal[_pick([t for t in legal if tehai[t] == fewest], cycle + seat)]
    return _fallback(m)


def _first_go_around_discards(arena, g, seat):
    """The discards of the other three seats as `seat` sees them (its own river is empty while it can still double-riichi)."""
    ps = arena.player_state(g, seat)
    return [(int(e) >> 1) & 63 for rel in (1, 2, 3) for e in ps.kawa(rel) if int(e) & 1]


def _wind_discards(arena, m, g, seat, sn, cycle):
    """`_terminal_discards`, but the first go-around follows the wind: a seat that holds the wind which every discard so far shows
    discards it too, and the first seat opens with a wind (one it holds once before one it holds more often).  Kyuushu kyuuhai
    is declared when `seat + cycle` is odd: both the abort and the kyoku played on from such a hand occur."""
    if m[44] and (seat + cycle) & 1:
        return 44
    legal = _legal_discards(m)
    # (`can_w_riichi`: the seat has not discarded and nobody has called or declared a kan, so the rivers are read four times
    # per kyoku at the most)
    if legal and sn["can_w_riichi"]:
        seen = _first_go_around_discards(arena, g, seat)
        if not seen:
            winds = [t for t in _WINDS if t in legal]
            if winds:
                tehai = sn["tehai"]
                return legal[_pick([t for t in winds if tehai[t] == 1] or winds, cycle + seat)]
        elif len(set(seen)) == 1 and seen[0] in _WINDS and seen[0] in legal:
            return legal[seen[0]]
    return _terminal_discards(arena, m, g, seat, sn, cycle)


def _calling_terminal_discards(arena, m, g, seat, sn, cycle):
    """The seat opposite the dealer calls every pon and chi it can and discards its non-terminals first; the other three play
    `_terminal_discards`.  A terminal-only river that loses a tile to the caller is no nagashi mangan at the exhaustive draw."""
    if seat != ((int(arena.game_view(g)[10]) + 2) & 3):
        return _terminal_discards(arena, m, g, seat, sn, cycle)
    for a in (41, 38, 39, 40):
        if m[a]:
            return a
    legal = _legal_discards(m)
    if legal:
        plain = [t for t in legal if t not in _YAOKYUU]
        return legal[_pick(plain or list(legal), cycle + seat)]
    return _fallback(m)


def _first_go_around(arena, m, g, seat, sn, cycle):
    """Wins in the first go-around: everybody wins when possible, nobody calls or declares riichi, and a seat that has not discarded
    yet discards a tile that a seat still to come waits on (it looks at their hands in the oracle) if it holds one.  After its
    first discard a seat plays shanten-lowering discards."""
    if m[43]:
        return 43
    legal = _legal_discards(m)
    if legal:
        if sn["can_w_riichi"]:
            fed = set()
            for other in range(4):
                o = arena.player_state(g, other).snapshot() if other != seat else None
                if o is not None and o["can_w_riichi"]:
                    fed.update(t for t in legal if o["waits"][t])
            if fed:
                return legal[_pick(fed, cycle + seat)]
        return _shanten_discard(m, sn, cycle + seat)
    return _fallback(m)


def _honour_hoarding(arena, m, g, seat, sn, cycle):
    """The seat opposite the dealer keeps every honour and pons each one it can (and anything else once it has two melds).  The
    other three stay closed, declare riichi and discard honours on sight: first one the hoarder holds a pair of (they look at the
    hoarder's hand in the oracle), then dragons, then winds.  Everybody wins when possible."""
    if m[43]:
        return 43
    hoarder = (int(arena.game_view(g)[10]) + 2) & 3
    honours = range(27, 34)
    if seat == hoarder:
        if m[41] or (m[42] and not _legal_discards(m)):
            pai = _last_event(arena, g).get("pai")
            is_honour = pai in ("E", "S", "W", "N", "P", "F", "C")
            if m[41] and (is_honour or sn["tehai_len_div3"] <= 2):
                return 41
            if m[42] and is_honour and not m[41]:
                return 42
        if _legal_discards(m):
            return _shanten_discard(m, sn, cycle + seat, avoid=honours)
        return _fallback(m)
    if m[37]:
        return 37
    legal = _legal_discards(m)
    if legal:
        held = arena.player_state(g, hoarder).snapshot()["tehai"]
        for c in ([t for t in honours if t in legal and held[t] >= 2], [t for t in (31, 32, 33) if t in legal],
                  [t for t in (27, 28, 29, 30) if t in legal]):
            if c:
                return legal[_pick(c, cycle + seat)]
        return _shanten_discard(m, sn, cycle + seat)
    return _fallback(m)


def _everybody_rons(arena, m, g, seat, sn, cycle):
    """Always agari, always riichi, shanten-lowering discards, a pon on one decision in eight."""
    if m[43]:
        return 43
    if m[37]:
        return 37
    if _legal_discards(m):
        return _shanten_discard(m, sn, cycle + seat)
    if m[41] and (cycle * 5 + seat * 3) % 8 == 0:
        return 41
    return _fallback(m)


POLICIES = {
    "kan_seeking": _drive(_kan_seeking),
    "closed_riichi_no_win": _drive(_closed_riichi_no_win),
    "terminal_discards": _drive(_terminal_discards),
    "honour_hoarding": _drive(_honour_hoarding),
    "everybody_rons": _drive(_everybody_rons),
    "wind_discards": _drive(_wind_discards),
    "calling_terminal_discards": _drive(_calling_terminal_discards),
    "first_go_around": _drive(_first_go_around),
}
# policies whose tables run to their recorded stop cycle and no further: under the first five nobody wins by choice and the games
# need not end; `first_go_around` is searched over the first cycles of very many hanchan, of which nothing more is known
NEVER_ENDING = ("kan_seeking", "closed_riichi_no_win", "terminal_discards", "wind_discards", "calling_terminal_discards",
                "first_go_around")


def _non_dealer_tenpai_at_deal(arena, g):
    oya = int(arena.game_view(g)[10])
    return any(arena.player_state(g, s).snapshot()["shanten"] == 0 for s in range(4) if s != oya)


# policy -> `(arena, table) -> bool`, asked after the first poll: can the hanchan's first kyoku reach what the policy was written
# for?  tools/find_situation_seeds.py plays on only the tables that can (a win by a non-dealer in the first go-around needs a hand
# that is tenpai as dealt: one deal in some thousand).  A test replays a seed whatever this says.
DEAL_FILTER = {"first_go_around": _non_dealer_tenpai_at_deal}


def play_oracle(oracle, seeds, policy, deal_algo=0, max_cycles=6000, version=3):
    """The oracle alone under `policy` (a name of POLICIES or a callable): -> (arena, kyoku_ends) where kyoku_ends[g] lists the cycle
    in which each finished kyoku of table g ended.  Stops when every table has finished or reached `max_cycles`."""
    if isinstance(policy, str):
        policy = POLICIES[policy]
    arena = oracle.Arena(seeds, deal_algo=deal_algo, enable_quick_eval=True, version=version, keep_log=True)
    n = len(seeds)
    ends = [[] for _ in range(n)]
    seen = [None] * n
    for cycle in range(max_cycles):
        rows = arena.poll()
        for g in range(n):
            v = arena.game_view(g)
            key = (int(v[1]), int(v[2]), int(v[0]))
            if seen[g] is not None and key != seen[g] and not seen[g][2]:
                ends[g].append(cycle)
            seen[g] = key
        if len(rows) == 0 and arena.n_live == 0:
            break
        _, masks = arena.encode(0, len(rows), want_obs=False)
        arena.commit(policy(arena, masks, rows, cycle))
    return arena, ends
