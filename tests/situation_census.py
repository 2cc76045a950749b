"""Which rule situations does a game log hold?  `census(events)` reads one decoded mjai event list (what `oracle_lib.Arena.log(g)`
and `mortal_amd.mjai_log.decode_events` produce, a whole hanchan or a prefix of one) and returns a Counter of named situations.

Pure Python on the events alone: neither the oracle nor the device code is asked anything, so the census can judge both.  The
names are those of SITUATIONS below; a key that starts with "mismatch:" means the log contradicts the rule the census derived from
the events themselves (exhaustive-draw payments from the seats' hands and discards, the payer of a pao win, the abort after four
equal winds), and no log of a correct engine holds one.

Rule references: the reference's arena/board.rs (step :511-678, exhaustive_ryukyoku :241-294, update_nagashi_mangan_and_four_wind
and check_four_wind :296-340, handle_hora :366-471, update_paos :473-499)."""
from collections import Counter

SITUATIONS = (
    "kyoku", "hora_total", "tsumo", "ron_single", "ron_double", "ron_triple", "chankan_ron", "ron_on_ankan", "rinshan_tsumo",
    "haitei_tsumo", "houtei_ron", "first_turn_win", "tenhou", "chiihou_position", "renhou_position", "double_riichi_declared",
    "double_riichi_win", "ippatsu_win", "abort_kyuushu", "abort_four_winds", "four_winds_broken", "abort_four_riichi", "abort_four_kans",
    "four_kans_one_seat_play_goes_on", "exhaustive_tenpai_0", "exhaustive_tenpai_1", "exhaustive_tenpai_2", "exhaustive_tenpai_3",
    "exhaustive_tenpai_4", "nagashi_mangan_1", "nagashi_mangan_2", "nagashi_mangan_3", "nagashi_mangan_4", "nagashi_lost_to_call", "pao_set_daisangen",
    "pao_set_daisuushi", "pao_tsumo_paid", "pao_ron_split_paid", "pao_ron_from_liable", "win_32000_plus", "kan_dora_at_discard",
    "kan_dora_at_next_draw", "kan_dora_at_ankan", "consecutive_kans", "hanchan_ends_negative", "west_round_kyoku", "honba_3_plus",
    "kyotaku_2_plus",
)

_NAMES = [f"{n}{s}" for s in "mps" for n in range(1, 10)] + ["E", "S", "W", "N", "P", "F", "C"]
_ID = {n: i for i, n in enumerate(_NAMES)}
_ID.update({"5mr": 4, "5pr": 13, "5sr": 22})
_YAOKYUU = frozenset([0, 8, 9, 17, 18, 26, 27, 28, 29, 30, 31, 32, 33])
_KANS = ("daiminkan", "kakan", "ankan")
_CALLS = ("chi", "pon") + _KANS


def tile_id(name):
    """Tile name -> 0..33 (a red five counts as its plain five)."""
    return _ID[name]


def _sets(c, i, need):
    """Can counts c[i:] of one hand be split into exactly `need` more runs and triplets (nothing left over)?"""
    while i < 34 and c[i] == 0:
        i += 1
    if i == 34:
        return need == 0
    if need == 0:
        return False
    if c[i] >= 3:
        c[i] -= 3
        ok = _sets(c, i, need - 1)
        c[i] += 3
        if ok:
            return True
    if i < 27 and i % 9 <= 6 and c[i + 1] and c[i + 2]:
        c[i] -= 1; c[i + 1] -= 1; c[i + 2] -= 1
        ok = _sets(c, i, need - 1)
        c[i] += 1; c[i + 1] += 1; c[i + 2] += 1
        if ok:
            return True
    return False


def is_complete(counts):
    """A 3k+2-tile concealed part (34 counts): k sets and a pair, seven pairs, or thirteen orphans."""
    n = sum(counts)
    if n % 3 != 2:
        return False
    c = list(counts)
    if n == 14:
        if all(x in (0, 2) for x in c):
            return True
        if all(c[t] >= 1 for t in _YAOKYUU) and sum(c[t] for t in _YAOKYUU) == 14:
            return True
    for p in range(34):
        if c[p] >= 2:
            c[p] -= 2
            ok = _sets(c, 0, n // 3)
            c[p] += 2
            if ok:
                return True
    return False


def is_tenpai(counts):
    """A 3k+1-tile concealed part that some 34th of the tile kinds completes (a kind held four times cannot be drawn again)."""
    c = list(counts)
    if sum(c) % 3 != 1:
        return False
    for t in range(34):
        if c[t] < 4:
            c[t] += 1
            ok = is_complete(c)
            c[t] -= 1
            if ok:
                return True
    return False


class _Kyoku:
    def __init__(self, ev):
        self.oya = ev["oya"]
        self.honba = ev["honba"]
        self.kyotaku = ev["kyotaku"]
        self.scores = list(ev["scores"])
        self.hands = [[0] * 34 for _ in range(4)]
        for s in range(4):
            for t in ev["tehais"][s]:
                self.hands[s][tile_id(t)] += 1
        self.draws = 0
        self.n_discards = [0] * 4
        self.all_yaokyuu = [True] * 4      # every discard so far a terminal or an honour
        self.called_on = [False] * 4       # a discard of the seat was taken by chi / pon / daiminkan
        self.any_call = False              # chi / pon / any kan so far (the first go-around is "uninterrupted" without one)
        self.first_discards = []
        self.four_winds_due = False        # the last event was the fourth of four equal first wind discards, nothing called
        self.kans_by = [0] * 4
        self.accepted = [False] * 4
        self.reach_pending = None          # seat whose riichi awaits its discard
        self.double_riichi = [False] * 4
        self.ippatsu = [False] * 4
        self.honour_melds = [set() for _ in range(4)]
        self.pao = [None] * 4
        self.last_draw_rinshan = False
        self.prev = None                   # previous event, `dora` skipped
        self.prev_raw = None               # previous event, `dora` included
        self.after_fourth_kan_discard = False
        self.kan_since_discard = [False] * 4
        self.deltas = [0] * 4
        self.hora_group = []


def census_by_kyoku(events):
    """-> one Counter per kyoku of the log, in order (the last one may be of an unfinished kyoku)."""
    out = []
    k = None
    cnt = None
    for ev in events:
        t = ev["type"]
        if t in ("start_game", "end_game", "none"):
            continue
        if t == "start_kyoku":
            k = _Kyoku(ev)
            cnt = Counter(kyoku=1)
            out.append(cnt)
            if ev["bakaze"] == "W":
                cnt["west_round_kyoku"] += 1
            if ev["honba"] >= 3:
                cnt["honba_3_plus"] += 1
            if ev["kyotaku"] >= 2:
                cnt["kyotaku_2_plus"] += 1
            continue
        if k is None:
            raise ValueError(f"{t} before any start_kyoku")
        if t != "hora" and k.hora_group:
            _close_hora_group(k, cnt)
        if k.four_winds_due:
            # the abort follows the fourth discard at once: no ron on it, no riichi accepted, no draw (board.rs:314-340, :587-600)
            k.four_winds_due = False
            if t != "ryukyoku":
                cnt["mismatch:four_winds_not_aborted"] += 1
        if t == "tsumo":
            a = ev["actor"]
            k.draws += 1
            k.hands[a][tile_id(ev["pai"])] += 1
            k.last_draw_rinshan = k.prev is not None and k.prev["type"] in _KANS
            if k.prev_raw is not None and k.prev_raw["type"] == "dora" and k.last_draw_rinshan:
                if k.prev["type"] != "ankan":
                    cnt["kan_dora_at_next_draw"] += 1
            if k.after_fourth_kan_discard and max(k.kans_by) == 4:
                cnt["four_kans_one_seat_play_goes_on"] += 1
                k.after_fourth_kan_discard = False
        elif t == "dahai":
            a = ev["actor"]
            p = tile_id(ev["pai"])
            k.hands[a][p] -= 1
            if k.prev_raw is not None and k.prev_raw["type"] == "dora":
                cnt["kan_dora_at_discard"] += 1
            if len(k.first_discards) < 4:
                k.first_discards.append(p)
                if len(k.first_discards) == 4 and _three_winds(k):
                    if p == k.first_discards[0]:
                        k.four_winds_due = True
                    else:
                        cnt["four_winds_broken"] += 1
            k.n_discards[a] += 1
            if p not in _YAOKYUU:
                k.all_yaokyuu[a] = False
            k.ippatsu[a] = False
            if k.reach_pending == a:
                k.reach_pending = None
            k.kan_since_discard[a] = False
            if sum(k.kans_by) == 4:
                k.after_fourth_kan_discard = True
        elif t in _CALLS:
            a = ev["actor"]
            if k.after_fourth_kan_discard and max(k.kans_by) == 4:
                cnt["four_kans_one_seat_play_goes_on"] += 1
                k.after_fourth_kan_discard = False
            if len(k.first_discards) == 3 and _three_winds(k):
                cnt["four_winds_broken"] += 1
            for c in ev["consumed"]:
                if t != "kakan":
                    k.hands[a][tile_id(c)] -= 1
            if t == "kakan":
                k.hands[a][tile_id(ev["pai"])] -= 1
            k.any_call = True
            k.ippatsu = [False] * 4
            if t in ("chi", "pon", "daiminkan"):
                k.called_on[ev["target"]] = True
            if t in _KANS:
                if k.kan_since_discard[a]:
                    cnt["consecutive_kans"] += 1
                k.kan_since_discard[a] = True
                k.kans_by[a] += 1
            if t in ("pon", "daiminkan") and tile_id(ev["pai"]) >= 27:
                p = tile_id(ev["pai"])
                k.honour_melds[a].add(p)
                if p >= 31 and k.honour_melds[a] >= {31, 32, 33}:
                    cnt["pao_set_daisangen"] += 1
                    k.pao[a] = ev["target"]
                elif p < 31 and k.honour_melds[a] >= {27, 28, 29, 30}:
                    cnt["pao_set_daisuushi"] += 1
                    k.pao[a] = ev["target"]
        elif t == "dora":
            if k.prev_raw is not None and k.prev_raw["type"] == "ankan":
                cnt["kan_dora_at_ankan"] += 1
        elif t == "reach":
            a = ev["actor"]
            k.reach_pending = a
            if k.n_discards[a] == 0 and not k.any_call:
                cnt["double_riichi_declared"] += 1
                k.double_riichi[a] = True
        elif t == "reach_accepted":
            a = ev["actor"]
            k.accepted[a] = True
            k.ippatsu[a] = True
            k.kyotaku += 1
            k.scores[a] -= 1000
        elif t == "hora":
            k.hora_group.append(ev)
        elif t == "ryukyoku":
            _ryukyoku(k, cnt, ev)
        elif t == "end_kyoku":
            if any(k.scores[s] + k.deltas[s] < 0 for s in range(4)):
                cnt["hanchan_ends_negative"] += 1
        else:
            raise ValueError(f"unknown event type {t!r}")
        if t not in ("dora", "hora"):
            k.prev = ev
        k.prev_raw = ev
    if k is not None and k.hora_group:
        _close_hora_group(k, cnt)
    return out


def _three_winds(k):
    """The first three discards of the kyoku are one and the same wind and nothing was called or declared before or among them
    (to be asked before the event at hand is booked: a call that answers the third discard still finds `any_call` unset)."""
    f = k.first_discards[:3]
    return len(f) == 3 and not k.any_call and f[0] == f[1] == f[2] and 27 <= f[0] <= 30


def census(events):
    """-> Counter of the situations of one game log."""
    total = Counter()
    for c in census_by_kyoku(events):
        total.update(c)
    return total


def _close_hora_group(k, cnt):
    group, k.hora_group = k.hora_group, []
    n = len(group)
    cnt["hora_total"] += n
    first = group[0]
    is_ron = first["actor"] != first["target"]
    before = k.prev  # the event the win answers (dora skipped): a discard, a kakan, an ankan, or the winner's own draw
    if is_ron:
        cnt[("ron_single", "ron_double", "ron_triple")[n - 1]] += 1
        if before["type"] == "kakan":
            cnt["chankan_ron"] += 1
        elif before["type"] == "ankan":
            cnt["ron_on_ankan"] += 1
        elif k.draws == 70:
            cnt["houtei_ron"] += 1
    else:
        cnt["tsumo"] += 1
        if k.last_draw_rinshan:
            cnt["rinshan_tsumo"] += 1
        elif k.draws == 70:
            cnt["haitei_tsumo"] += 1
    kp, hb = k.kyotaku * 1000, k.honba * 300  # riichi sticks and honba go to the first winner in turn order only (board.rs:419-420)
    for ev in group:
        a, tg = ev["actor"], ev["target"]
        d = ev["deltas"]
        for s in range(4):
            k.deltas[s] += d[s]
        if k.n_discards[a] == 0 and not k.any_call:
            cnt["first_turn_win"] += 1
            cnt["renhou_position" if is_ron else "tenhou" if a == k.oya else "chiihou_position"] += 1
        if k.accepted[a]:
            if k.double_riichi[a]:
                cnt["double_riichi_win"] += 1
            if k.ippatsu[a]:
                cnt["ippatsu_win"] += 1
        if d[a] - kp - hb >= 32000:
            cnt["win_32000_plus"] += 1
        pao = k.pao[a]
        if pao is not None:
            # the liable seat pays the whole hand on a tsumo, half of it on a ron from a third seat, and the honba alone in
            # either case (board.rs:407-416, :442-446); nobody else pays anything
            ok = d[pao] < 0 and all(d[s] == 0 for s in range(4) if s not in (a, pao, tg)) and sum(d) == kp
            if not is_ron:
                cnt["pao_tsumo_paid"] += 1
            elif tg == pao:
                cnt["pao_ron_from_liable"] += 1
            else:
                cnt["pao_ron_split_paid"] += 1
                ok = ok and d[tg] < 0 and d[pao] - d[tg] == -hb
            if not ok:
                cnt["mismatch:pao_deltas"] += 1
        kp = hb = 0
    k.kyotaku = 0


def _ryukyoku(k, cnt, ev):
    d = ev["deltas"]
    for s in range(4):
        k.deltas[s] += d[s]
    prev = k.prev["type"]
    kans = sum(k.kans_by)
    if sum(k.accepted) == 4:
        cnt["abort_four_riichi"] += 1
        kind = "abort"
    elif kans == 4 and max(k.kans_by) < 4 and prev == "dahai":
        cnt["abort_four_kans"] += 1
        kind = "abort"
    elif prev == "tsumo" and k.draws < 70:
        a = k.prev["actor"]
        kind = "abort"
        cnt["abort_kyuushu"] += 1
        if k.any_call or k.n_discards[a] or sum(k.hands[a][t] > 0 for t in _YAOKYUU) < 9:
            cnt["mismatch:kyuushu"] += 1
    elif (prev == "dahai" and sum(k.n_discards) == 4 and not k.any_call and len(set(k.first_discards)) == 1
          and 27 <= k.first_discards[0] <= 30):
        cnt["abort_four_winds"] += 1
        kind = "abort"
    elif prev == "dahai" and k.draws == 70:
        kind = "exhaustive"
    else:
        cnt["mismatch:unclassified_ryukyoku"] += 1
        return
    if kind == "abort":
        if any(d):
            cnt["mismatch:abort_deltas"] += 1
        return
    nagashi = [s for s in range(4) if k.all_yaokyuu[s] and not k.called_on[s]]
    if any(k.all_yaokyuu[s] and k.called_on[s] for s in range(4)):
        cnt["nagashi_lost_to_call"] += 1  # (such a seat is in no `nagashi` below: the payments wanted of it are those by tenpai)
    want = [0] * 4
    if nagashi:
        cnt[f"nagashi_mangan_{len(nagashi)}"] += 1
        for i in nagashi:
            for s in range(4):
                if i == k.oya:
                    want[s] += 12000 if s == i else -4000
                else:
                    want[s] += 8000 if s == i else -4000 if s == k.oya else -2000
    tenpai = [s for s in range(4) if is_tenpai(k.hands[s])]
    if not nagashi:
        cnt[f"exhaustive_tenpai_{len(tenpai)}"] += 1
        plus, minus = {1: (3000, -1000), 2: (1500, -1500), 3: (1000, -3000)}.get(len(tenpai), (0, 0))
        want = [plus if s in tenpai else minus for s in range(4)]
    if want != list(d):
        cnt["mismatch:exhaustive_deltas"] += 1
