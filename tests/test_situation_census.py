"""tests/situation_census.py on hand-written event lists of a few events each (the oracle is not the census's only check), and on
the golden game of tests/golden/example_game.jsonl.  (tests/golden/state_scenarios.json holds one seat's view of a kyoku, without the
other hands and without deltas: not a game log the census can read.)"""
import json
import os

import situation_census as C

ANY = ["1m", "2m", "3m", "4p", "5p", "6p", "7s", "8s", "9s", "E", "E", "S", "P"]          # 13 tiles, not tenpai
TENPAI = ["1m", "2m", "3m", "4p", "5p", "6p", "7s", "8s", "9s", "E", "E", "S", "S"]       # waits E / S
KYUUSHU = ["1m", "9m", "1p", "9p", "1s", "9s", "E", "S", "W", "2m", "3m", "4m", "5m"]


def sk(oya=0, honba=0, kyotaku=0, bakaze="E", tehais=None, scores=(25000,) * 4):
    return {"type": "start_kyoku", "bakaze": bakaze, "dora_marker": "1s", "kyoku": oya + 1, "honba": honba, "kyotaku": kyotaku,
            "oya": oya, "scores": list(scores), "tehais": tehais or [ANY] * 4}


def ts(a, p="9p"):
    return {"type": "tsumo", "actor": a, "pai": p}


def da(a, p="9p"):
    return {"type": "dahai", "actor": a, "pai": p, "tsumogiri": False}


def hora(a, t, deltas):
    return {"type": "hora", "actor": a, "target": t, "deltas": deltas, "ura_markers": []}


def ryu(deltas=(0, 0, 0, 0)):
    return {"type": "ryukyoku", "deltas": list(deltas)}


def pon(a, t, p):
    return {"type": "pon", "actor": a, "target": t, "pai": p, "consumed": [p, p]}


def kan(kind, a, p, t=None):
    if kind == "ankan":
        return {"type": "ankan", "actor": a, "consumed": [p] * 4}
    if kind == "kakan":
        return {"type": "kakan", "actor": a, "pai": p, "consumed": [p] * 3}
    return {"type": "daiminkan", "actor": a, "target": t, "pai": p, "consumed": [p] * 3}


DORA = {"type": "dora", "dora_marker": "2s"}
END = {"type": "end_kyoku"}


def reach(a, p="9p"):
    return [{"type": "reach", "actor": a}, da(a, p), {"type": "reach_accepted", "actor": a}]


def has(events, **want):
    got = C.census(events)
    assert not [k for k in got if k.startswith("mismatch:")], got
    for k, v in want.items():
        assert got[k] == v, (k, got)
    return got


def test_single_double_triple_ron():
    base = [sk(), ts(0), da(0)]
    has(base + [hora(1, 0, [-1000, 1000, 0, 0]), END], ron_single=1, hora_total=1, ron_double=0)
    has(base + [hora(1, 0, [-1000, 1000, 0, 0]), hora(3, 0, [-2000, 0, 0, 2000]), END], ron_double=1, hora_total=2, ron_single=0)
    has(base + [hora(1, 0, [-1000, 1000, 0, 0]), hora(2, 0, [-1000, 0, 1000, 0]), hora(3, 0, [-2000, 0, 0, 2000]), END],
        ron_triple=1, hora_total=3)


def test_chankan_and_ron_on_ankan_and_rinshan():
    has([sk(), ts(0), da(0, "P"), pon(1, 0, "P"), da(1), ts(2), da(2), ts(3), da(3), ts(0), da(0), ts(1, "P"), kan("kakan", 1, "P"),
         hora(2, 1, [0, -8000, 8000, 0]), END], chankan_ron=1, ron_single=1, ron_on_ankan=0)
    has([sk(), ts(0, "1m"), kan("ankan", 0, "1m"), DORA, hora(2, 0, [-32000, 0, 32000, 0]), END], ron_on_ankan=1, chankan_ron=0,
        kan_dora_at_ankan=1, win_32000_plus=1)
    for k in (kan("ankan", 0, "1m"), kan("kakan", 0, "1m")):
        ev = [sk(), ts(0, "1m"), k] + ([DORA] if k["type"] == "ankan" else []) + [ts(0), hora(0, 0, [6000, -2000, -2000, -2000]), END]
        has(ev, rinshan_tsumo=1, tsumo=1, haitei_tsumo=0)
    has([sk(), ts(0), da(0), ts(1), hora(1, 1, [-2000, 4000, -1000, -1000]), END], rinshan_tsumo=0, tsumo=1)


def _seventy_draws(last_discard=True):
    ev = [sk(tehais=[TENPAI, ANY, ANY, ANY])]
    for i in range(70):
        ev += [ts(i % 4, "5m")] + ([da(i % 4, "5m")] if i < 69 or last_discard else [])
    return ev


def test_haitei_and_houtei():
    has(_seventy_draws(False) + [hora(1, 1, [-2000, 4000, -1000, -1000]), END], haitei_tsumo=1)
    has(_seventy_draws() + [hora(2, 1, [0, -1000, 1000, 0]), END], houtei_ron=1)


def test_first_go_around_positions_and_double_riichi():
    has([sk(), ts(0), hora(0, 0, [48000, -16000, -16000, -16000]), END], tenhou=1, first_turn_win=1, win_32000_plus=1)
    has([sk(), ts(0), da(0), ts(1), hora(1, 1, [-16000, 32000, -8000, -8000]), END], chiihou_position=1, first_turn_win=1)
    has([sk(), ts(0), da(0), hora(2, 0, [-1000, 0, 1000, 0]), END], renhou_position=1, first_turn_win=1)
    # a call interrupts the go-around; a seat that has discarded is past it
    has([sk(), ts(0), da(0, "P"), pon(2, 0, "P"), da(2), hora(3, 2, [0, 0, -1000, 1000]), END], first_turn_win=0)
    has([sk(), ts(0), da(0), ts(1), da(1), ts(2), da(2), ts(3), da(3), ts(0), hora(0, 0, [3000, -1000, -1000, -1000]), END],
        first_turn_win=0)
    ev = [sk(), ts(0)] + reach(0) + [ts(1), da(1, "E"), hora(0, 1, [2000, -1000, 0, 0]), END]
    has(ev, double_riichi_declared=1, double_riichi_win=1, ippatsu_win=1)
    ev = [sk(), ts(0), da(0), ts(1), da(1), ts(2), da(2), ts(3), da(3), ts(0)] + reach(0) + [ts(1), da(1), hora(0, 1, [2000, -1000, 0, 0]), END]
    has(ev, double_riichi_declared=0, double_riichi_win=0, ippatsu_win=1)


def test_ippatsu_ends_with_a_call_or_the_next_discard():
    head = [sk(), ts(0), da(0), ts(1), da(1), ts(2), da(2), ts(3), da(3), ts(0)] + reach(0)
    has(head + [ts(1), da(1, "P"), pon(3, 1, "P"), da(3), hora(0, 3, [2000, 0, 0, -1000]), END], ippatsu_win=0, ron_single=1)
    has(head + [ts(1), da(1), ts(2), da(2), ts(3), da(3), ts(0), da(0), ts(1), da(1), hora(0, 1, [2000, -1000, 0, 0]), END], ippatsu_win=0)
    has(head + [ts(1), da(1), ts(2), da(2), ts(3), da(3), ts(0), hora(0, 0, [4000, -1000, -1000, -1000]), END], ippatsu_win=1)


def test_abortive_draws_by_kind():
    has([sk(tehais=[KYUUSHU, ANY, ANY, ANY]), ts(0, "N"), ryu(), END], abort_kyuushu=1)
    has([sk(), ts(0), da(0, "W"), ts(1), da(1, "W"), ts(2), da(2, "W"), ts(3), da(3, "W"), ryu(), END], abort_four_winds=1)
    ev = [sk()]
    for s in range(4):
        ev += [ts(s)] + reach(s)[:2] + ([{"type": "reach_accepted", "actor": s}] if s < 3 else [])
    # the fourth riichi is accepted when nobody rons its discard, together with the next draw; the abort follows that draw
    has(ev + [{"type": "reach_accepted", "actor": 3}, ts(0), ryu(), END], abort_four_riichi=1, abort_kyuushu=0)
    ev = [sk()]
    for s in range(4):
        ev += [ts(s, "1m"), kan("ankan", s, "1m"), DORA, ts(s), da(s)] if s < 3 else [ts(s, "1m"), kan("ankan", s, "1m"), DORA, ts(s), da(s), ryu(), END]
    has(ev, abort_four_kans=1, kan_dora_at_ankan=4, four_kans_one_seat_play_goes_on=0)


def test_four_kans_in_one_hand_do_not_abort():
    ev = [sk(), ts(0, "1m")]
    for p in ("1m", "2m", "3m", "4m"):
        ev += [kan("ankan", 0, p), DORA, ts(0, p)]
    has(ev + [da(0), ts(1), da(1)], four_kans_one_seat_play_goes_on=1, abort_four_kans=0, consecutive_kans=3)


def test_exhaustive_draw_by_tenpai_seats_tells_none_from_all():
    def run(n_tenpai, deltas):
        ev = [sk(tehais=[TENPAI] * n_tenpai + [ANY] * (4 - n_tenpai))]
        for i in range(70):
            ev += [ts(i % 4, "5m"), da(i % 4, "5m")]
        return ev + [ryu(deltas), END]

    has(run(0, [0, 0, 0, 0]), exhaustive_tenpai_0=1, exhaustive_tenpai_4=0)
    has(run(4, [0, 0, 0, 0]), exhaustive_tenpai_4=1, exhaustive_tenpai_0=0)
    has(run(1, [3000, -1000, -1000, -1000]), exhaustive_tenpai_1=1)
    has(run(2, [1500, 1500, -1500, -1500]), exhaustive_tenpai_2=1)
    has(run(3, [1000, 1000, 1000, -3000]), exhaustive_tenpai_3=1)
    assert C.census(run(1, [1500, 1500, -1500, -1500]))["mismatch:exhaustive_deltas"] == 1


def _nagashi_run(yao_seats, deltas):
    ev = [sk(oya=1)]
    for i in range(70):
        s = (1 + i) % 4
        p = "9p" if s in yao_seats else "5m"
        ev += [ts(s, p), da(s, p)]
    return ev + [ryu(deltas), END]


def test_nagashi_mangan_by_number_of_seats():
    run = _nagashi_run
    has(run({1}, [-4000, 12000, -4000, -4000]), nagashi_mangan_1=1)
    has(run({2}, [-2000, -4000, 8000, -2000]), nagashi_mangan_1=1)
    has(run({0, 2}, [6000, -8000, 6000, -4000]), nagashi_mangan_2=1, nagashi_mangan_1=0)
    # a discard that somebody called ends the seat's nagashi: the draw is paid by tenpai again
    ev = run({2}, [0, 0, 0, 0])
    at = next(i for i, e in enumerate(ev) if e["type"] == "dahai" and e["actor"] == 2)
    ev[at - 1], ev[at] = ts(2, "E"), da(2, "E")
    ev[at + 1:at + 1] = [pon(0, 2, "E"), da(0, "1m")]
    has(ev, nagashi_mangan_1=0, exhaustive_tenpai_0=1)


def test_four_winds_aborted_broken_and_not_aborted():
    three = [sk(), ts(0), da(0, "W"), ts(1), da(1, "W"), ts(2), da(2, "W"), ts(3)]
    has(three + [da(3, "W"), ryu(), END], abort_four_winds=1, four_winds_broken=0, abort_kyuushu=0)
    # the fourth discard differs (another wind included), or a call or a concealed kan comes first: play goes on
    has(three + [da(3, "N"), ts(0), da(0)], four_winds_broken=1, abort_four_winds=0)
    has(three + [da(3, "1m"), ts(0), da(0)], four_winds_broken=1)
    has(three[:-1] + [pon(0, 2, "W"), da(0), ts(1), da(1)], four_winds_broken=1)
    has(three[:-1] + [ts(3, "1m"), kan("ankan", 3, "1m"), DORA, ts(3), da(3, "W"), ts(0), da(0)], four_winds_broken=1, abort_four_winds=0)
    # not three of a kind, not winds, or a call before the third: nothing to break
    has([sk(), ts(0), da(0, "W"), ts(1), da(1, "N"), ts(2), da(2, "W"), ts(3), da(3, "W"), ts(0), da(0)], four_winds_broken=0)
    has([sk(), ts(0), da(0, "P"), ts(1), da(1, "P"), ts(2), da(2, "P"), ts(3), da(3, "P"), ts(0), da(0)], four_winds_broken=0)
    has([sk(), ts(0), da(0, "W"), ts(1), da(1, "W"), pon(3, 1, "W"), da(3, "W"), ts(0), da(0, "W"), ts(1), da(1)], four_winds_broken=0)
    # four equal winds and the game goes on, by a draw, a ron or an accepted riichi: the log contradicts the rule
    for after in ([ts(0), da(0)], [hora(0, 3, [1000, 0, 0, -1000]), END], [{"type": "reach_accepted", "actor": 3}, ts(0)]):
        got = C.census(three + [da(3, "W")] + after)
        assert got["mismatch:four_winds_not_aborted"] == 1 and got["abort_four_winds"] == 0, got
    assert not [k for k in C.census(three + [da(3, "W")]) if k.startswith("mismatch:")]  # (a log that stops there says nothing)


def test_the_two_early_aborts_are_told_apart_by_the_events_alone():
    # a `ryukyoku` carries deltas and nothing else: after a draw it is the nine terminals, after the fourth wind the four winds
    kyuushu = [sk(tehais=[ANY, KYUUSHU, ANY, ANY]), ts(0), da(0, "W"), ts(1, "N"), ryu(), END]
    has(kyuushu, abort_kyuushu=1, abort_four_winds=0)
    winds = [sk(tehais=[KYUUSHU] * 4), ts(0), da(0, "E"), ts(1), da(1, "E"), ts(2), da(2, "E"), ts(3), da(3, "E"), ryu(), END]
    has(winds, abort_four_winds=1, abort_kyuushu=0)
    # nine terminals declared by a hand that does not hold them, or after a call
    assert C.census([sk(), ts(0, "N"), ryu(), END])["mismatch:kyuushu"] == 1
    assert C.census([sk(tehais=[ANY, ANY, KYUUSHU, ANY]), ts(0), da(0, "P"), pon(1, 0, "P"), da(1), ts(2, "N"), ryu(), END])["mismatch:kyuushu"] == 1


def test_nagashi_lost_to_a_call_is_paid_by_tenpai():
    def run(deltas, tehais=None):
        ev = [sk(oya=1, tehais=tehais)]
        for i in range(70):
            s = (1 + i) % 4
            p = "9p" if s == 2 else "5m"
            ev += [ts(s, p), da(s, p)]
        at = next(i for i, e in enumerate(ev) if e["type"] == "dahai" and e["actor"] == 2)
        ev[at - 1], ev[at] = ts(2, "E"), da(2, "E")
        ev[at + 1:at + 1] = [pon(0, 2, "E"), da(0, "1m")]
        return ev + [ryu(deltas), END]

    has(run([0, 0, 0, 0]), nagashi_lost_to_call=1, nagashi_mangan_1=0, exhaustive_tenpai_0=1)
    has(run([-1000, -1000, 3000, -1000], tehais=[ANY, ANY, TENPAI, ANY]), nagashi_lost_to_call=1, exhaustive_tenpai_1=1)
    # the mangan paid all the same
    assert C.census(run([-2000, -4000, 8000, -2000]))["mismatch:exhaustive_deltas"] == 1
    # terminals only, nothing called: a nagashi mangan, nothing lost
    has(_nagashi_run({2}, [-2000, -4000, 8000, -2000]), nagashi_mangan_1=1, nagashi_lost_to_call=0)


def _daisangen(last="pon"):
    ev = [sk(oya=0, honba=1, kyotaku=1), ts(0), da(0, "P"), pon(2, 0, "P"), da(2), ts(3), da(3, "F"), pon(2, 3, "F"), da(2), ts(3), da(3)]
    ev += [ts(0), da(0), ts(1), da(1, "C")]
    return ev + [pon(2, 1, "C") if last == "pon" else kan("daiminkan", 2, "C", 1), da(2)]


def test_pao_liability_and_who_pays():
    has(_daisangen(), pao_set_daisangen=1, pao_set_daisuushi=0)
    has(_daisangen("daiminkan"), pao_set_daisangen=1)
    # tsumo: seat 1 pays all of it and the honba; ron from seat 3: half each, seat 1 carries the honba
    has(_daisangen() + [ts(3), da(3), ts(0), da(0), ts(1), da(1), ts(2), hora(2, 2, [0, -32300, 33300, 0]), END],
        pao_tsumo_paid=1, win_32000_plus=1)
    has(_daisangen() + [ts(3), da(3), hora(2, 3, [0, -16300, 33300, -16000]), END], pao_ron_split_paid=1, win_32000_plus=1)
    has(_daisangen() + [ts(3), da(3), ts(0), da(0), ts(1), da(1), hora(2, 1, [0, -32300, 33300, 0]), END], pao_ron_from_liable=1,
        pao_ron_split_paid=0)
    wrong = C.census(_daisangen() + [ts(3), da(3), hora(2, 3, [0, -32300, 33300, 0]), END])
    assert wrong["mismatch:pao_deltas"] == 1
    wrong = C.census(_daisangen() + [ts(3), da(3), ts(0), da(0), ts(1), da(1), ts(2), hora(2, 2, [-16300, -8000, 33300, -8000]), END])
    assert wrong["mismatch:pao_deltas"] == 1
    ev = [sk()]
    for k, w in enumerate("ESWN"):
        ev += [ts(0), da(0, w), pon(1, 0, w), da(1)] if k < 3 else [ts(0), da(0), ts(3), da(3, w), pon(1, 3, w), da(1)]
    has(ev, pao_set_daisuushi=1, pao_set_daisangen=0)


def test_kan_dora_timings():
    has([sk(), ts(0), da(0, "P"), kan("daiminkan", 1, "P", 0), ts(1), DORA, da(1)], kan_dora_at_discard=1, kan_dora_at_next_draw=0)
    has([sk(), ts(0), da(0, "P"), kan("daiminkan", 1, "P", 0), ts(1, "1m"), kan("kakan", 1, "1m"), DORA, ts(1), DORA, da(1)],
        kan_dora_at_next_draw=1, kan_dora_at_discard=1, consecutive_kans=1)


def test_kyoku_start_flags_and_negative_end():
    has([sk(bakaze="W", honba=3, kyotaku=2)], west_round_kyoku=1, honba_3_plus=1, kyotaku_2_plus=1, kyoku=1)
    has([sk(bakaze="S", honba=2, kyotaku=1)], west_round_kyoku=0, honba_3_plus=0, kyotaku_2_plus=0)
    has([sk(scores=(1000, 33000, 33000, 33000)), ts(0), da(0), hora(1, 0, [-2000, 2000, 0, 0]), END], hanchan_ends_negative=1)
    has([sk(scores=(2000, 33000, 32000, 33000)), ts(0), da(0), hora(1, 0, [-2000, 2000, 0, 0]), END], hanchan_ends_negative=0)


def test_tenpai_reader():
    from oracle_lib import hand

    assert C.is_tenpai(hand("123m456p789s1122z")) and not C.is_tenpai(hand("123m456p789s1123z"))
    assert C.is_tenpai(hand("1133557799m1133p"[:-1] + "p")[:34]) is False  # 14 tiles: not a 3k+1 hand
    assert C.is_tenpai(hand("113355779m1133p"))          # seven pairs
    assert C.is_tenpai(hand("19m19p19s1234567z"))        # thirteen orphans, thirteen waits
    assert C.is_tenpai(hand("2m")) and C.is_tenpai(hand("2345m")) and not C.is_tenpai(hand("1479m"))


def test_golden_example_game():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example_game.jsonl")
    with open(path) as f:
        ev = [json.loads(l) for l in f if l.strip()]
    # three kyoku, three single rons (one of them ippatsu), and the third leaves a seat below zero
    has(ev, kyoku=3, hora_total=3, ron_single=3, ippatsu_win=1, hanchan_ends_negative=1, tsumo=0)
