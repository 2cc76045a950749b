"""Shared by tests/test_stat_device_emu.py (host emulation of the device code) and tests/test_gpu_stat.py (the real library): log
sources, the host reading every case is compared with -- `Stat.from_game(decode_events(words), seat)` -- and the cases that run
on both.  All values are integers: every comparison is exact."""
import numpy as np

import situation_fixture as F
import steering

from mortal_amd import mjai_log as ML
from mortal_amd.stat import STAT_FIELDS, Stat, stat_logs

NF = len(STAT_FIELDS)
FIXTURE_GROUPS = (("everybody_rons", "rand08"), ("terminal_discards", "rand08"))
_cache = {}


def fixture_logs(oracle):
    """The 44 logs of the two steering groups as packed words (the oracle plays them in about a second; cached per process).
    The terminal_discards games never end: they stop at the group's last stop cycle, in the middle of a kyoku."""
    if "logs" not in _cache:
        logs = []
        for group in FIXTURE_GROUPS:
            tables, _ = F.groups()[group]
            arena, _ = steering.play_oracle(oracle, [(n, k) for n, k, _ in tables], group[0], deal_algo=F.ALGO[group[1]],
                                            max_cycles=max(stop for _, _, stop in tables))
            logs += [ML.encode_events(arena.log(g)) for g in range(len(tables))]
        _cache["logs"] = logs
        _cache["want"] = expected(logs)
    return _cache["logs"], _cache["want"]


def expected(words_list):
    """int64 [n, 4, 44]: the host reading of every (log, seat); an empty log is a row of zeros."""
    out = np.zeros((len(words_list), 4, NF), dtype=np.int64)
    for i, w in enumerate(words_list):
        if len(w):
            ev = ML.decode_events(w)
            for s in range(4):
                out[i, s] = Stat.from_game(ev, s).counters()
    return out


def totals_of(rows, seats, groups):
    """[2, 44]: the selected seats of `rows` summed per group bit."""
    tot = np.zeros((2, NF), dtype=np.int64)
    for i in range(rows.shape[0]):
        for s in range(4):
            if (int(seats[i]) >> s) & 1:
                tot[(int(groups[i]) >> s) & 1] += rows[i, s]
    return tot


def check(words_list, lib, seats=None, groups=None, want=None):
    """stat_logs on `lib` against the host reading: per seat and in total."""
    n = len(words_list)
    want = expected(words_list) if want is None else want
    totals, rows, counts = stat_logs(words_list, seats=seats, groups=groups, per_seat=True, lib=lib)
    sm = np.full(n, 15, dtype=np.uint8) if seats is None else np.asarray(seats, dtype=np.uint8)
    gm = np.zeros(n, dtype=np.uint8) if groups is None else np.asarray(groups, dtype=np.uint8)
    sel = np.array([[(int(sm[i]) >> s) & 1 for s in range(4)] for i in range(n)], dtype=np.int64)
    bad = np.argwhere(rows != want * sel[:, :, None])
    assert bad.size == 0, [(int(i), int(s), STAT_FIELDS[f], int(rows[i, s, f]), int(want[i, s, f])) for i, s, f in bad[:8]]
    got = np.array([t.counters() for t in totals], dtype=np.int64)
    assert (got == totals_of(want, sm, gm)).all()
    n_empty = sum(1 for w in words_list if len(w) == 0)
    assert counts == dict(reduced=n - n_empty, skipped=n_empty, malformed=0), counts
    totals2, none, counts2 = stat_logs(words_list, seats=seats, groups=groups, lib=lib)  # (the kernel without the per-seat rows)
    assert none is None and counts2 == counts and [t.counters() for t in totals2] == [t.counters() for t in totals]
    return rows, totals


def check_fixture_logs(oracle, lib):
    """(a) the 44 fixture logs; the coverage the case relies on is asserted, so a stale fixture cannot hollow it out."""
    logs, want = fixture_logs(oracle)
    assert len(logs) == 44 and max(len(w) for w in logs) > 20 * 64  # a log spans many 64-word reads
    per_field = np.abs(want).sum(axis=(0, 1))
    assert (per_field > 0).all(), [STAT_FIELDS[f] for f in np.flatnonzero(per_field == 0)]
    tot = dict(zip(STAT_FIELDS, want.sum(axis=(0, 1))))
    assert tot["yakuman"] > 0 and tot["nagashi_mangan"] > 0 and tot["tobi"] > 0 and tot["chasing_riichi"] > 0 and tot["fuuro_houjuu"] > 0
    ends = [ML.decode_events(w)[-1]["type"] for w in logs]
    assert any(e != "end_kyoku" for e in ends) and any(e == "end_kyoku" for e in ends)  # prefixes that stop in mid-kyoku, and whole kyoku
    check(logs, lib, want=want)


def check_masks_and_groups(oracle, lib):
    """(b) seat masks 0b0001 / 0b1010 / 0 and a group byte per log."""
    logs, want = fixture_logs(oracle)
    n = len(logs)
    seats = np.array([(0b0001, 0b1010, 0)[i % 3] for i in range(n)], dtype=np.uint8)
    groups = np.array([(i * 7 + 3) & 15 for i in range(n)], dtype=np.uint8)
    _, totals = check(logs, lib, seats=seats, groups=groups, want=want)
    assert totals[0].game > 0 and totals[1].game > 0 and totals[0].game + totals[1].game == sum(bin(int(m)).count("1") for m in seats)
    check(logs, lib, groups=groups, want=want)
    check(logs, lib, seats=seats, want=want)


# ---- (c) one short synthetic game, shifted through every position of a 64-word read
_HAND = ["1m", "2m", "3m", "4m", "5m", "6m", "7m", "8m", "9m", "1p", "2p", "3p", "4p"]
TAG_WORD = (1 << 63) | 0x1234_5678_9ABC_DE01  # reads as a start_kyoku header with the wall bit: a payload word may look like any header


def synthetic_events(k, lead):
    """Two kyoku: riichi, a chasing riichi, a pon, a ron off the caller (seat 3, whose turn count grows with k) with an ura
    marker; then a chi, a daiminkan, a riichi and a ryukyoku.  `lead` (0 / 1) tsumo events in front of the first start_kyoku
    and k tsumo / dahai pairs of seat 3 behind it shift every later word, one word at a time over the (k, lead) pairs."""
    sk = dict(type="start_kyoku", bakaze="E", dora_marker="1s", kyoku=1, honba=0, kyotaku=0, oya=0, scores=[25000] * 4,
              tehais=[_HAND] * 4)
    ev = [dict(type="tsumo", actor=2, pai="E")] * lead + [sk]
    for _ in range(k):
        ev += [dict(type="tsumo", actor=3, pai="N"), dict(type="dahai", actor=3, pai="N", tsumogiri=True)]
    ev += [
        dict(type="tsumo", actor=0, pai="5s"), dict(type="reach", actor=0), dict(type="dahai", actor=0, pai="5s", tsumogiri=True),
        dict(type="reach_accepted", actor=0),
        dict(type="tsumo", actor=1, pai="6s"), dict(type="reach", actor=1), dict(type="dahai", actor=1, pai="6s", tsumogiri=True),
        dict(type="reach_accepted", actor=1),
        dict(type="pon", actor=3, target=1, pai="6s", consumed=["6s", "6s"]), dict(type="dahai", actor=3, pai="C", tsumogiri=False),
        dict(type="hora", actor=1, target=3, deltas=[0, 14000, 0, -12000], ura_markers=["3p"]),
        dict(type="end_kyoku"),
        dict(sk, kyoku=2, honba=0, oya=1, scores=[24000, 38000, 25000, 13000]),
        dict(type="tsumo", actor=1, pai="9s"), dict(type="dahai", actor=1, pai="9s", tsumogiri=True),
        dict(type="chi", actor=2, target=1, pai="9s", consumed=["7s", "8s"]), dict(type="dahai", actor=2, pai="P", tsumogiri=False),
        dict(type="daiminkan", actor=0, target=2, pai="P", consumed=["P", "P", "P"]), dict(type="tsumo", actor=0, pai="1s"),
        dict(type="dora", dora_marker="2s"), dict(type="dahai", actor=0, pai="1s", tsumogiri=True),
        dict(type="tsumo", actor=1, pai="F"), dict(type="reach", actor=1), dict(type="dahai", actor=1, pai="F", tsumogiri=True),
        dict(type="reach_accepted", actor=1),
        dict(type="ryukyoku", deltas=[-3000, -3000, 8000, -2000]),
        dict(type="end_kyoku"),
    ]
    return ev


def synthetic_words(k, lead, tagged):
    """The events as packed words; `tagged`: every reaction header (discards, calls, riichi, hora) carries LG_TAG_BIT and one
    tag word, as in the logs a pool writes for its agents' decisions."""
    out = []
    for e in synthetic_events(k, lead):
        w = [int(x) for x in ML.encode_events([e])]
        if tagged and e["type"] in ("dahai", "chi", "pon", "daiminkan", "reach", "hora"):
            w = [w[0] | (1 << 43), TAG_WORD] + w[1:]
        out += w
    return np.array(out, dtype=np.uint64)


def check_alignment_sweep(lib):
    for tagged in (False, True):
        logs = [synthetic_words(k, lead, tagged) for k in range(64) for lead in (0, 1)]
        want = expected(logs)
        assert (want[:, :, STAT_FIELDS.index("game")] == 1).all() and (want[0] == want[-1]).sum() < want[0].size  # (seat 3's houjuu_jun grows with k)
        for f in ("riichi", "chasing_riichi", "riichi_got_chased", "riichi_agari", "fuuro_houjuu", "fuuro", "nagashi_mangan",
                  "riichi_ryukyoku"):
            assert want[0, :, STAT_FIELDS.index(f)].any(), f
        check(logs, lib, want=want)


def check_alignment_sweep_grp(lib):
    """The same 2 x 128 synthetic logs through grp_logs against the host `Grp.load_events`: the shared walk's window restart
    (an event at window index 60 / 61 among them) under its second consumer."""
    from mortal_amd.dataset import Grp, grp_logs

    for tagged in (False, True):
        pairs = [(k, lead) for k in range(64) for lead in (0, 1)]
        logs = [synthetic_words(k, lead, tagged) for k, lead in pairs]
        grps, n_kyoku, counts = grp_logs(logs, max_kyoku=2, lib=lib)
        assert counts == dict(reduced=len(logs), skipped=0, malformed=0), counts
        assert (n_kyoku == 2).all()
        for g, (k, lead) in zip(grps, pairs):
            want = Grp.load_events(ML.decode_events(synthetic_words(k, lead, tagged)))
            assert want.feature.shape == (2, 7) and sum(want.final_scores) == 100_000
            assert (g.feature.view(np.uint64) == want.feature.view(np.uint64)).all(), (tagged, k, lead)
            assert g.rank_by_player == want.rank_by_player and g.final_scores == want.final_scores, (tagged, k, lead)


# ---- (d) bad and empty input: ten logs, read by all three routes
def check_bad_and_empty_input(lib):
    """A log cut inside a hora payload, one cut inside a start_kyoku payload and headers of type 15 / 0 are counted as malformed
    and contribute nothing; an empty log is skipped; their neighbours are reduced as if they stood alone.  No route reads beyond a
    log's length, so this is a contained error path.  Stat (stat_logs), Grp (grp_logs / Grp.from_packed) and the augmenting copy
    (mjai_log.augment_logs / mj_augment_logs) agree on the ten: logs 0, 2, 4, 6, 9 accepted, log 5 skipped, logs 1, 3, 7, 8
    malformed -- counts 5 / 1 / 4.  Grp's two extra rules: every accepted log has two start_kyoku, so none falls under "no
    start_kyoku", and with max_kyoku = 1 the five become malformed as well (0 / 1 / 9)."""
    import pytest

    from mortal_amd.dataset import Grp, grp_logs

    good = [synthetic_words(k, 0, tagged) for k, tagged in ((0, False), (31, True), (5, False), (62, True), (17, False))]
    base = synthetic_words(29, 1, False)
    hora = next(i for i, w in enumerate(base) if int(w) & 15 == ML.LG_HORA and i > 60)
    assert ML.decode_events(base[:hora])[-1]["type"] == "dahai"  # (a header found by walking, not a payload word that looks like one)
    cut_hora = base[:hora + 2]
    cut_start = base[:6]
    type15 = np.concatenate([base[:hora], np.array([15], dtype=np.uint64), base[hora:]])
    type0 = np.concatenate([base, np.array([0], dtype=np.uint64)])
    empty = np.zeros(0, dtype=np.uint64)
    logs = [good[0], cut_hora, good[1], type15, good[2], empty, good[3], type0, cut_start, good[4]]
    for w in (cut_hora, cut_start, type15, type0):
        with pytest.raises((IndexError, ValueError)):
            ML.decode_events(w)
    is_good, is_bad = [0, 2, 4, 6, 9], [1, 3, 7, 8]
    # Stat
    want = np.zeros((len(logs), 4, NF), dtype=np.int64)
    want[is_good] = expected(good)
    groups = np.array([1, 15, 2, 15, 4, 15, 8, 15, 15, 0], dtype=np.uint8)
    totals, rows, counts = stat_logs(logs, groups=groups, per_seat=True, lib=lib)
    assert counts == dict(reduced=5, skipped=1, malformed=4), counts
    assert (rows == want).all()
    assert (np.array([t.counters() for t in totals]) == totals_of(want, np.full(len(logs), 15), groups)).all()
    assert totals[0].game == 16 and totals[1].game == 4
    # Grp
    grps, n_kyoku, counts = grp_logs(logs, lib=lib)
    assert counts == dict(reduced=5, skipped=1, malformed=4), counts
    assert n_kyoku.tolist() == [2, -1, 2, -1, 2, 0, 2, -1, -1, 2]
    for i, g in enumerate(grps):
        if i in is_good:
            w = Grp.load_events(ML.decode_events(logs[i]))
            assert (g.feature.view(np.uint64) == w.feature.view(np.uint64)).all() and g.rank_by_player == w.rank_by_player \
                and g.final_scores == w.final_scores, i
        else:
            assert g is None, i
    with pytest.raises(ValueError, match="log 1"):
        Grp.from_packed(logs, lib=lib)
    grps, n_kyoku, counts = grp_logs(logs, max_kyoku=1, lib=lib)
    assert counts == dict(reduced=0, skipped=1, malformed=9) and grps == [None] * 10
    assert n_kyoku.tolist() == [-1, -1, -1, -1, -1, 0, -1, -1, -1, -1]
    # the augmenting copy: an accepted log comes back augmented (as it does alone), the others as they came
    with pytest.raises(ValueError, match="log 1 is malformed"):
        ML.augment_logs(logs, lib=lib)
    alone = ML.augment_logs(good, lib=lib)
    off = np.zeros(len(logs) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in logs])
    words = np.ascontiguousarray(np.concatenate(logs), dtype=np.uint64)
    out = np.full_like(words, 0x5A5A)
    counts = np.full(3, 7, dtype=np.int64)
    stream = None
    if lib is None:
        import ctypes

        import torch

        from mortal_amd._lib import lib
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mj_augment_logs(words.ctypes.data, off.ctypes.data, len(logs), out.ctypes.data, counts.ctypes.data, stream) == 0
    assert counts.tolist() == [5, 1, 4]
    for i in range(len(logs)):
        got = out[int(off[i]):int(off[i + 1])]
        if i in is_good:
            assert (got == alone[is_good.index(i)]).all() and (got != logs[i]).any(), i
        else:
            assert (got == logs[i]).all(), i
    assert sorted(is_good + is_bad + [5]) == list(range(10))
    # nothing at all
    totals, rows, counts = stat_logs([], per_seat=True, lib=lib)
    assert totals[0] == totals[1] == Stat() and rows.shape == (0, 4, 44) and counts == dict(reduced=0, skipped=0, malformed=0)


# ---- the pool path: TablePool.log_stat on the log the step kernel wrote (tag words on every decision)
def check_pool(pool_cls, n, probe_cycle=40, max_cycles=8000):
    """n tables, obs v3, both agents on the device's greedy policy, log on, to completion: log_stat against the host reading of
    read_logs(), the group split against agent_of_seat; a call at `probe_cycle` finds every table still playing."""
    import parity_util

    pool = pool_cls(n, version=3)
    try:
        pool.enable_log()
        aos = np.array([(0b0110, 0b1001, 0b1110, 0b0000, 0b1111)[i % 5] for i in range(n)], dtype=np.uint8)
        pool.reset(parity_util.default_seeds(n), game_ids=np.arange(n), agent_of_seat=aos, n_games_total=n)
        acts, mid = [None, None], None
        for c in range(max_cycles):
            n_rows = pool.step(acts[0], acts[1])
            if c == probe_cycle:
                mid = pool.log_stat(per_seat=True)
            if n_rows[0] == 0 and n_rows[1] == 0 and pool.counters()["games"] >= n:
                break
            acts = [None, None]
            for a in (0, 1):
                if n_rows[a]:
                    obs, masks = pool.encode(a)
                    acts[a] = pool.greedy_policy(a, masks, obs, 7, c)
        assert pool.counters()["games"] == n and pool.first_error()[0] == 0
        totals, rows, counts = mid
        assert counts == dict(reduced=0, skipped=n, malformed=0) and not rows.any() and totals[0] == totals[1] == Stat()
        logs = pool.read_logs()
        tags = []
        ML.decode_events(logs[0], tags)
        assert any(t is not None for t in tags)  # device-played logs carry a tag word per decision
        want = expected(logs)
        totals, rows, counts = pool.log_stat(per_seat=True)
        assert counts == dict(reduced=n, skipped=0, malformed=0), counts
        assert (rows == want).all()
        assert (np.array([t.counters() for t in totals]) == totals_of(want, np.full(n, 15), aos)).all()
        assert totals[0].game + totals[1].game == 4 * n and totals[0].game == sum(4 - bin(int(b)).count("1") for b in aos)
        seats = np.array([(i * 5 + 1) & 15 for i in range(n)], dtype=np.uint8)
        totals, none, _ = pool.log_stat(seats=seats)
        assert none is None and (np.array([t.counters() for t in totals]) == totals_of(want, seats, aos)).all()
    finally:
        pool.close()
