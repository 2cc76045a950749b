"""Shared by tests/test_gpu_pool_augment.py (the real library, `-m gpu`) and tests/test_emu_pool_augment.py (host emulation of the
device code): suit augmentation on the device (mj_k_log_pack<true> in mortal_amd/csrc/mj_gameplay.hip behind MJ_LOAD_AUGMENT and
mj_augment_logs; GameplayLoader.load_pool / load_harvest(..., augmented=True), mjai_log.augment_logs).

The yardsticks are never the code under test: packed words are compared with the host codec (mjai_log.encode_events(...,
augmented=True), the code behind load_logs), samples with the reference loader restated on the oracle (tests/dataset_ref.py) over
the suit-swapped events, and with the host route GameplayLoader(augmented=True).load_logs over the dumped JSON of the same games.
Every comparison is exact.

The played games are those of tests/pool_gameplay_cases.py: table t plays seed (G.SEED_START + t, G.KEY) under the greedy policy.
Tables 0..2 were played on the CPU emulator and counted (conditions() below): 5 start_kyoku whose payload crosses a 64-word
boundary, 141 chi / pon, 11 kans -- every role the copy kernel carries from one window into the next occurs in them."""
import numpy as np

import dataset_ref
import harvest_cases as H
import pool_gameplay_cases as G

from mortal_amd import mjai_log as ML
from mortal_amd.dataset import GameplayLoader

TN = ML.TILE_NAMES
# tag words as a pool writes them (bit 63 set), chosen to read as a start_kyoku header with the wall bit and as a hora header with
# n_ura = 5: the kernel must know them by their place in the chain, never by their bits
TAG_AS_START_KYOKU = (1 << 63) | (3 << 56) | (77 << 20) | 0x12341
TAG_AS_HORA = (1 << 63) | (2 << 56) | (5 << 39) | (9 << 20) | 0x0432C
# 52 haipai tiles of every suit and every branch of the swap: the ends of manzu (0, 8), pinzu (9, 17) and souzu (18, 26), the first and
# the last honour (27, 33) and the three red fives (34, 35, 36)
HAIPAI = [0, 8, 9, 17, 18, 26, 27, 33, 34, 35, 36] + [(5 * i + 2) % 34 for i in range(41)]
# scores whose packed words read as a start_kyoku header (low 4 bits 1) and as a hora header (12)
SCORES = [24993, 25007, 25004, 24996]
assert len(HAIPAI) == 52 and SCORES[0] & 15 == ML.LG_START_KYOKU and SCORES[2] & 15 == ML.LG_HORA and sum(SCORES) == 100_000


def start_kyoku(marker="5mr"):
    return dict(type="start_kyoku", bakaze="S", dora_marker=marker, kyoku=3, honba=2, kyotaku=1, oya=2, scores=list(SCORES),
                tehais=[[TN[x] for x in HAIPAI[s * 13:(s + 1) * 13]] for s in range(4)])


def directed_events(k):
    """k one-word fillers, a start_kyoku, one of every event that holds tiles, a tagged dahai, a tagged hora with 5 ura indicators,
    a hora with none, a ryukyoku, an end_kyoku -> list of (event, tag word or None).  The chain is well formed, the game is not
    legal: only the walk is under test."""
    ev = [(dict(type="reach", actor=i & 3), None) for i in range(k)]
    ev += [(start_kyoku(), None),
           (dict(type="tsumo", actor=0, pai="9m"), None),
           (dict(type="dahai", actor=0, pai="1p", tsumogiri=True), None),
           (dict(type="chi", actor=1, target=0, pai="1p", consumed=["2p", "3p"]), None),
           (dict(type="pon", actor=2, target=1, pai="5mr", consumed=["5m", "5m"]), None),
           (dict(type="daiminkan", actor=3, target=2, pai="9p", consumed=["9p", "9p", "9p"]), None),
           (dict(type="kakan", actor=2, pai="5m", consumed=["5mr", "5m", "5m"]), None),
           (dict(type="ankan", actor=0, consumed=["5p", "5p", "5p", "5pr"]), None),
           (dict(type="dahai", actor=1, pai="1m", tsumogiri=False), TAG_AS_START_KYOKU),
           (dict(type="hora", actor=2, target=1, deltas=[1, -8001, 8012, -12], ura_markers=["1m", "9p", "5sr", "5pr", "C"]), TAG_AS_HORA),
           (dict(type="hora", actor=3, target=3, deltas=[-1000, -1000, -2000, 4000], ura_markers=[]), None),
           (dict(type="ryukyoku", deltas=[12, -1, 1, -12]), None),
           (dict(type="end_kyoku"), None)]
    return ev


def words_of(tagged_events, augmented=False):
    """The packed words, each tag word behind its header (LG_TAG_BIT set); with `augmented` the host codec swaps the tiles and the
    tags stay what they are: what the device must give."""
    out = []
    for e, tag in tagged_events:
        w = [int(x) for x in ML.encode_events([e], augmented=augmented)]
        out += [w[0] | (1 << 43), tag] + w[1:] if tag is not None else w
    return np.array(out, dtype=np.uint64)


def wall_log(augmented=False):
    """50 fillers, a start_kyoku with LG_SK_WALL_BIT (27 words, the wall words cross index 63 | 64), 44 fillers, a plain start_kyoku
    whose haipai crosses 127 | 128, an end_kyoku."""
    rest = [x for x in range(34) for _ in range(4)]
    for x in HAIPAI:
        rest.remove(x if x < 34 else (4, 13, 22)[x - 34])
    wall = HAIPAI + rest
    assert len(wall) == 136
    if augmented:
        wall = [ML.augment_tile_id(x) for x in wall]
    fill = lambda n: [int(x) for x in ML.encode_events([dict(type="reach", actor=i & 3) for i in range(n)])]  # noqa: E731
    sk_wall = [int(x) for x in ML.encode_events([start_kyoku("9p")], augmented=augmented, walls=[wall])]
    sk = [int(x) for x in ML.encode_events([start_kyoku("E")], augmented=augmented)]
    assert len(sk_wall) == 27 and len(sk) == 10
    return np.array(fill(50) + sk_wall + fill(44) + sk + [ML.LG_END_KYOKU], dtype=np.uint64)


def roles_at(words):
    """index -> 'header' / 'haipai' / 'wall' / 'ura' / 'tag' / 'other' by walking the chain on the host."""
    roles, i = {}, 0
    while i < len(words):
        w = int(words[i])
        t = w & 15
        roles[i] = "header"
        if t == ML.LG_START_KYOKU:
            n = 27 if (w >> 63) & 1 else 10
            for j in range(1, n):
                roles[i + j] = "other" if j < 3 else "haipai" if j < 10 else "wall"
        else:
            tag = (w >> 43) & 1
            n = (4 if t == ML.LG_HORA else 3 if t == ML.LG_RYUKYOKU else 1) + tag
            for j in range(1, n):
                roles[i + j] = "tag" if tag and j == 1 else "ura" if t == ML.LG_HORA and j == n - 1 else "other"
        i += n
    return roles


def strip_tags(words):
    """The words without tag words and tag bits (what decode_events reads), and the (index, word) of every tag word."""
    out, tags = [], []
    roles = roles_at(words)
    for i, w in enumerate(words):
        if roles[i] == "tag":
            tags.append((i, int(w)))
        elif roles[i] == "header" and int(w) & 15 != ML.LG_START_KYOKU:
            out.append(int(w) & ~(1 << 43))
        else:
            out.append(int(w))
    return np.array(out, dtype=np.uint64), tags


def raw_augment(lib, logs, stream=None):
    """mj_augment_logs itself -> (list of arrays, counts); the output is pre-filled with a pattern: every word must be written."""
    n = len(logs)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in logs])
    words = np.ascontiguousarray(np.concatenate(logs), dtype=np.uint64)
    out = np.full(len(words), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    counts = np.full(3, 7, dtype=np.int64)
    rc = lib.mj_augment_logs(words.ctypes.data, off.ctypes.data, n, out.ctypes.data, counts.ctypes.data, stream)
    assert rc == 0, lib.mj_last_error().decode()
    return [out[off[i]:off[i + 1]].copy() for i in range(n)], counts.tolist()


def directed_logs():
    """-> (logs, expected): the 64 window offsets, the wall log, an empty log, one with an unknown event type, one cut inside a
    start_kyoku's payload (both malformed: expected unchanged)."""
    logs = [words_of(directed_events(k)) for k in range(64)] + [wall_log()]
    want = [words_of(directed_events(k), augmented=True) for k in range(64)] + [wall_log(augmented=True)]
    unknown = logs[5].copy()
    unknown[20] = (unknown[20] & ~np.uint64(15)) | np.uint64(15)  # the kakan's header becomes type 15
    assert roles_at(logs[5])[20] == "header"
    cut = logs[9][:9 + 6].copy()  # ends inside the haipai words
    extra = [np.zeros(0, dtype=np.uint64), unknown, cut]
    return logs + extra, want + [x.copy() for x in extra]


def check_directed(lib, stream=None, py_kw=None):
    """Case 1.  py_kw: what mjai_log.augment_logs is given besides the logs (None: `lib`)."""
    import pytest

    logs, want = directed_logs()
    n_ok = 65
    # the set of logs puts each carried role on both sides of the window boundary 63 | 64
    for role in ("haipai", "ura", "tag", "wall"):
        for index in (63, 64):
            assert any(roles_at(x).get(index) == role for x in logs[:n_ok]), (role, index)
    assert any(roles_at(x).get(127) == roles_at(x).get(128) == "haipai" for x in logs[:n_ok])
    # score and tag words that read as headers, all branches of the swap
    assert int(logs[0][1]) & 15 == ML.LG_START_KYOKU and int(logs[0][2]) & 15 == ML.LG_HORA
    got, counts = raw_augment(lib, logs, stream)
    assert counts == [n_ok, 1, 2], counts
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and (g == w).all(), (i, [hex(int(x)) for x in g[g != w][:4]], np.flatnonzero(g != w)[:8])
    for i in range(64):
        # the untagged events through the host codec, the tags where and what they were
        plain, tags = strip_tags(got[i])
        assert (plain == ML.encode_events(ML.decode_events(logs[i]), augmented=True)).all(), i
        assert tags == strip_tags(logs[i])[1] and len(tags) == 2, i
        heads = [j for j, r in roles_at(logs[i]).items() if r == "header" and int(logs[i][j]) & 15 != ML.LG_START_KYOKU]
        assert [(int(got[i][j]) >> 43) & 1 for j in heads] == [(int(logs[i][j]) >> 43) & 1 for j in heads], i
    assert (got[0] != logs[0]).sum() >= 15  # (the swap did something: header fields, haipai words, the ura word)
    back, counts2 = raw_augment(lib, got, stream)
    assert counts2 == counts
    for i, (b, x) in enumerate(zip(back, logs)):
        assert (b == x).all(), i
    # the Python entry: the same words for the good logs, the first malformed one named
    kw = dict(lib=lib) if py_kw is None else py_kw
    for g, w in zip(ML.augment_logs(logs[:n_ok + 1], **kw), want[:n_ok + 1]):
        assert g.dtype == np.uint64 and len(g) == len(w) and (g == w).all()
    with pytest.raises(ValueError, match=f"log {n_ok + 1} "):
        ML.augment_logs(logs, **kw)
    assert ML.augment_logs([], **kw) == []


# ---- played games
def conditions(logs):
    """Counted on the host over the packed logs: start_kyoku / hora whose payload crosses a 64-word boundary, chi / pon, kans."""
    cross = calls = kans = 0
    for words in logs:
        roles = roles_at(words)
        heads = [i for i in sorted(roles) if roles[i] == "header"] + [len(words)]
        for i, nxt in zip(heads, heads[1:]):
            t = int(words[i]) & 15
            cross += t in (ML.LG_START_KYOKU, ML.LG_HORA) and i // 64 != (nxt - 1) // 64
            calls += t in (ML.LG_CHI, ML.LG_PON)
            kans += t in (ML.LG_DAIMINKAN, ML.LG_KAKAN, ML.LG_ANKAN)
    return dict(crossing=cross, calls=calls, kans=kans)


def aug_events(ev):
    """The events as the reference's augmented loader sees them, through the host codec."""
    return ML.decode_events(ML.encode_events(ev, augmented=True))


def ref_game(seed, words, names, augmented=True):
    ev = ML.decode_events(words)
    return [dict(type="start_game", names=list(names), seed=[int(seed[0]), int(seed[1])])] + (aug_events(ev) if augmented else ev) \
        + [dict(type="end_game")]


def raw_json(seed, words, names):
    return ML.dump_json_log(names, seed, ML.decode_events(words))


def host_loader(pool_cls, version, **kw):
    """The host route: GameplayLoader(augmented=True).load_logs, on the library under test."""
    loader = GameplayLoader(version, augmented=True, **kw)
    loader.pool_cls = pool_cls
    return loader


def check_pool_route(oracle, pool_cls, pool, logs, version, n, want_conditions=True):
    """Case 2 over tables [0, n) of a finished pool."""
    if want_conditions:
        cs = conditions(logs[:n])
        print("conditions", cs)
        assert cs["crossing"] >= 1 and cs["calls"] >= 1 and cs["kans"] >= 1, cs
    seeds = G.seeds(pool.n_tables)
    loader = GameplayLoader(version, oracle=False)
    got = loader.load_pool(pool, 0, n, names=[G.NAMES] * n, augmented=True)
    assert len(got) == n
    got_bytes = G.samples_bytes(got)  # (before check_gameplay takes the obs away)
    total = 0
    for t in range(n):
        assert [g.player_id for g in got[t]] == [0, 1, 2, 3]
        ev = ref_game(seeds[t], logs[t], G.NAMES)
        for g in got[t]:
            total += G.check_gameplay(oracle, g, ev, version, True)
    host = host_loader(pool_cls, version, oracle=False).load_logs([raw_json(seeds[t], logs[t], G.NAMES) for t in range(n)])
    assert got_bytes == G.samples_bytes(host)
    plain = loader.load_pool(pool, 0, n, names=[G.NAMES] * n)
    assert got_bytes != G.samples_bytes(plain)
    for a, b in zip(got, plain):
        for x, y in zip(a, b):
            G.same_grp(x.grp, y.grp)
    assert [(w == again).all() for w, again in zip(logs, pool.read_logs())] == [True] * len(logs)  # the pool's log is not swapped
    return total


def check_invisible(pool_cls, n, version, deal_algo):
    """Case 3: events swapped, wall as the seed deals it -- byte for byte the host route with trust_seed."""
    pool = G.play(pool_cls, n, version=version, deal_algo=deal_algo)
    try:
        logs = pool.read_logs()
        got = GameplayLoader(version, oracle=True, deal_algo=deal_algo).load_pool(pool, augmented=True)  # (raises on MJ_ERR_WALL)
        plain = GameplayLoader(version, oracle=True, deal_algo=deal_algo).load_pool(pool, 0, 1)
        host = host_loader(pool_cls, version, oracle=True, trust_seed=True, deal_algo=deal_algo).load_logs(
            [raw_json(G.seeds(n)[t], logs[t], ["", "", "", ""]) for t in range(n)])
        total = 0
        for t in range(n):
            assert [g.player_id for g in got[t]] == [g.player_id for g in host[t]] == [0, 1, 2, 3]
            for a, b in zip(got[t], host[t]):
                x, y = np.stack(a.invisible_obs), np.stack(b.invisible_obs)
                assert x.shape == y.shape and len(x) == len(a.actions) > 0 and x.tobytes() == y.tobytes(), (t, a.player_id)
                total += len(x)
        assert G.samples_bytes(got) == G.samples_bytes(host)
        assert np.stack(got[0][0].invisible_obs).tobytes() != np.stack(plain[0][0].invisible_obs).tobytes()
        return total
    finally:
        pool.close()


def check_harvest_route(oracle, pool_cls, n=3, victim=1):
    """Case 4, first part: a refilling pool with one game in error."""
    import pytest

    run = H.Run(pool_cls, n, poison=(victim, 60))
    try:
        run.play_until(run.every_table(1), 8000)
        h = run.pool.take_harvest()
        try:
            keys = H.keys_of(run, h)
            assert (victim, 0) in keys and run.snap((victim, 0))["err"] == 1 and len(keys) >= n
            logs = h.read_logs()
            loader = GameplayLoader(3, oracle=False)
            got = loader.load_harvest(h, names=[G.NAMES] * len(keys), augmented=True)
            assert len(got) == len(keys)
            good = [i for i, k in enumerate(keys) if not run.snap(k)["err"]]
            got_bytes = G.samples_bytes([got[i] for i in good])  # (before check_gameplay takes the obs away)
            total = 0
            for i, key in enumerate(keys):
                if i not in good:
                    assert got[i] == [] and len(logs[i]) == 0
                    continue
                ev = ref_game(run.seed(key), logs[i], G.NAMES)
                assert [g.player_id for g in got[i]] == [0, 1, 2, 3]
                for g in got[i]:
                    total += G.check_gameplay(oracle, g, ev, 3, True)
            host = host_loader(pool_cls, 3, oracle=False).load_logs([raw_json(run.seed(keys[i]), logs[i], G.NAMES) for i in good])
            assert got_bytes == G.samples_bytes(host)
            rp = pool_cls(len(keys), version=3)
            try:
                assert rp.replay_load_harvest(h, 0, augmented=True) == dict(loaded=len(good), skipped=len(keys) - len(good), malformed=0)
            finally:
                rp.close()
            assert [(a == b).all() for a, b in zip(logs, h.read_logs())] == [True] * len(logs)
            with pytest.raises(ValueError, match=r"augmented.*per call"):
                GameplayLoader(3, oracle=False, augmented=True).load_harvest(h)
            return total
        finally:
            h.close()
    finally:
        run.close()


def check_runners(pool_cls, n_tables=2):
    """Case 4, second part: both runners pass the keyword on and name the seats by engine."""
    import test_sharding as TS

    from mortal_amd import arena as A

    engines = lambda: [TS._LowestLegalEngine("a"), TS._LowestLegalEngine("b")]  # noqa: E731
    aos = np.array([0b0001, 0b0110][:n_tables], dtype=np.uint8)
    loader = GameplayLoader(3, oracle=False, player_names=["b"])
    old = A.SelfPlayRunner.pool_cls, A.BatchRunner.pool_cls
    A.SelfPlayRunner.pool_cls = A.BatchRunner.pool_cls = pool_cls
    try:
        runner = A.SelfPlayRunner(engines(), n_tables, (10000, G.KEY), aos, deal_algo=0, max_games=8 * n_tables,
                                  max_words=8 * n_tables * 4096)
        try:
            h = runner.play(min_games=n_tables)
            try:
                got = runner.gameplays(loader, h, augmented=True)
                tables = [int(r["table"]) for r in h.games]
                names = [["b" if (int(aos[t]) >> s) & 1 else "a" for s in range(4)] for t in tables]
                want = host_loader(pool_cls, 3, oracle=False, player_names=["b"]).load_logs(
                    [raw_json((int(r["seed_nonce"]), int(r["seed_key"])), w, nm) for r, w, nm in zip(h.games, h.read_logs(), names)])
                assert [[g.player_id for g in per] for per in got] == [[s for s in range(4) if (int(aos[t]) >> s) & 1] for t in tables]
                assert all(g.player_name == "b" for per in got for g in per)
                assert G.samples_bytes(got) == G.samples_bytes(want) != G.samples_bytes(runner.gameplays(loader, h))
            finally:
                h.close()
        finally:
            runner.close()
        seeds = [(10000 + t, G.KEY) for t in range(n_tables)]
        runner = A.BatchRunner(engines(), seeds, aos, deal_algo=0, keep_stat=True)
        try:
            runner.run()
            got = runner.gameplays(loader, augmented=True)
            names = [["b" if (int(aos[t]) >> s) & 1 else "a" for s in range(4)] for t in range(n_tables)]
            want = host_loader(pool_cls, 3, oracle=False, player_names=["b"]).load_logs(
                [raw_json(seeds[t], w, names[t]) for t, w in enumerate(runner.pool.read_logs())])
            assert [[g.player_id for g in per] for per in got] == [[s for s in range(4) if (int(aos[t]) >> s) & 1] for t in range(n_tables)]
            assert all(g.player_name == "b" for per in got for g in per)
            assert G.samples_bytes(got) == G.samples_bytes(want) != G.samples_bytes(runner.gameplays(loader))
        finally:
            runner.close()
    finally:
        A.SelfPlayRunner.pool_cls, A.BatchRunner.pool_cls = old


def first_samples(p, steps=12):
    """The first samples of whatever p has loaded."""
    out = []
    for _ in range(steps):
        if p.replay_step():
            obs, masks = p.encode(0)
            out += [p.rows(0).tobytes(), obs.cpu().numpy().tobytes(), masks.cpu().numpy().tobytes(),
                    p.replay_meta().cpu().numpy().tobytes()]
    return b"".join(out)


def check_refusals(pool_cls, pool, version=3):
    """Case 5: an unknown flag bit is refused and leaves the destination usable; a loader constructed with augmented=True is
    refused by both device routes and told where the keyword goes."""
    import pytest

    L = pool_cls._L
    counts = np.zeros(3, dtype=np.int64)
    fresh = pool_cls(2, version=version)
    dst = pool_cls(2, version=version)
    try:
        assert fresh.replay_load_pool(pool, augmented=True) == dict(loaded=2, skipped=0, malformed=0)
        want = first_samples(fresh)
        assert len(want) > 1000
        dst.replay_load_pool(pool)
        plain = first_samples(dst, 5)
        assert plain and not want.startswith(plain)  # (a replay under way, on the un-augmented script)
        for flags in (4, 5, 6, 7, 1 << 16, -1):
            assert L.mj_replay_load_pool(dst.h, pool.h, 0, None, 1, flags, counts.ctypes.data, dst._stream()) == -1
            assert "unknown load flags" in L.mj_last_error().decode() and counts.tolist() == [0, 0, 0]
        assert dst.replay_load_pool(pool, augmented=True) == dict(loaded=2, skipped=0, malformed=0)
        assert first_samples(dst) == want
    finally:
        fresh.close()
        dst.close()
    with pytest.raises(ValueError, match=r"augmented.*per call"):
        GameplayLoader(version, oracle=False, augmented=True).load_pool(pool)
    with pytest.raises(ValueError, match=r"augmented.*per call"):
        GameplayLoader(version, oracle=False, augmented=True).load_pool(pool, augmented=True)
