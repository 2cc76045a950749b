"""-m gpu: libriichi's Stat reduced on the device (mortal_amd/csrc/mj_stat.hip) on the real library, against the host reading
`Stat.from_game(decode_events(words), seat)` per (log, seat) and in total, exactly.  The cases shared with the emulator leg
(tests/test_stat_device_emu.py) live in tests/stat_device_cases.py."""
import numpy as np
import pytest

import stat_device_cases as S

pytestmark = pytest.mark.gpu
KEY = 0xD5DFAA4CEF265CD7


def test_fixture_logs(oracle):
    S.check_fixture_logs(oracle, None)


def test_seat_masks_and_groups(oracle):
    S.check_masks_and_groups(oracle, None)


def test_alignment_sweep():
    S.check_alignment_sweep(None)


def test_alignment_sweep_grp():
    S.check_alignment_sweep_grp(None)


def test_bad_and_empty_input():
    S.check_bad_and_empty_input(None)


def test_more_logs_than_one_grid_pass(oracle):
    """5,003 logs (the 44 fixture logs repeated): not a multiple of the four wavefronts of a workgroup and more than the bounded
    grid takes in one pass, so wavefronts chain logs and the last workgroup is partly idle."""
    from mortal_amd.stat import stat_logs

    logs, want = S.fixture_logs(oracle)
    n = 5003
    idx = np.arange(n) % len(logs)
    many = [logs[i] for i in idx]
    seats = ((np.arange(n) * 11 + 5) & 15).astype(np.uint8)
    groups = ((np.arange(n) * 13 + 1) & 15).astype(np.uint8)
    totals, rows, counts = stat_logs(many, seats=seats, groups=groups, per_seat=True)
    assert counts == dict(reduced=n, skipped=0, malformed=0), counts
    sel = ((seats[:, None] >> np.arange(4)[None, :]) & 1).astype(np.int64)
    full = want[idx] * sel[:, :, None]
    for i in (0, 1, n // 2, n - 2, n - 1):  # the first, a middle and the last copy
        assert (rows[i] == full[i]).all(), i
    assert (rows == full).all()
    grp = ((groups[:, None] >> np.arange(4)[None, :]) & 1).astype(bool)
    tot = np.stack([(full * (~grp)[:, :, None]).sum(axis=(0, 1)), (full * grp[:, :, None]).sum(axis=(0, 1))])
    assert (np.array([t.counters() for t in totals]) == tot).all()
    totals2, none, counts2 = stat_logs(many, seats=seats, groups=groups)
    assert none is None and counts2 == counts and (np.array([t.counters() for t in totals2]) == tot).all()


def test_pool_log_stat():
    from mortal_amd.pool import TablePool

    S.check_pool(TablePool, 256)


def test_arena_collect_stat(oracle, tmp_path):
    """player.py's flow without the files: OneVsThree(collect_stat=True, log_dir=...) leaves in env.stats what Stat.from_dir
    reads back from the dumped logs."""
    import os

    import test_gpu_arena as G
    from libriichi.arena import OneVsThree
    from libriichi.stat import Stat

    chal, _ = G._engine(3, 1, "challenger", True)
    cham, _ = G._engine(3, 2, "champion", True)
    d = str(tmp_path / "logs")
    env = OneVsThree(disable_progress_bar=True, log_dir=d, collect_stat=True)
    got = env.py_vs_py(challenger=chal, champion=cham, seed_start=(10000, KEY), seed_count=2)
    assert len(os.listdir(d)) == 8 and sorted(env.stats) == ["challenger", "champion"]
    for name in ("challenger", "champion"):
        assert env.stats[name] == Stat.from_dir(d, name, True), name
    st = env.stats["challenger"]
    assert st.game == 8 and [st.rank_1, st.rank_2, st.rank_3, st.rank_4] == got and env.stats["champion"].game == 24
