"""The sample store (mortal_amd/csrc/mj_samples.hip behind mj_samples_*; SampleStore, GameplayLoader.store_pool / store_harvest, the
runners' sample_store), run on the host emulation of the device code.  The cases and their yardsticks live in
tests/sample_store_cases.py, shared with the `-m gpu` leg; the allocation and synchronise failures at the end are the emulator's own."""
import gc
import os
import shutil
import sys

import numpy as np
import pytest

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
if HOST not in sys.path:
    sys.path.insert(0, HOST)

from emu_alloc import stats as _stats  # noqa: E402
import pool_gameplay_cases as G  # noqa: E402
import sample_store_cases as SC  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build_emu

    if not (os.path.exists(build_emu.CXX) or shutil.which("g++")):
        pytest.skip("no host C++ compiler")
    import emu_pool

    return emu_pool.make_pool_class()


@pytest.fixture(scope="module")
def played(oracle, emu):
    """Three finished games, their logs and the reference's reading of them, shared and left unchanged."""
    P = SC.Played(oracle, emu, 3)
    yield P
    P.close()


def test_store_equals_the_reference_loader_v3(played):
    assert SC.check_parity(played, 3, SC.TABLE0, SC.SEATS, 24, want_census=True) > 1000


def test_store_equals_the_reference_loader_v4(played):
    assert SC.check_parity(played, 4, 1, [2, 4], 16) > 200


def test_shuffled_batches_v3(played):
    assert SC.check_shuffled(played, 3, SC.TABLE0, SC.SEATS, 24) == 1 + 24 + 25 + 67 + 3 + 2


def test_shuffled_batches_v4(played):
    assert SC.check_shuffled(played, 4, 1, [2, 4], 16) == 1 + 16 + 17 + 43 + 3 + 2


@pytest.mark.parametrize("version", [1, 3])
def test_invisible_obs(played, version):
    assert SC.check_invisible(played, version, 0, 5) > 200


def test_augmented(played):
    assert SC.check_augmented(played, 2, 10) > 200


def test_two_harvests_into_one_store(oracle, emu):
    assert SC.check_harvest(oracle, emu) > 200


def test_capacity_and_refusals(played):
    SC.check_capacity_and_refusals(played)


def test_bytes_per_sample(emu):
    SC.check_size(emu._L)


def test_batch_runner_sample_store(oracle, emu):
    SC.check_batch_runner(oracle, emu)


def test_self_play_runner_sample_store(oracle, emu):
    SC.check_self_play_runner(oracle, emu)


# ---- allocation and synchronise failures (as tests/test_emu_pool_gameplay.py sweeps mj_replay_load_pool)
@pytest.mark.parametrize("version", [3, 4])
def test_allocation_and_synchronise_failures(emu, version):
    """For every allocation and every synchronise of mj_samples_create, mj_samples_append and the store's first mj_samples_encode
    (for obs v4 that is the SP set-up too; three indices on two rows per launch: two chunks and a grown index buffer): the call
    fails, nothing is freed twice, the same call then succeeds, the store encodes the bytes of a run that never saw a failure, and
    when it is destroyed the live allocations are back at the baseline."""
    from mortal_amd import mjai_log as ML
    from mortal_amd.pool import OBS_ROWS

    L = emu._L
    script = ML.encode_events(G.golden_events())
    rp = emu(2, version=version)
    try:
        rp.replay_load([script] * 2, [0xF] * 2)
        while rp.replay_step() == 0:
            pass
        n_rows = rp.n_rows[0]
        assert n_rows >= 2
        idx = np.array([n_rows - 1, 0, 0], dtype=np.int32)

        def create(h):
            return L.mj_samples_create(64, version, 2)

        def append(h):
            return L.mj_samples_append(h, rp.h, 0, None)

        out = {}

        def encode(h):
            obs = np.full((3, OBS_ROWS[version], 34), np.nan, dtype=np.float32)
            masks = np.full((3, 46), 0xA5, dtype=np.uint8)
            rc = L.mj_samples_encode(h, idx.ctypes.data, 3, obs.ctypes.data, masks.ctypes.data, None)
            out["bytes"] = obs.tobytes() + masks.tobytes()
            return rc

        calls = [("create", create), ("append", append), ("encode", encode)]

        def failed(rc):
            return rc is None or rc == -1

        gc.collect()
        base = _stats(L)["live"]
        # the undisturbed run: what each call allocates and synchronises, and the bytes
        made, h = {}, None
        for name, call in calls:
            before = _stats(L)
            rc = call(h)
            assert not failed(rc), (name, L.mj_last_error().decode())
            if name == "create":
                h = rc
            made[name] = {kind: _stats(L)[kind] - before[kind] for kind in ("alloc", "sync")}
        want = out["bytes"]
        assert not np.isnan(np.frombuffer(want[:3 * OBS_ROWS[version] * 34 * 4], dtype=np.float32)).any()
        L.mj_samples_destroy(h)
        assert _stats(L)["live"] == base and _stats(L)["bad_frees"] == 0
        assert made["create"]["alloc"] >= 12 and made["encode"]["alloc"] >= (8 if version == 4 else 2), made
        assert version != 4 or made["encode"]["sync"] >= 2, made
        n_cases = 0
        for victim in range(3):
            for kind, k in [(kind, k) for kind in ("alloc", "sync") for k in range(1, made[calls[victim][0]][kind] + 1)]:
                h = None
                for i, (name, call) in enumerate(calls):
                    if i == victim:
                        L.mj_emu_fail_nth(k if kind == "alloc" else 0, k if kind == "sync" else 0)
                        rc = call(h)
                        L.mj_emu_fail_nth(0, 0)
                        assert failed(rc) and L.mj_last_error().decode(), (name, kind, k)
                        assert _stats(L)["bad_frees"] == 0, (name, kind, k)
                        if name == "create":
                            assert _stats(L)["live"] == base, (kind, k)
                    rc = call(h)
                    assert not failed(rc), (name, kind, k, L.mj_last_error().decode())
                    if name == "create":
                        h = rc
                assert out["bytes"] == want, (calls[victim][0], kind, k)
                info = np.zeros(4, dtype=np.int64)
                assert L.mj_samples_info(h, info.ctypes.data) == 0 and info.tolist()[:2] == [n_rows, 64] and info[3] == 0
                L.mj_samples_destroy(h)
                assert _stats(L)["live"] == base and _stats(L)["bad_frees"] == 0, (calls[victim][0], kind, k)
                n_cases += 1
        assert n_cases >= 14
    finally:
        rp.close()
