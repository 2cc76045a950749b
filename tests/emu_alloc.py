"""Shared by the test_emu_* modules that watch the emulated runtime's registry (tests/host/emu/hip/hip_runtime.h through
mj_emu_alloc_stats) or drive a replay pool by hand."""
import ctypes as C


def stats(L):
    """live = (buffers, events, streams) of library L that are allocated now; frees of something not live; allocations and stream
    synchronises so far."""
    out = (C.c_uint64 * 6)()
    L.mj_emu_alloc_stats(out)
    return dict(live=(out[0], out[1], out[2]), bad_frees=out[3], alloc=out[4], sync=out[5])


def first_samples(pool, steps=8):
    """Rows, obs, masks and meta of a replay pool's first steps, encoded from the pool itself (TablePool.encode / replay_meta)."""
    out = []
    for _ in range(steps):
        if pool.replay_step():
            obs, masks = pool.encode(0)
            out += [pool.rows(0).tobytes(), obs.numpy().tobytes(), masks.numpy().tobytes(), pool.replay_meta().numpy().tobytes()]
    assert len(out) >= 4
    return b"".join(out)
