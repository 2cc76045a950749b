"""ctypes binding of the C-ABI in include/mortal_amd.h (libmortal_amd.so, built by __graft_entry__.build()).

There is no fallback: if the shared library is missing or fails to load, importing this module raises.
"""
import ctypes as C
import os

# torch ships its own libamdhip64; it must be in the process before libmortal_amd.so is opened, otherwise the
# system copy gets bound first and the two HIP runtimes disagree about the visible devices
import torch

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MORTAL_AMD_LIB") or os.path.join(_DIR, "libmortal_amd.so")  # env override: A/B builds

_vp, _i32, _u32, _u64, _i64, _sz, _str = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_int64, C.c_size_t, C.c_char_p
# name: (restype, argtypes) of every symbol include/mortal_amd.h declares (tests/test_host.py checks the names and the number
# of parameters against the header, and that the library exports all of them)
PROTOTYPES = {
    "mj_last_error": (_str, []),
    "mj_abi_version": (_i32, []),
    "mj_tables_upload": (_i32, [_vp, _sz]),
    "mj_pool_create": (_vp, [_i32, _i32, _i32, _i32]),
    "mj_pool_destroy": (None, [_vp]),
    "mj_pool_reset": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32]),
    "mj_pool_configure": (_i32, [_vp, _i32, _i32, _i32, _i32]),
    "mj_pool_set_refill": (_i32, [_vp, _u64]),
    "mj_pool_set_start_stagger": (_i32, [_vp, _u32, _vp]),
    "mj_table_apply_event": (_i32, [_vp, _i32, _vp, _i32, _vp]),
    "mj_table_mark_row": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "mj_table_query": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mj_replay_load": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "mj_replay_step": (_i32, [_vp, _vp]),
    "mj_replay_meta": (_i32, [_vp, _vp, _vp]),
    "mj_pool_enable_log": (_i32, [_vp, _u32]),
    "mj_log_lengths": (_i32, [_vp, _vp, _vp]),
    "mj_log_read": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "mj_step": (_i32, [_vp, _vp, _vp, _vp]),
    "mj_step_q": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mj_step_ev": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mj_rows_count": (_i32, [_vp, _vp, _vp]),
    "mj_rows_dev": (_vp, [_vp, _i32]),
    "mj_encode": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "mj_encode_oracle": (_i32, [_vp, _i32, _vp, _vp]),
    "mj_oracle_obs_rows": (_i32, [_i32]),
    "mj_encode_timing": (_i32, [_vp, _i32, _vp, _vp]),
    "mj_sp_timing": (_i32, [_vp, _vp, _vp]),
    "mj_sp_phase_ticks": (_i32, [_vp, _vp, _vp]),
    "mj_pool_set_sp_schedule": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32]),
    "mj_sp_schedule_stats": (_i32, [_vp, _vp, _vp]),
    "mj_random_policy": (_i32, [_vp, _i32, _vp, _u64, _u64, _vp, _vp]),
    "mj_greedy_policy": (_i32, [_vp, _i32, _vp, _vp, _u64, _u64, _vp, _vp]),
    "mj_counters": (_i32, [_vp, _vp, _vp]),
    "mj_results": (_i32, [_vp, _vp, _vp, _vp]),
    "mj_pool_first_error": (_i32, [_vp, _vp, _vp]),
    "mj_debug_table": (_i32, [_vp, _i32, _vp, _sz, _vp]),
    "mj_debug_table_size": (_sz, []),
    "mj_debug_layout": (_str, []),
    "mj_obs_rows": (_i32, [_i32]),
    "mj_algo_query": (_i32, [_vp, _i32, _vp, _vp]),
    "mj_stat_logs": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mj_pool_stat": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mj_replay_load_pool": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp]),
    "mj_grp_logs": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mj_pool_grp": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mj_augment_logs": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "mj_pool_enable_harvest": (_i32, [_vp, _u32, _u64]),
    "mj_harvest_pending": (_i32, [_vp, _vp, _vp]),
    "mj_harvest_take": (_i32, [_vp, _vp, _vp]),
    "mj_harvest_destroy": (None, [_vp]),
    "mj_harvest_info": (_i32, [_vp, _vp]),
    "mj_harvest_games": (_i32, [_vp, _vp]),
    "mj_harvest_read": (_i32, [_vp, _i32, _vp]),
    "mj_harvest_stat": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mj_harvest_grp": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mj_replay_load_harvest": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp]),
    "mj_samples_create": (_vp, [_i64, _i32, _i32]),
    "mj_samples_destroy": (None, [_vp]),
    "mj_samples_append": (_i32, [_vp, _vp, _i32, _vp]),
    "mj_samples_truncate": (_i32, [_vp, _i64]),
    "mj_samples_info": (_i32, [_vp, _vp]),
    "mj_samples_meta": (_i32, [_vp, _i64, _i64, _vp, _vp]),
    "mj_samples_encode": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "mj_samples_encode_oracle": (_i32, [_vp, _vp, _i32, _vp, _vp]),
}
SYMBOLS = list(PROTOTYPES)


class MortalAmdError(RuntimeError):
    pass


def _hip_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _no_stream():
    return None


class Library:
    """One loaded C-ABI library: its functions, its own error text and the stream its calls take.  A pool, a harvest and
    everything made from them call, check and take their stream through the Library they were created on, so an error is
    never described by another library's mj_last_error (the test suite runs a host emulation next to the product)."""

    def __init__(self, path, host_emulation=False):
        self.cdll = C.CDLL(path)
        for name, (restype, argtypes) in PROTOTYPES.items():  # plain attributes, bound once: pool.step is a hot loop
            fn = getattr(self.cdll, name)
            fn.restype, fn.argtypes = restype, argtypes
            setattr(self, name, fn)
        # stream() -> the stream argument of a call: torch's current HIP stream; the host emulation has none
        self.stream = _no_stream if host_emulation else _hip_stream
        self.host_emulation = bool(host_emulation)  # its "device" memory is host memory (SampleStore puts its tensors there)

    def __getattr__(self, name):
        """Only a name outside the header gets here (a test hook the emulation build exports): bound on first use."""
        if not name.startswith("mj_"):
            raise AttributeError(name)
        fn = getattr(self.cdll, name)
        setattr(self, name, fn)
        return fn

    def check(self, rc):
        """rc of a call into this library -> rc, or MortalAmdError with this library's text when it reports a failure."""
        if rc is None or rc < 0:
            raise MortalAmdError(self.mj_last_error().decode())
        return rc


def _load(path=None, host_emulation=None):
    """dlopen the C-ABI library and declare its prototypes -> Library.  `path` and `host_emulation` are for the test suite
    only (the host emulation of the same sources, tests/host); the product always binds LIB_PATH.  A library loaded from a
    given path is the emulation unless the caller says otherwise: an A/B build of the product comes through MORTAL_AMD_LIB."""
    if host_emulation is None:
        host_emulation = path is not None
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise MortalAmdError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The HIP extension is mandatory; there is no CPU fallback."
        )
    return Library(path, host_emulation)


lib = _load()
