"""CPU-only checks of the host side: C-ABI exports, libriichi surface, seat/seed planning, proxy zero-copy trick."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_every_declared_symbol():
    """The shared library must load without a GPU and export every symbol include/mortal_amd.h declares."""
    import __graft_entry__ as g

    g.build()
    hdr = open(os.path.join(ROOT, "include", "mortal_amd.h")).read()
    declared = set(re.findall(r"\b(mj_[a-z0-9_]+)\s*\(", hdr))
    from mortal_amd import _lib

    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    # every declaration's parameter list (plain C, over several lines for some, `(void)` for none) has as many entries as the
    # binding's argtypes
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", hdr, flags=re.S)
    params = {name: [p for p in re.split(r"\s*,\s*", plist.strip()) if p != "void"]
              for name, plist in re.findall(r"\b(mj_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code)}
    assert set(params) == declared, set(params) ^ declared
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        assert len(argtypes) == len(params[name]) and "" not in params[name], (name, params[name], argtypes)
    assert len(params["mj_pool_set_sp_schedule"]) == 6 and params["mj_last_error"] == []
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
    assert L.mj_abi_version() == 1
    assert [L.mj_obs_rows(v) for v in (1, 2, 3, 4)] == [938, 942, 934, 1012]


def test_libriichi_surface():
    import libriichi
    from libriichi import consts
    from libriichi.consts import ACTION_SPACE, GRP_SIZE, MAX_VERSION, obs_shape, oracle_obs_shape

    assert (ACTION_SPACE, GRP_SIZE, MAX_VERSION) == (46, 7, 4)
    assert obs_shape(4) == (1012, 34) and obs_shape(1) == (938, 34) and oracle_obs_shape(3) == (217, 34)
    assert libriichi.__profile__ and libriichi.__version__ and consts is libriichi.consts
    from libriichi.arena import OneVsThree, TwoVsTwo

    env = OneVsThree(disable_progress_bar=True, log_dir=None)
    assert hasattr(env, "py_vs_py") and hasattr(TwoVsTwo(), "py_vs_py")
    with pytest.raises(TypeError):
        OneVsThree(True)  # keyword-only like the pyo3 signature (one_vs_three.rs:27)
    assert hasattr(libriichi.stat.Stat, "from_dir") and hasattr(libriichi.stat.Stat, "avg_pt")
    assert hasattr(libriichi.dataset.GameplayLoader, "load_gz_log_files") and hasattr(libriichi.dataset.Grp, "load_log")
    assert "oracle: true" in repr(libriichi.dataset.GameplayLoader(4)).lower()  # oracle=True is the reference's default
    assert hasattr(libriichi.mjai.Bot, "react")


def test_stack_proxy_is_zero_copy():
    """np.stack([proxy], axis=0) must hand back the very tensor (mortal/engine.py:54 path)."""
    import torch

    from mortal_amd.arena import _StackedBatch

    t = torch.zeros((5, 7, 34))
    out = np.stack([_StackedBatch(t)], axis=0)
    assert out is t
    assert torch.as_tensor(out, device=torch.device("cpu")) is t


def test_rank_and_seat_plan():
    from mortal_amd.arena import _rank_by_player

    assert _rank_by_player([25000, 25000, 30000, 20000]) == [1, 2, 0, 3]  # rankings.rs:29-65: ties -> lower seat first
    assert _rank_by_player([25000] * 4) == [0, 1, 2, 3]
    # challenger seat of game g is g % 4; mask bit s = 1 -> champion
    aos = [0xF & ~(1 << (g % 4)) for g in range(8)]
    assert aos[:4] == [0b1110, 0b1101, 0b1011, 0b0111]


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    import importlib

    import mortal_amd._lib as L

    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(L.MortalAmdError):
        L._load()
    importlib.reload(L)


def test_rankings_reference_vectors():
    """rankings.rs:29-65: the five vectors of the reference's own test, applied to every host-side ranking in the product
    (arena rank histogram, Stat, Grp) — stable sort by descending score, ties to the lower seat."""
    from mortal_amd.arena import _rank_by_player

    vectors = [([25000, 25000, 30000, 20000], [1, 2, 0, 3]), ([25000, 25000, 25000, 25000], [0, 1, 2, 3]),
               ([18000, 32000, 32000, 18000], [2, 0, 1, 3]), ([32000, 18000, 18000, 32000], [0, 2, 3, 1]),
               ([0, 100000, 0, 0], [1, 0, 2, 3])]
    from mortal_amd.dataset import Grp
    from mortal_amd.stat import Stat

    for scores, rank_by_player in vectors:
        assert _rank_by_player(scores) == rank_by_player
        ev = [{"type": "start_game", "names": list("abcd")},
              {"type": "start_kyoku", "bakaze": "E", "dora_marker": "1m", "kyoku": 1, "honba": 0, "kyotaku": 0, "oya": 0,
               "scores": scores, "tehais": [["?"] * 13] * 4},
              {"type": "ryukyoku", "deltas": [0, 0, 0, 0]}, {"type": "end_kyoku"}, {"type": "end_game"}]
        assert Grp.load_events(ev).rank_by_player == rank_by_player
        for p in range(4):
            st = Stat.from_game(ev, p)
            assert [st.rank_1, st.rank_2, st.rank_3, st.rank_4].index(1) == rank_by_player[p]


def test_device_helpers_host_equivalence(tmp_path):
    """The optimised pure helpers of mj_algo.h (static-index sh_final) against their reference-shaped formulations, compiled
    for the host by hipcc (tests/host/algo_check.hip; no GPU involved)."""
    import shutil
    import subprocess

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        import pytest

        pytest.skip("hipcc not available")
    exe = str(tmp_path / "algo_check")
    src = os.path.join(os.path.dirname(__file__), "host", "algo_check.hip")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wno-unused-value", "-o", exe, src],
                          stderr=subprocess.DEVNULL)
    from mortal_amd import tables

    payload = tmp_path / "mjtables.bin"
    payload.write_bytes(tables.payload())
    out = subprocess.run([exe, str(payload)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sh_final == reference-shaped loop" in out.stdout
    assert "draw candidates cover every shanten-lowering draw" in out.stdout  # the SP kernel's pruned "+t" probe set


# mj_k_sp as compiled in round 6 (hipcc of ROCm 7.2.0); lower them when the kernel improves, never raise them unmeasured
# (round 5: 28 / 218 / 464 at 13.7-13.8 ms; round 6: the kernel body became a template shared with mj_k_sp_promo / mj_k_sp_wide -- the same
# code for this instantiation, the allocator lands on 33-36 / 221-226 / 480, measured 13.75-13.79 ms at 65,536 tables on a box where the build WITH
# the parking code compiled in (53 VGPR spills) took 14.12-14.17: that one stays out of mj_k_sp, see mj_k_sp_promo; with the tuned LDS
# team strides, no calls for idle wavefronts and one scoring call per wavefront the report is 34 / 217 / 512 -- the 512 bytes are the
# deepest callee's frame -- and the kernel measured 13.77-13.80 ms against 13.88-13.93 for the build before, interleaved in one call)
SP_MAX_VGPR_SPILLS, SP_MAX_SGPR_SPILLS, SP_MAX_SCRATCH_BYTES = 36, 226, 512


def test_sp_kernel_isa_has_no_flat_or_spilled_hot_paths(tmp_path):
    """Static ISA review of the SP kernel's phase functions (cross-compiled, no GPU): every memory access has a known
    address space (no flat_* instruction: a flat load counts on both wait counters and serialises LDS reads behind HBM
    gathers), the dense passes and the evaluation teams do not spill, and the kernel keeps its 4-workgroups-per-CU budget
    (<= 128 VGPRs, <= 40 KB LDS)."""
    import shutil
    import subprocess

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    asm = str(tmp_path / "lib.s")
    cc = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value",
                         "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", asm,
                         os.path.join(root, "mortal_amd", "csrc", "mj_capi.hip")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    text = open(asm).read()
    # the compiler's own resource report of the kernel (the round's largest step was a register-allocation artefact
    # found by search; pin what it left so that an edit to the 19 k-instruction loop body cannot lose it silently)
    rep = cc.stderr[cc.stderr.index("Function Name: _Z7mj_k_sp8SpParams"):]
    rep = rep[: rep.index("LDS Size") + 200]
    usage = {k: int(v) for k, v in re.findall(r"remark:\s+(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|VGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", rep)}
    print("mj_k_sp resource usage:", usage)
    assert usage["Occupancy [waves/SIMD]"] == 4 and usage["VGPRs"] <= 128, usage
    assert usage["VGPRs Spill"] <= SP_MAX_VGPR_SPILLS and usage["SGPRs Spill"] <= SP_MAX_SGPR_SPILLS, usage
    assert usage["ScratchSize [bytes/lane]"] <= SP_MAX_SCRATCH_BYTES, usage
    assert usage["LDS Size [bytes/block]"] * 4 <= 160 * 1024, usage  # four workgroups per CU
    funcs = {}
    for m in re.finditer(r"^(_Z\d+(?:sp_\w+|mj_k_sp\w*)):.*?^\.Lfunc_end\d+:", text, re.S | re.M):
        funcs[m.group(1)] = m.group(0)
    names = " ".join(funcs)
    for want in ("sp_l0_probe_chunk", "sp_l0_score", "sp_eval_wave0ILi8E", "sp_eval_waveILi16ELi1E", "sp_eval_waveILi17ELi2E", "mj_k_sp"):
        assert want in names, (want, sorted(funcs))
    for name, body in funcs.items():
        assert "flat_" not in body, name
        if "sp_eval_wave" in name or "chunk" in name:
            # scratch traffic only as callee-saved register saves / restores in the prologue and epilogue (once per call:
            # a call evaluates a team's whole share of a level), never inside the loops
            lines = body.split("\n")
            where = [i for i, ln in enumerate(lines) if "scratch_" in ln]
            assert all(i < 60 or i > len(lines) - 100 for i in where), (name, where[:8], len(lines))
    # the expansion is inlined into the kernel (a call per 16-state chunk cost 74 scratch operations of callee-saved registers);
    # the kernel's own spills stay few: the lane-derived constants are recomputed, not hoisted and spilled (SP_OPAQUE_TID)
    assert not any("sp_expand_chunk" in n for n in funcs), sorted(funcs)
    kern = funcs["_Z7mj_k_sp8SpParams"]
    assert kern.count("scratch_") <= 80, kern.count("scratch_")
    k = re.search(r"\.amdhsa_kernel _Z7mj_k_sp8SpParams(.*?)\.end_amdhsa_kernel", text, re.S).group(1)
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", k).group(1)) <= 512
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", k).group(1)) <= 128
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", k).group(1)) <= 40960
