"""Static ISA review of the SP kernel's level-0 scoring pass (cross-compiled, no GPU).  sp_l0_score_all is called once per wavefront and
row; its item loop scores one (tenpai state, winning tile, red / plain variant) per lane and iteration.  The loop used to build an AgariIn
on the stack, call the out-of-line agari_full through a pointer to it and let the callee read it back, save its registers and index its
tile list in scratch memory -- once per item, with the scratch of 1,024 workgroups not staying in L2.  Now the agari code is inlined
(mj_algo.h: agari_full_inl, Tile14::at<true>) and the row's constants sit in scalar registers, so between the loop header and the
epilogue there must be neither a scratch access nor a call, and the function's frame holds its callee-saved registers and little else."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def score_fn(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    asm = str(tmp_path_factory.mktemp("sp_score_isa") / "lib.s")
    cc = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value",
                         "--cuda-device-only", "-S", "-o", asm, os.path.join(ROOT, "mortal_amd", "csrc", "mj_capi.hip")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    text = open(asm).read()
    found = [m for m in re.finditer(r"^(_Z\d+\w+):.*?^\.Lfunc_end\d+:", text, re.S | re.M) if "sp_l0_score_all" in m.group(1)]
    assert len(found) == 1, [m.group(1) for m in found]  # one out-of-line function shared by mj_k_sp, mj_k_sp_promo and mj_k_sp_wide
    name, lines = found[0].group(1), found[0].group(0).split("\n")
    frame = int(re.search(r"^\s*\.set \.L%s\.private_seg_size, (\d+)" % re.escape(name), text, re.M).group(1))
    return name, lines, frame


def _loop_region(lines):
    """Line indices [first loop header, last line of any loop): everything behind it is the way out and the epilogue."""
    in_loop = [i for i, ln in enumerate(lines) if "Loop Header" in ln or "in Loop:" in ln or "Parent Loop" in ln]
    assert in_loop, "the item loop is gone"
    first = in_loop[0]
    last = in_loop[-1]
    while last + 1 < len(lines) and not re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", lines[last + 1]):  # to the end of that loop's last block
        last += 1
    return first, last + 1


def test_scoring_loop_touches_no_scratch_and_makes_no_call(score_fn):
    name, lines, _ = score_fn
    first, end = _loop_region(lines)
    body = lines[first:end]
    assert len(body) > 1000, (name, first, end)  # the inlined agari code is in there, not behind a call
    assert [ln for ln in body if "scratch_" in ln] == []
    assert [ln for ln in body if "s_swappc_b64" in ln] == []
    # the whole function: no call at all (full inlining), no access through a pointer of unknown address space
    assert not any("s_swappc_b64" in ln or "flat_" in ln for ln in lines)
    # ... and what scratch traffic there is saves and restores callee-saved registers, ahead of the loop and behind it
    where = [i for i, ln in enumerate(lines) if "scratch_" in ln]
    assert all(i < first or i >= end for i in where)
    assert all("Folded Spill" in lines[i] or "Folded Reload" in lines[i] for i in where), [lines[i] for i in where][:8]


def test_scoring_function_frame_is_its_register_saves(score_fn):
    name, lines, frame = score_fn
    first, _ = _loop_region(lines)
    saves = sum(4 * int(m.group(1) or 1) for m in
                (re.search(r"scratch_store_dword(?:x(\d))? .*Folded Spill", ln) for ln in lines[:first]) if m)
    print(f"{name}: frame {frame} B, callee-saved register saves {saves} B")
    assert frame - saves <= 64, (frame, saves)
    assert frame <= 256  # (it was 256 B + the 64 B of agari_full and agari_search below it)
