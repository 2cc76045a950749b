"""Static ISA review of the expansion's insert pass in mj_k_sp (cross-compiled, no GPU).  P4 of sp_expand_chunk runs as straight-line
stages behind wavefront-uniform tests; as per-lane control flow (decode, look, claim, probe and list with their early returns, inlined
once per entry) more than half of its instructions kept exec masks.  The pass is isolated by source-line attribution, as
tools/isa_phases.py does it: the kernel is compiled with line tables, and the pass is the span of mj_k_sp's instruction stream from the
first to the last instruction attributed to the source lines of P4 (the helpers inlined into it lie inside that span).  The same span
of the commit before the stages (b810d16, compiled here from git history) is the yardstick:

  exec-mask saves (s_*_saveexec_b64) at most half the parent's -- the staged form needs a few tens; half only fails if the compiler
      nests the stages again;
  fewer instructions than the parent's span;
  no scratch_ and no flat_ instruction in the span."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = "b810d16"  # the commit before the stages
# its span as compiled by ROCm 7.2.0's hipcc: used only where the history is not at hand (an exported tree)
PARENT_COUNTS = {"total": 1990, "saveexec": 216, "cbranch_exec": 161, "valu": 843, "salu": 762, "waitcnt": 72, "ds_cmpst": 8}
KERNEL = "_Z7mj_k_sp8SpParams"
FIRST, LAST = "// P4: children, one lane per CHILD ENTRY", "tp4 = wall_clock64();"  # the source lines that bound the pass


def _p4_lines(csrc):
    lines = open(os.path.join(csrc, "mj_sp.hip")).read().split("\n")
    first = next(i for i, ln in enumerate(lines) if FIRST in ln) + 1
    last = next(i for i, ln in enumerate(lines) if i >= first and LAST in ln)  # (1-based: the line before the timer)
    assert first < last, (first, last)
    return first, last


def insert_pass_counts(csrc, out_dir):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    asm = os.path.join(out_dir, "lib.s")
    cc = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value",
                         "--cuda-device-only", "-S", "-gline-tables-only", "-o", asm, os.path.join(csrc, "mj_capi.hip")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    text = open(asm).read()
    files = {int(m.group(1)): m.group(2).split("/")[-1] for m in re.finditer(r'\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', text)}
    first, last = _p4_lines(csrc)
    body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % KERNEL, text, re.S | re.M).group(0).split("\n")
    ins, inside = [], False
    for ln in body:
        s = ln.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            inside = files.get(int(m.group(1))) == "mj_sp.hip" and first <= int(m.group(2)) <= last
            continue
        if not s or s[0] in ".;" or s.endswith(":"):
            continue
        ins.append((s.split()[0], inside))
    idx = [i for i, (_, own) in enumerate(ins) if own]
    assert idx, "no instruction of mj_k_sp is attributed to the insert pass"
    c = collections.Counter()
    for op, _ in ins[idx[0]:idx[-1] + 1]:
        c["total"] += 1
        c["valu"] += op.startswith("v_")
        c["salu"] += op.startswith("s_") and not op.startswith(("s_waitcnt", "s_cbranch", "s_branch", "s_nop"))
        c["saveexec"] += bool(re.match(r"s_\w+_saveexec_b64", op))
        c["cbranch_exec"] += op.startswith("s_cbranch_exec")
        c["waitcnt"] += op.startswith("s_waitcnt")
        c["scratch"] += op.startswith("scratch_")
        c["flat"] += op.startswith("flat_")
        c["ds_cmpst"] += op.startswith("ds_cmpst_rtn_b64")
    return dict(c)


@pytest.fixture(scope="module")
def new_counts(tmp_path_factory):
    return insert_pass_counts(os.path.join(ROOT, "mortal_amd", "csrc"), str(tmp_path_factory.mktemp("sp_insert_isa")))


@pytest.fixture(scope="module")
def parent_counts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sp_insert_isa_parent")
    src = tmp / "mortal_amd" / "csrc"
    src.mkdir(parents=True)
    (tmp / "include").mkdir()
    try:
        names = subprocess.run(["git", "-C", ROOT, "ls-tree", "--name-only", f"{PARENT}:mortal_amd/csrc"], capture_output=True, text=True,
                               timeout=60)
        if names.returncode != 0 or not names.stdout.split():
            raise OSError(names.stderr)
        for name in names.stdout.split():
            (src / name).write_bytes(subprocess.run(["git", "-C", ROOT, "show", f"{PARENT}:mortal_amd/csrc/{name}"], capture_output=True,
                                                    check=True, timeout=60).stdout)
        (tmp / "include" / "mortal_amd.h").write_bytes(subprocess.run(["git", "-C", ROOT, "show", f"{PARENT}:include/mortal_amd.h"],
                                                                      capture_output=True, check=True, timeout=60).stdout)
    except (OSError, subprocess.SubprocessError) as e:
        print(f"no git history of {PARENT} here ({str(e)[:100]}): the recorded counts stand in")
        return dict(PARENT_COUNTS)
    return insert_pass_counts(str(src), str(tmp))


def test_insert_pass_is_staged(new_counts, parent_counts):
    print("insert pass of mj_k_sp, new:   ", new_counts)
    print("insert pass of mj_k_sp, parent:", parent_counts)
    assert new_counts["ds_cmpst"] >= 1 and parent_counts.get("ds_cmpst", 1) >= 1  # the spans hold the expansion's compare-and-swaps
    assert 2 * new_counts["saveexec"] <= parent_counts["saveexec"], (new_counts["saveexec"], parent_counts["saveexec"])
    assert new_counts["total"] < parent_counts["total"], (new_counts["total"], parent_counts["total"])
    assert new_counts["scratch"] == 0 and new_counts["flat"] == 0, new_counts
