"""Static ISA review of the SP kernel's triangular sums (cross-compiled, no GPU).  sp_eval_wave / sp_eval_wave0 add their terms in groups
of four behind one scalar branch; a group's basic block holds the LDS reads of its rows and numerators, the divisions and the sums.
The divisions run two at a time (mj_algo.h: sp_div_domain2 -> v_pk_mul_f32 + 2 v_pk_fma_f32 per pair) and the parked rows are laid out
so that the numerators of two consecutive terms and a row's (win, EV) values each arrive in an aligned register pair: no v_mov_b32
assembles an operand.  The count of the group's VALU instructions is set against the same block of the commit this layout replaced
(558a029, where the compiler's own pairing of the scalar code needed ten moves per group at level 1), compiled here from git history."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = "558a029"         # the commit before the packed sums
PARENT_GROUP_VALU = 30     # its count as compiled by ROCm 7.2.0's hipcc: used only where the history is not at hand (an exported tree)
WAVE1, WAVE0 = "sp_eval_waveILi17ELi1E", "sp_eval_wave0ILi17E"


def _functions(csrc, out_dir):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    asm = os.path.join(out_dir, "lib.s")
    cc = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value",
                         "--cuda-device-only", "-S", "-o", asm, os.path.join(csrc, "mj_capi.hip")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    text = open(asm).read()
    return {m.group(1): m.group(0).split("\n") for m in re.finditer(r"^(_Z\d+sp_eval_wave\w+):.*?^\.Lfunc_end\d+:", text, re.S | re.M)}


def _fn(funcs, part):
    found = [n for n in funcs if part in n]
    assert len(found) == 1, (part, sorted(funcs))
    return funcs[found[0]]


def group_blocks(lines):
    """The basic blocks that read LDS and make four divisions (eight fmas, packed or not): one per group of four terms."""
    blocks, cur = [], []
    for ln in lines:
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", ln):
            blocks.append(cur)
            cur = []
        cur.append(ln)
    blocks.append(cur)
    def fmas(b):
        return sum(2 if "v_pk_fma_f32" in ln else 1 for ln in b if re.search(r"^\s+v_(pk_)?fma(c)?_f32", ln))
    return [b for b in blocks if any("ds_read" in ln for ln in b) and fmas(b) >= 8]


def valu(block):
    return [ln.split()[0] for ln in block if re.match(r"^\s+v_", ln)]


@pytest.fixture(scope="module")
def new_funcs(tmp_path_factory):
    return _functions(os.path.join(ROOT, "mortal_amd", "csrc"), str(tmp_path_factory.mktemp("sp_eval_isa")))


@pytest.fixture(scope="module")
def parent_group_valu(tmp_path_factory):
    """VALU instructions of the first group's block of sp_eval_wave<17, 1> at PARENT, from its own sources where git has them."""
    tmp = tmp_path_factory.mktemp("sp_eval_isa_parent")
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
        print(f"no git history of {PARENT} here ({str(e)[:100]}): the recorded count {PARENT_GROUP_VALU} stands in")
        return PARENT_GROUP_VALU
    return len(valu(group_blocks(_fn(_functions(str(src), str(tmp)), WAVE1))[0]))


def test_divisions_are_packed(new_funcs):
    for part in (WAVE1, WAVE0, "sp_eval_waveILi17ELi2E", "sp_eval_waveILi8ELi1E", "sp_eval_wave0ILi8E"):
        lines = _fn(new_funcs, part)
        groups = group_blocks(lines)
        assert groups and any("v_pk_fma_f32" in ln for ln in lines), part
        for b in groups:
            ops = valu(b)
            # a pair of divisions = one packed multiply + two packed fmas; no plain fma is left in a group of four
            if len([o for o in ops if o.startswith("v_pk_fma_f32")]) >= 4:
                assert not [o for o in ops if re.match(r"v_fma(c)?_f32", o)], (part, ops)


def test_level1_group_needs_no_moves_and_fewer_instructions(new_funcs, parent_group_valu):
    groups = group_blocks(_fn(new_funcs, WAVE1))
    assert len(groups) == 5  # 17 turns: five groups of four
    counts = [len(valu(b)) for b in groups]
    print(f"sp_eval_wave<17, 1>: VALU instructions per four-term group {counts}, parent {parent_group_valu}")
    for b in groups:
        ops = valu(b)
        assert not [o for o in ops if o.startswith("v_mov_b32")], ops
        assert len(ops) <= 0.8 * parent_group_valu, (len(ops), parent_group_valu)
        assert len([ln for ln in b if "ds_read" in ln]) <= 4  # (no more LDS instructions than the four ds_read_b128 of the 16-byte rows)
