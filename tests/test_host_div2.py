"""CPU-only: the two-wide division of the SP kernel's sums (mj_algo.h: sp_div_domain2) against the one-wide sp_div_domain, bit for bit in
both components over the kernel's whole operand domain (tests/host/div2_check.hip, a stand-alone host program) -- built plain and with
the host sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_div_domain2_equals_div_domain_on_the_whole_domain(tmp_path, sanitize):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "div2_check")
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *flags, "-std=c++17", "-ffp-contract=off", "-Wno-unused-value", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "div2_check.hip")], stderr=subprocess.DEVNULL)
    if sanitize:  # the runtime is linked into the program itself
        assert b"__asan_init" in subprocess.run(["nm", "-D", exe], capture_output=True).stdout + subprocess.run(["nm", exe], capture_output=True).stdout
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sp_div_domain2 == sp_div_domain in both components on 4331124 operand pairs" in out.stdout
