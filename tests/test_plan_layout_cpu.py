"""plan_launch_layout (hc-spmm_amd/csrc/plan_layout.h), the one place where the grid of the planned hybrid launch is laid
out for the binary, weighted, multi-head (direct and indexed) and extremum launchers: tests/capi/plan_layout_check.cpp
sweeps small plans on the host and asserts the invariants their device decodes rely on.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hc-spmm_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_plan_launch_layout_invariants(tmp_path):
    exe = str(tmp_path / "plan_layout_check")
    # a .cpp: host code only (the header needs HIP's headers for the argument structs, no device compilation)
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "capi", "plan_layout_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "plan_layout ok" in r.stdout, r.stdout[-2000:]
