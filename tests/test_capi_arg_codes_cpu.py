"""Return codes of the planned entry points of the C ABI for failing arguments, and which defect wins when two are present:
tests/capi/arg_codes.cpp calls them from a main of its own with every single defect and every pair out of a list, with a
plan and plan-free, and prints the codes; they must equal tests/golden/capi_arg_codes.txt, recorded from the library before
the entry points shared one binder.  Every call returns before a launch, so no GPU is needed (and none is shown to it)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hc-spmm_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_argument_error_codes_and_precedence(tmp_path):
    assert os.path.exists(os.path.join(CSRC, "libhcspmm.so")), "libhcspmm.so is not built"
    exe = str(tmp_path / "arg_codes")
    # a .cpp: host code only
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "capi", "arg_codes.cpp"), "-L", CSRC, "-lhcspmm", "-Wl,-rpath," + CSRC,
                           "-o", exe])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    with open(os.path.join(ROOT, "tests", "golden", "capi_arg_codes.txt")) as f:
        want = f.read().splitlines()
    assert len(got) == len(want) and len(got) > 1000
    differ = [(g, w) for g, w in zip(got, want) if g != w]
    assert not differ, "%d argument sets return other codes, e.g. got / want:\n%s\n%s" % (len(differ), differ[0][0], differ[0][1])
    # the sweep reaches every code an argument can earn: OK (N = 0), EINVAL, EPLAN, EWORKSPACE, ERANGE -- and never a launch (EHIP)
    codes = {c for line in got for c in line.rsplit("|", 1)[1].split()}
    assert codes == {"0", "-1", "-3", "-5", "-6"}, codes
