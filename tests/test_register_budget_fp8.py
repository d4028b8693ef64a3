"""Register budget of the 8-bit (e4m3fn) SpMM kernels, by the method of test_register_budget.py: the
compiler's own resource report of the two new translation units, cross-compiled for gfx950.  The bar is the 16-bit builds':
every planned build keeps four waves per SIMD and spills nothing."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hc-spmm_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
UNITS = ("spmm_kernels_f8.hip", "spmm_weighted_f8.hip")


def _resource_usage(unit):
    cmd = [HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, unit), "-o", os.devnull]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-2000:]
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"\bAGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


@pytest.fixture(scope="module")
def usage():
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(2) as ex:
        return dict(zip(UNITS, ex.map(_resource_usage, UNITS)))


def _lv(name, kernel):
    """kernel<F8, L, VEC, ...> -> (L, VEC) from the mangled name"""
    m = re.search(kernel + r"INS_2F8ELi(\d+)ELi(\d+)E", name)
    return (int(m.group(1)), int(m.group(2))) if m else None


# 8 codes per lane (D >= 32) and 4, L = 4 ... 64 lanes per task
BUILDS = {(L, V) for L in (4, 8, 16, 32, 64) for V in (4, 8)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("unit,plan,tiny,window", [
    ("spmm_kernels_f8.hip", "hybrid_plan_kernel", "tiny_kernel", "hybrid_window_kernel"),
    ("spmm_weighted_f8.hip", "hybrid_plan_w_kernel", "tiny_w_kernel", "hybrid_window_w_kernel")])
def test_fp8_planned_kernels_keep_four_waves_and_do_not_spill(usage, unit, plan, tiny, window):
    u = usage[unit]
    for n in u:  # nothing but 8-bit instantiations in these units
        assert "2F8E" in n, n
    planned = {_lv(n, plan): v for n, v in u.items() if _lv(n, plan)}
    assert set(planned) == BUILDS, sorted(planned)
    for a, v in planned.items():
        assert v["occupancy"] >= 4 and v["scratch"] == 0, (unit, a, v)
    # the tiny tasks' own launch and the fix-up pass belong to the planned launch
    own_tiny = {_lv(n, tiny): v for n, v in u.items() if _lv(n, tiny)}
    assert set(own_tiny) == BUILDS, sorted(own_tiny)
    for a, v in own_tiny.items():
        assert v["occupancy"] >= 4 and v["scratch"] == 0, (unit, a, v)
    fixups = {n: v for n, v in u.items() if "fixup_kernel" in n}
    assert len(fixups) == 2
    for n, v in fixups.items():
        assert v["occupancy"] >= 4 and v["scratch"] == 0, (n, v)
    # plan-free kernels: never spill (three waves per SIMD at 8 codes per lane, like the 16-bit weighted builds)
    plan_free = {_lv(n, window): v for n, v in u.items() if _lv(n, window)}
    assert set(plan_free) == BUILDS, sorted(plan_free)
    for a, v in plan_free.items():
        assert v["scratch"] == 0 and v["occupancy"] >= 3, (unit, a, v)
    assert len(u) == 3 * len(BUILDS) + 2, sorted(u)


def test_fp8_builds_stay_out_of_the_pinned_units():
    """test_register_budget.py counts the instantiations of the fp32 / 16-bit units: no 8-bit build goes into them"""
    for unit in ("spmm_kernels.hip", "spmm_kernels_h16.hip", "spmm_weighted.hip", "spmm_weighted_h16.hip",
                 "spmm_weighted_heads.hip", "spmm_weighted_indexed.hip", "spmm_extremum.hip", "fused_rows.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "F8" not in text, unit
