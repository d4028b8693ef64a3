"""SDDMM and edge softmax without a GPU: the register budgets of their translation unit (cross-compiled for gfx950), the
argument checks hcspmm_sddmm / hcspmm_edge_softmax* make before they touch HIP, and the driver's GAT flags."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest

from hcspmm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hc-spmm_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def usage():
    cmd = [HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "sddmm.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-2000:]
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_sddmm_kernels_keep_their_budgets(usage):
    """SDDMM: 9 fp32 builds (L = 1 ... 64 with 16-byte lanes, the 8-byte and single-element builds of D <= 3) and 21 per
    16-bit type (L = 1 ... 64 for 16-, 8- and 2-byte lanes); nothing spilled, at least six waves per SIMD (the L = 64
    16-byte 16-bit builds; the rest seven or eight) -- DESIGN.md section 3.9.  Edge softmax: seven (forward) and eight
    (backward) waves, nothing spilled."""
    sd = {n: v for n, v in usage.items() if "sddmm_kernel" in n}
    assert len(sd) == 9 + 21 + 21, sorted(usage)
    for n, v in sd.items():
        assert v["scratch"] == 0 and v["occupancy"] >= 6 and v["vgprs"] <= 80, (n, v)
        if "ELi64ELi8E" not in n:
            assert v["occupancy"] >= 7, (n, v)
    sm = {n: v for n, v in usage.items() if "edge_softmax_kernel" in n}
    assert len(sm) == 2
    for n, v in sm.items():
        assert v["scratch"] == 0 and v["occupancy"] >= (8 if "ILb1E" in n else 7), (n, v)


def _sd(A=1, B=1, out=1, rp=1, col=1, lda=16, ldb=16, b_rows=32, dtype=0, N=16, E=8, D=16, plan=0):
    vp = lambda v: ctypes.c_void_p(0x1000 if v else 0)  # never dereferenced: every case fails before HIP is touched
    return capi.lib().hcspmm_sddmm(vp(A), lda, vp(B), b_rows, ldb, dtype, vp(out), vp(rp), vp(col), vp(plan), None, N, E, D,
                                   ctypes.c_void_p(0))


@pytest.mark.parametrize("case", [dict(A=0), dict(B=0), dict(out=0), dict(rp=0), dict(col=0), dict(D=0), dict(D=-3),
                                  dict(lda=15), dict(ldb=8), dict(dtype=3), dict(dtype=-1), dict(N=-1), dict(E=-1),
                                  dict(b_rows=-1), dict(N=0), dict(plan=1)])
def test_sddmm_argument_checks(case):
    assert _sd(**case) == capi.EINVAL


def test_sddmm_without_entries_launches_nothing():
    assert _sd(A=0, B=0, out=0, col=0, E=0) == 0


def _sm(x=1, y=1, out=1, rp=1, N=16, E=8, heads=1, backward=False):
    vp = lambda v: ctypes.c_void_p(0x1000 if v else 0)
    L = capi.lib()
    if backward:
        return L.hcspmm_edge_softmax_backward(vp(x), vp(y), vp(out), vp(rp), N, E, heads, ctypes.c_void_p(0))
    return L.hcspmm_edge_softmax(vp(x), vp(out), vp(rp), N, E, heads, ctypes.c_void_p(0))


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("case", [dict(x=0), dict(out=0), dict(rp=0), dict(heads=0), dict(heads=-2), dict(N=-1), dict(E=-1),
                                  dict(N=0)])
def test_edge_softmax_argument_checks(case, backward):
    assert _sm(backward=backward, **case) == capi.EINVAL


def test_edge_softmax_backward_needs_grad_alpha():
    assert _sm(y=0, backward=True) == capi.EINVAL


def test_driver_refuses_norm_with_gat():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_gat_cpu", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(["--model", "gat", "--heads", "3"])
    assert args.model == "gat" and args.heads == 3 and args.norm == "none"
    assert mod.parse_args([]).heads == 1
    for bad in (["--model", "gat", "--norm", "sym"], ["--model", "gat", "--norm", "mean"], ["--model", "gat", "--heads", "0"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
