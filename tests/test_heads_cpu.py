"""Multi-head weighted SpMM and SDDMM without a GPU: the register budgets of their translation units (cross-compiled for
gfx950) and the argument checks hcspmm_forward_weighted_heads / hcspmm_sddmm_heads make before they touch HIP."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from hcspmm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hc-spmm_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (scratch bytes per lane, waves per SIMD) of every build, by kernel; the same for every L
BUDGETS = {
    "hybrid_plan_wh_kernel": (0, 5),
    "tiny_wh_kernel": (0, 8),
    "hybrid_window_wh_kernel": (0, 4),
    "sddmm_heads_kernel": (0, 5),
    "fixup_kernel": (0, 7),  # (the binary fix-up pass, instantiated here for the split rows)
}


def _usage(src):
    cmd = [HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", os.devnull]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-2000:]
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("src,n_builds", [("spmm_weighted_heads.hip", 16), ("sddmm_heads.hip", 7)])
def test_heads_kernels_keep_their_budgets(src, n_builds):
    """fp32, 16-byte lanes, L = 4 ... 64 (sddmm: 1 ... 64): no scratch anywhere (the weighted builds they mirror allow up to
    36 B at L = 32), occupancy as pinned above"""
    usage = _usage(src)
    assert len(usage) == n_builds, sorted(usage)
    for name, v in usage.items():
        kernel = next((k for k in BUDGETS if k in name), None)
        assert kernel is not None, name
        assert (v["scratch"], v["occupancy"]) == BUDGETS[kernel], (name, v)


def _vp(v):
    return ctypes.c_void_p(0x1000 if v else 0)  # never dereferenced: every case fails before HIP is touched


def _fw(X=1, Z=1, dtype=0, rp=1, col=1, bp=1, e2c=1, e2r=1, ht=1, N=64, E=100,
        D=32, ldx=None, ldz=None, values=1, heads=4):
    return capi.lib().hcspmm_forward_weighted_heads(_vp(X), N, ldx or D, _vp(Z), ldz or D, dtype, _vp(rp), _vp(col), _vp(bp),
                                                    _vp(e2c), _vp(e2r), _vp(ht), ctypes.c_void_p(0), None, N, E, D,
                                                    ctypes.c_void_p(0), 0, ctypes.c_void_p(0), _vp(values), heads)


def _sd(A=1, B=1, dtype=0, out=1, rp=1, col=1, N=64, E=100, D=32, lda=None, ldb=None, b_rows=64, heads=4):
    return capi.lib().hcspmm_sddmm_heads(_vp(A), lda or D, _vp(B), b_rows, ldb or D, dtype, _vp(out), _vp(rp), _vp(col),
                                         ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), heads)


# heads <= 0, D % heads != 0, Dh % 4 != 0, 16-bit features (HCSPMM_DTYPE_F16 = 1, BF16 = 2)
BAD_HEADS = [dict(heads=0), dict(heads=-2), dict(D=30, heads=4), dict(D=30, heads=3), dict(D=24, heads=4), dict(D=12, heads=2),
             dict(D=2, heads=1), dict(D=36, heads=6), dict(dtype=1), dict(dtype=2)]


@pytest.mark.parametrize("case", BAD_HEADS + [dict(values=0), dict(X=0), dict(Z=0), dict(rp=0), dict(D=0), dict(N=-1),
                                              dict(E=-1), dict(ldx=16), dict(dtype=7)])
def test_forward_weighted_heads_argument_checks(case):
    assert _fw(**case) == capi.EINVAL


@pytest.mark.parametrize("case", BAD_HEADS + [dict(A=0), dict(B=0), dict(out=0), dict(rp=0), dict(col=0), dict(N=-1), dict(E=-1),
                                              dict(b_rows=-1), dict(lda=16), dict(ldb=16), dict(dtype=7)])
def test_sddmm_heads_argument_checks(case):
    assert _sd(**case) == capi.EINVAL


def test_nothing_to_do_launches_nothing():
    assert _fw(N=0) == 0  # as hcspmm_forward_weighted: no rows, no launch
    assert _sd(A=0, B=0, out=0, col=0, E=0) == 0
