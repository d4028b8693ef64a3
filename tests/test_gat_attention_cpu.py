"""GAT attention without a GPU: the register budgets of its translation unit (cross-compiled for gfx950) and the argument
checks hcspmm_gat_attention / hcspmm_gat_attention_backward make before they touch HIP."""
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

# waves per SIMD of every kernel build, by head-group size
OCCUPANCY = {
    "gat_attention_kernel": {1: 8, 2: 8, 3: 6, 4: 5},
    "gat_attention_rows_kernel": {1: 8, 2: 7, 3: 5, 4: 3},
    "gat_attention_cols_kernel": {1: 8, 2: 8, 3: 8, 4: 8},
}


@pytest.fixture(scope="module")
def usage():
    cmd = [HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "gat_attention.hip"), "-o", os.devnull]
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
def test_gat_kernels_keep_their_budgets(usage):
    """12 builds (3 kernels x head groups of 1-4): nothing spilled, occupancy as pinned above"""
    assert len(usage) == 12, sorted(usage)
    for name, v in usage.items():
        m = re.search(r"(gat_attention(?:_rows|_cols)?_kernel)ILi(\d)E", name)
        assert m, name
        assert v["scratch"] == 0, (name, v)
        assert v["occupancy"] == OCCUPANCY[m.group(1)][int(m.group(2))], (name, v)


def _vp(v):
    return ctypes.c_void_p(0x1000 if v else 0)  # never dereferenced: every case fails before HIP is touched


def _fwd(s_dst=1, s_src=1, src_rows=32, slope=0.2, alpha=1, rp=1, col=1, N=16, E=8, heads=2):
    return capi.lib().hcspmm_gat_attention(_vp(s_dst), _vp(s_src), src_rows, slope, _vp(alpha), _vp(rp), _vp(col), N, E, heads,
                                           ctypes.c_void_p(0))


def _bwd(alpha=1, ga=1, s_dst=1, s_src=1, slope=0.2, rp=1, col=1, perm=1, N=16, E=8, heads=2, out=1, gd=1, gs=1):
    return capi.lib().hcspmm_gat_attention_backward(_vp(alpha), _vp(ga), _vp(s_dst), _vp(s_src), slope, _vp(rp), _vp(col),
                                                    _vp(perm), N, E, heads, _vp(out), _vp(gd), _vp(gs), ctypes.c_void_p(0))


BAD_SLOPES = [float("nan"), float("inf"), -float("inf")]


@pytest.mark.parametrize("case", [dict(s_dst=0), dict(s_src=0), dict(alpha=0), dict(rp=0), dict(col=0), dict(heads=0),
                                  dict(heads=-3), dict(N=-1), dict(E=-1), dict(src_rows=-1), dict(N=0), dict(src_rows=0)] +
                         [dict(slope=s) for s in BAD_SLOPES])
def test_forward_argument_checks(case):
    assert _fwd(**case) == capi.EINVAL


def test_forward_without_entries_launches_nothing():
    assert _fwd(alpha=0, col=0, E=0) == 0
    assert _fwd(s_dst=0, s_src=0, alpha=0, col=0, N=0, E=0, src_rows=0) == 0


@pytest.mark.parametrize("case", [dict(alpha=0), dict(ga=0), dict(s_dst=0), dict(s_src=0), dict(rp=0), dict(col=0),
                                  dict(perm=0), dict(out=0), dict(gd=0), dict(gs=0), dict(heads=0), dict(heads=-1),
                                  dict(N=-1), dict(E=-1), dict(N=0)] + [dict(slope=s) for s in BAD_SLOPES])
def test_backward_argument_checks(case):
    assert _bwd(**case) == capi.EINVAL


def test_backward_of_nothing_launches_nothing():
    assert _bwd(alpha=0, ga=0, s_dst=0, s_src=0, col=0, perm=0, out=0, gd=0, gs=0, N=0, E=0) == 0
