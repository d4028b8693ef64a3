"""Max / min aggregation without a GPU: the register budgets of spmm_extremum.hip (cross-compiled for gfx950), the argument
checks hcspmm_forward_extremum / hcspmm_forward_extremum_backward make before they touch HIP, and the driver's flags."""
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

# (scratch bytes per lane, waves per SIMD) by kernel and build: L lanes per row, VEC floats per lane,
# forward (0) or backward (1)
PLAN_OCC = {(4, 4, 0): 6, (8, 4, 0): 6, (16, 4, 0): 6, (32, 4, 0): 6, (64, 4, 0): 7, (4, 2, 0): 8, (4, 1, 0): 8,
            (4, 4, 1): 7, (8, 4, 1): 7, (16, 4, 1): 7, (32, 4, 1): 7, (64, 4, 1): 8, (4, 2, 1): 8, (4, 1, 1): 8}
WINDOW_OCC = {(4, 4, 0): 7, (8, 4, 0): 6, (16, 4, 0): 6, (32, 4, 0): 6, (64, 4, 0): 8, (4, 2, 0): 8, (4, 1, 0): 8,
              (4, 4, 1): 7, (8, 4, 1): 7, (16, 4, 1): 7, (32, 4, 1): 7, (64, 4, 1): 8, (4, 2, 1): 8, (4, 1, 1): 8}
FIXUP_OCC = {4: 8, 2: 8, 1: 8}     # extremum_fixup_kernel<VEC>
BIN_FIXUP_OCC = {4: 7, 2: 8, 1: 8}  # the binary fix-up pass, instantiated here for the backward's split rows


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


def _expected(name):
    m = re.search(r"extremum_plan_kernelILi(\d+)ELi(\d+)ELb(\d)E", name)
    if m:
        return PLAN_OCC[tuple(int(x) for x in m.groups())]
    m = re.search(r"extremum_window_kernelILi(\d+)ELi(\d+)ELb(\d)E", name)
    if m:
        return WINDOW_OCC[tuple(int(x) for x in m.groups())]
    m = re.search(r"extremum_fixup_kernelILi(\d+)E", name)
    if m:
        return FIXUP_OCC[int(m.group(1))]
    m = re.search(r"fixup_kernelINS_3F32ELi(\d+)E", name)
    if m:
        return BIN_FIXUP_OCC[int(m.group(1))]
    return None


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_extremum_kernels_keep_their_budgets():
    """fp32, L = 4 ... 64 at 16-byte lanes and L = 4 at 8- / 4-byte lanes, forward and backward: no scratch anywhere,
    occupancy as pinned above"""
    usage = _usage("spmm_extremum.hip")
    assert len(usage) == 34, sorted(usage)
    for name, v in usage.items():
        occ = _expected(name)
        assert occ is not None, name
        assert (v["scratch"], v["occupancy"]) == (0, occ), (name, v)


def _vp(v):
    return ctypes.c_void_p(0x1000 if v else 0)  # never dereferenced: every case fails before HIP is touched


def _fx(X=1, Z=1, dtype=0, rp=1, col=1, bp=1, e2c=1, e2r=1, ht=1, N=64, E=100, D=32, ldx=None, ldz=None, reduce=0, arg=1,
        ldarg=None):
    return capi.lib().hcspmm_forward_extremum(_vp(X), N, ldx or D, _vp(Z), ldz or D, dtype, _vp(rp), _vp(col), _vp(bp), _vp(e2c),
                                              _vp(e2r), _vp(ht), ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), 0,
                                              ctypes.c_void_p(0), reduce, _vp(arg), ldarg or D)


def _bw(G=1, arg=1, GX=1, rp=1, col=1, bp=1, e2c=1, e2r=1, ht=1, perm=1, N=64, E=100, D=32, ldg=None, ldarg=None, ldgx=None):
    return capi.lib().hcspmm_forward_extremum_backward(_vp(G), ldg or D, _vp(arg), ldarg or D, _vp(GX), ldgx or D, _vp(rp),
                                                       _vp(col), _vp(bp), _vp(e2c), _vp(e2r), _vp(ht), ctypes.c_void_p(0), None,
                                                       N, E, D, _vp(perm), ctypes.c_void_p(0), 0, ctypes.c_void_p(0))


@pytest.mark.parametrize("case", [dict(dtype=1), dict(dtype=2), dict(dtype=7), dict(reduce=2), dict(reduce=-1), dict(X=0),
                                  dict(Z=0), dict(rp=0), dict(col=0), dict(bp=0), dict(ht=0), dict(D=0), dict(N=-1), dict(E=-1),
                                  dict(ldx=16), dict(ldz=16), dict(ldarg=16)])
def test_forward_extremum_argument_checks(case):
    assert _fx(**case) == capi.EINVAL


@pytest.mark.parametrize("case", [dict(G=0), dict(arg=0), dict(GX=0), dict(rp=0), dict(col=0), dict(perm=0), dict(D=0),
                                  dict(N=-1), dict(E=-1), dict(ldg=16), dict(ldarg=16), dict(ldgx=16)])
def test_forward_extremum_backward_argument_checks(case):
    assert _bw(**case) == capi.EINVAL


def test_extremum_nothing_to_do_and_optional_arg():
    assert _fx(N=0) == 0 and _bw(N=0) == 0  # no rows, no launch
    assert _fx(N=0, arg=0, ldarg=1) == 0  # arg_out NULL: its stride is not looked at
    assert capi.lib().hcspmm_extremum_workspace_bytes(None, 32) == 0


def _driver():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_sage", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_sage_flags():
    mod = _driver()
    for aggr in ("max", "min", "mean"):
        args = mod.parse_args(["--model", "sage", "--aggr", aggr])
        assert args.model == "sage" and args.aggr == aggr
    for norm in ("sym", "mean"):
        with pytest.raises(SystemExit):
            mod.parse_args(["--model", "sage", "--norm", norm])
    with pytest.raises(SystemExit):
        mod.parse_args(["--model", "sage", "--aggr", "sum"])
