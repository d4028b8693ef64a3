"""Softmax aggregation on fp16 / bf16 features without a GPU: the argument checks hcspmm_forward_softmax_typed and
hcspmm_softmax_backward_typed make before they touch HIP, the fp32 entry point's unchanged refusal of the 16-bit types, and the
register budget of spmm_softmax16.hip and softmax_aggr_grad16.hip (cross-compiled for gfx950 with the build's flags; DESIGN.md
section 3.18b)."""
import ctypes
import os
import re
import subprocess

import pytest

from hcspmm import capi
from test_softmax_aggr_cpu import CSRC, HIPCC, ROOT, _fs, _vp

F16, BF16 = 1, 2


def _at(p):
    return ctypes.c_void_p(p)


def _fwd(dtype=BF16, X=0x1000, beta=1, Z=0x1000, lse=1, var=1, rp=1, col=1, N=64, E=100, D=32, ldx=None, ldz=None, ld_stat=None):
    return capi.lib().hcspmm_forward_softmax_typed(
        _at(X), N, ldx or D, dtype, _vp(beta), _at(Z), ldz or D, _vp(lse), _vp(var), ld_stat or D, _vp(rp), _vp(col), _vp(1), _vp(1),
        _vp(1), _vp(1), ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), 0, ctypes.c_void_p(0))


def _bwd(dtype=BF16, G=0x1000, Z=0x1000, lse=1, X=0x1000, beta=1, gX=1, rp=1, col=1, N=64, E=100, D=32, src_rows=64, ld_in=None,
         ld_stat=None, ldx=None, ldgx=None):
    return capi.lib().hcspmm_softmax_backward_typed(
        _at(G), _at(Z), ld_in or D, _vp(lse), ld_stat or D, src_rows, _at(X), ldx or D, dtype, _vp(beta), _vp(gX), ldgx or D, _vp(rp),
        _vp(col), _vp(1), _vp(1), _vp(1), _vp(1), ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), 0, ctypes.c_void_p(0))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("case", [dict(D=33), dict(D=2), dict(D=0), dict(ldx=33), dict(ldz=35), dict(X=0x1002), dict(Z=0x1002),
                                  dict(ld_stat=16), dict(ldx=16), dict(ldz=16), dict(X=0), dict(Z=0), dict(beta=0), dict(rp=0),
                                  dict(col=0), dict(N=-1), dict(E=-1)])
def test_forward_argument_checks_come_before_hip(dtype, case):
    """never-dereferenced pointers: an odd width or stride, D = 2, a base off the dword grid, a short statistics stride and the
    fp32 entry's cases"""
    assert _fwd(dtype, **case) == capi.EINVAL


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("case", [dict(D=33), dict(D=2), dict(D=0), dict(ld_in=33), dict(ldx=35), dict(G=0x1002), dict(Z=0x1002),
                                  dict(X=0x1002), dict(ld_in=16), dict(ld_stat=16), dict(ldx=16), dict(ldgx=16), dict(G=0), dict(Z=0),
                                  dict(lse=0), dict(X=0), dict(beta=0), dict(gX=0), dict(rp=0), dict(col=0), dict(N=-1), dict(E=-1),
                                  dict(src_rows=-1), dict(src_rows=0)])
def test_backward_argument_checks_come_before_hip(dtype, case):
    assert _bwd(dtype, **case) == capi.EINVAL


def test_symbols_abi_dtype_range_and_nothing_to_do():
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    assert re.search(r"\bint hcspmm_forward_softmax_typed\(", header) and re.search(r"\bint hcspmm_softmax_backward_typed\(", header)
    assert re.search(r"#define HCSPMM_ABI_VERSION 3\b", header) and capi.lib().hcspmm_abi_version() == 3
    assert len(capi.SYMBOLS["hcspmm_forward_softmax_typed"][1]) == 24 and len(capi.SYMBOLS["hcspmm_softmax_backward_typed"][1]) == 26
    for fn in (_fwd, _bwd):
        for bad in (-1, 0, 3):  # fp32 is refused here: its outputs differ
            assert fn(bad) == capi.EINVAL and fn(bad, N=0) == capi.EINVAL
        for dtype in (F16, BF16):
            assert fn(dtype, N=0) == 0 and fn(dtype, N=0, D=33) == capi.EINVAL
    assert _fwd(BF16, N=0, lse=0, var=0, ld_stat=1) == 0  # statistics that are not asked for need no stride


def test_the_fp32_entry_point_still_refuses_the_16_bit_types():
    assert _fs(dtype=F16) == capi.EINVAL and _fs(dtype=BF16) == capi.EINVAL and _fs(dtype=BF16, N=0) == capi.EINVAL


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("unit,kernels", [("spmm_softmax16", 60), ("softmax_aggr_grad16", 29)])
def test_softmax16_kernels_keep_their_budget(unit, kernels):
    """forward: 2 element types x (with, without Var) x (7 builds x (planned, plan-free) + a fix-up kernel); backward: 2 x 7 x 2
    and the binary fix-up pass: no scratch and at least four waves per SIMD everywhere"""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    extra = re.search(r"^%s\.o: HIPFLAGS \+= (.*)$" % unit, makefile, re.M).group(1).split()
    r = subprocess.run([HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", *extra, "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, unit + ".hip"), "-o",
                        os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-2000:]
    blocks = re.split(r"Function Name: ", r.stdout)[1:]
    assert len(blocks) == kernels
    for b in blocks:
        v, scratch, occ = (int(re.search(p, b).group(1)) for p in (r"\bVGPRs: (\d+)", r"ScratchSize \[bytes/lane\]: (\d+)",
                                                                   r"Occupancy \[waves/SIMD\]: (\d+)"))
        print(b.split()[0], v, occ)
        assert scratch == 0 and occ >= 4, (b.split()[0], scratch, occ)
