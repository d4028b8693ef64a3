"""One-pass sum / sumsq / max / min aggregation on fp16 / bf16 features without a GPU: the argument checks
hcspmm_forward_multi_typed makes before it touches HIP, the fp32 entry point's unchanged refusal of the 16-bit types, and the
register budget of spmm_multi16.hip (cross-compiled for gfx950 with the build's flags)."""
import ctypes
import os
import re

import pytest

from hcspmm import capi
from test_multi_aggr_cpu import CSRC, HIPCC, ROOT, _fm, _usage, _vp

F16, BF16 = 1, 2
# waves per SIMD of the (L, elements per lane) builds, planned and plan-free alike, both element types
OCC = {(4, 8): 4, (8, 8): 4, (16, 8): 4, (32, 8): 4, (64, 8): 4, (4, 4): (6, 7), (8, 4): (5, 5)}


def _typed(dtype=BF16, X=1, zsum=1, zsumsq=1, zmax=1, zmin=1, amax=1, amin=1, rp=1, col=1, N=64, E=100, D=32, ldx=None, ld_sum=None,
           ldz=None, ldarg=None, at=0x1000, zat=0x1000):
    p = lambda on, a=0x1000: ctypes.c_void_p(a if on else 0)  # noqa: E731  (never dereferenced)
    return capi.lib().hcspmm_forward_multi_typed(
        p(X, at), N, ldx or D, dtype, p(zsum), p(zsumsq), ld_sum or D, p(zmax, zat), p(zmin, zat), ldz or D, p(amax), p(amin),
        ldarg or D, _vp(rp), _vp(col), _vp(1), _vp(1), _vp(1), _vp(1), ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), 0,
        ctypes.c_void_p(0))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("case", [dict(D=33), dict(D=2), dict(D=0), dict(ldx=33), dict(ldz=35), dict(at=0x1002), dict(zat=0x1002),
                                  dict(ldx=16), dict(ldz=16), dict(ld_sum=16), dict(ldarg=16), dict(ldarg=16, amax=0),
                                  dict(zsum=0, zsumsq=0, zmax=0, zmin=0), dict(X=0), dict(rp=0), dict(col=0), dict(N=-1), dict(E=-1)])
def test_argument_checks_come_before_hip(dtype, case):
    assert _typed(dtype, **case) == capi.EINVAL


def test_symbol_abi_dtype_range_nothing_to_do_and_the_fp32_forward():
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    assert re.search(r"\bint hcspmm_forward_multi_typed\(", header) and re.search(r"#define HCSPMM_ABI_VERSION 3\b", header)
    assert "hcspmm_forward_multi_typed (round 27)" in header
    assert len(capi.SYMBOLS["hcspmm_forward_multi_typed"][1]) == 27 and capi.lib().hcspmm_abi_version() == 3
    assert _typed(-1) == capi.EINVAL and _typed(3) == capi.EINVAL and _typed(3, N=0) == capi.EINVAL
    for dtype in (0, F16, BF16):
        assert _typed(dtype, N=0) == 0 and _typed(dtype, N=0, amax=0, amin=0, ldarg=1) == 0
        assert _typed(dtype, N=0, ldarg=16) == capi.EINVAL
    # fp32 forwards: an odd width is served there, one stride for all four values
    assert _typed(0, D=33, N=0) == 0 and _typed(0, D=33, ldx=16) == capi.EINVAL and _typed(0, N=0, ld_sum=64) == capi.EINVAL
    assert _typed(BF16, D=33, N=0) == capi.EINVAL and _typed(BF16, N=0, ld_sum=64, ldz=40) == 0


def test_the_fp32_entry_point_still_refuses_the_16_bit_types():
    assert _fm(dtype=F16) == capi.EINVAL and _fm(dtype=BF16) == capi.EINVAL and _fm(dtype=BF16, N=0) == capi.EINVAL


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_multi16_kernels_keep_their_budget():
    """2 element types x 7 builds x (planned, plan-free) and a fix-up kernel per type: no scratch anywhere, at least four waves
    per SIMD on every 8-column build, occupancies as the DESIGN table has them"""
    usage = _usage("spmm_multi16.hip")
    assert len(usage) == 30 and sum("multi16_fixup_kernel" in k for k in usage) == 2
    for name, u in usage.items():
        print(name, u)
        assert u["scratch"] == 0, (name, u)
        m = re.search(r"multi16_(plan|window)_kernelINS_\d\w+?ELi(\d+)ELi(\d+)EEE", name)
        if m is None:
            assert u["occupancy"] == 5, (name, u)  # the fix-up kernels
            continue
        want = OCC[(int(m.group(2)), int(m.group(3)))]
        assert u["occupancy"] == (want if isinstance(want, int) else want[m.group(1) == "window"]), (name, u)
        assert u["occupancy"] >= 4
