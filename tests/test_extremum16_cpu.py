"""Max / min aggregation on fp16 / bf16 features without a GPU: the argument checks hcspmm_forward_extremum_typed makes before it
touches HIP, the fp32 entry point's unchanged refusal of the 16-bit types, and the register budget of spmm_extremum16.hip
(cross-compiled for gfx950 with the build's flags)."""
import ctypes
import os
import re
import subprocess

import pytest

from hcspmm import capi
from test_extremum_cpu import _fx
from test_gated_cpu import CSRC, HIPCC, ROOT, _vp

F16, BF16 = 1, 2


def _typed(dtype=BF16, X=1, Z=1, rp=1, col=1, N=64, E=100, D=32, ldx=None, ldz=None, reduce=0, arg=1, ldarg=None, at=0x1000,
           zat=0x1000):
    return capi.lib().hcspmm_forward_extremum_typed(
        ctypes.c_void_p(at if X else 0), N, ldx or D, ctypes.c_void_p(zat if Z else 0), ldz or D, dtype, _vp(rp), _vp(col), _vp(1),
        _vp(1), _vp(1), _vp(1), ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), 0, ctypes.c_void_p(0), reduce, _vp(arg),
        ldarg or D)


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("case", [dict(D=33), dict(D=2), dict(D=0), dict(ldx=33), dict(ldz=35), dict(at=0x1002), dict(zat=0x1002),
                                  dict(ldarg=16), dict(reduce=2), dict(reduce=-1), dict(ldx=16), dict(ldz=16), dict(X=0), dict(Z=0),
                                  dict(rp=0), dict(col=0), dict(N=-1), dict(E=-1)])
def test_argument_checks_come_before_hip(dtype, case):
    """never-dereferenced pointers: an odd width or stride, D = 2, a base off the dword grid, a short arg stride, a bad reduce and
    the fp32 entry's cases"""
    assert _typed(dtype, **case) == capi.EINVAL


def test_symbol_abi_dtype_range_and_nothing_to_do():
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    assert re.search(r"\bint hcspmm_forward_extremum_typed\(", header) and re.search(r"#define HCSPMM_ABI_VERSION 3\b", header)
    assert len(capi.SYMBOLS["hcspmm_forward_extremum_typed"][1]) == 23 and capi.lib().hcspmm_abi_version() == 3
    assert _typed(-1) == capi.EINVAL and _typed(3) == capi.EINVAL and _typed(3, N=0) == capi.EINVAL
    for dtype in (0, F16, BF16):
        assert _typed(dtype, N=0) == 0 and _typed(dtype, N=0, arg=0, ldarg=1) == 0 and _typed(dtype, N=0, reduce=2) == capi.EINVAL
    assert _typed(0, D=33, ldz=16) == capi.EINVAL and _typed(0, D=33, N=0) == 0  # fp32 forwards: an odd width is served there
    assert _typed(BF16, D=33, N=0) == capi.EINVAL


def test_the_fp32_entry_point_still_refuses_the_16_bit_types():
    assert _fx(dtype=F16) == capi.EINVAL and _fx(dtype=BF16) == capi.EINVAL and _fx(dtype=BF16, N=0) == capi.EINVAL


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_extremum16_kernels_keep_their_budget():
    """2 element types x 7 builds (L = 4 ... 64 at 8 elements per lane, L = 4, 8 at 4) x (planned, plan-free) and a fix-up kernel
    per type: no scratch and at least four waves per SIMD everywhere"""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    extra = re.search(r"^spmm_extremum16\.o: HIPFLAGS \+= (.*)$", makefile, re.M).group(1).split()
    r = subprocess.run([HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", *extra, "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spmm_extremum16.hip"), "-o",
                        os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-2000:]
    blocks = re.split(r"Function Name: ", r.stdout)[1:]
    assert len(blocks) == 30 and sum("extremum16_fixup_kernel" in b.split()[0] for b in blocks) == 2
    for b in blocks:
        v, scratch, occ = (int(re.search(p, b).group(1)) for p in (r"\bVGPRs: (\d+)", r"ScratchSize \[bytes/lane\]: (\d+)",
                                                                   r"Occupancy \[waves/SIMD\]: (\d+)"))
        print(b.split()[0], v, occ)
        assert scratch == 0 and occ >= 4, (b.split()[0], scratch, occ)
