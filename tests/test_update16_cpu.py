"""The 16-bit update GEMM and weight gradient without a GPU: the three symbols, the argument checks hcspmm_dense_update_typed and
hcspmm_weight_grad_typed make before they touch HIP (never-dereferenced pointers), and the register / scratch / LDS report of
update_kernels_h16.hip cross-compiled for gfx950 with the build's flags (DESIGN.md section 3.4b holds the table)."""
import ctypes
import os
import re
import subprocess

import pytest

from hcspmm import capi
from test_gated_cpu import CSRC, HIPCC, ROOT

F32, F16, BF16 = 0, 1, 2


def _update(in_dtype=BF16, w_dtype=None, out_dtype=None, N=64, D=32, H=32, ld_in=None, ld_out=None, at=0x1000, W=0x2000, out=0x3000):
    vp = ctypes.c_void_p
    return capi.lib().hcspmm_dense_update_typed(vp(at), D if ld_in is None else ld_in, in_dtype, vp(W), in_dtype if w_dtype is None else w_dtype,
                                                H, 1, vp(out), H if ld_out is None else ld_out, in_dtype if out_dtype is None else out_dtype,
                                                N, D, H, vp(0))


def _wgrad(dtype=BF16, N=64, D=32, H=32, lda=None, ldb=None, A=0x1000, B=0x2000, ws=0x4000, ws_bytes=1 << 30):
    vp = ctypes.c_void_p
    return capi.lib().hcspmm_weight_grad_typed(vp(A), lda or D, vp(B), ldb or H, dtype, vp(0x3000), N, D, H, vp(ws), ws_bytes, vp(0))


def test_symbols_and_abi_version():
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    for name, n_args in (("hcspmm_dense_update_typed", 14), ("hcspmm_weight_grad_typed_workspace", 3), ("hcspmm_weight_grad_typed", 12)):
        assert re.search(r"\b%s\(" % name, header) and len(capi.SYMBOLS[name][1]) == n_args
    assert re.search(r"#define HCSPMM_ABI_VERSION 3\b", header) and capi.lib().hcspmm_abi_version() == 3


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("case", [dict(D=31, ld_in=32), dict(ld_in=33), dict(H=129), dict(H=0), dict(D=0), dict(at=0x1002), dict(ld_in=30),
                                  dict(ld_out=30), dict(w_dtype=3), dict(out_dtype=3), dict(N=-1), dict(D=10240, H=128), dict(W=0),
                                  dict(out=0)])
def test_update_refuses_before_hip(dtype, case):
    """odd D or stride, H outside 1 ... 128, a base off the dword grid, short strides, weights too large for LDS, NULL operands"""
    assert _update(dtype, **case) == capi.EINVAL


def test_update_dtype_pairs_and_nothing_to_do():
    for in_dtype, w_dtype, out_dtype in ((F16, BF16, F16), (BF16, F16, BF16), (F16, F16, BF16), (BF16, F32, F16), (3, 3, 3), (-1, F32, F32),
                                         (F32, BF16, F32), (F32, F32, BF16)):
        assert _update(in_dtype, w_dtype, out_dtype) == capi.EINVAL
    assert _update(F32, ld_in=34) == capi.EINVAL and _update(F32, ld_out=34) == capi.EINVAL  # fp32 forwards contiguous rows only
    for dtype in (F16, BF16):
        for w_dtype in (dtype, F32):
            for out_dtype in (dtype, F32):
                assert _update(dtype, w_dtype, out_dtype, N=0) == 0 and _update(dtype, w_dtype, out_dtype, N=0, ld_in=40, ld_out=34) == 0
        assert _update(dtype, N=0, D=31) == capi.EINVAL
    assert _update(F32, N=0) == 0


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("case", [dict(D=31), dict(H=31), dict(lda=33), dict(ldb=33), dict(lda=30), dict(A=0x1002), dict(B=0x2002),
                                  dict(D=144), dict(H=80), dict(N=0), dict(A=0)])
def test_weight_grad_refuses_before_hip(dtype, case):
    assert _wgrad(dtype, **case) == capi.EINVAL


def test_weight_grad_workspace():
    L = capi.lib()
    assert L.hcspmm_weight_grad_typed_workspace(70000, 96, 64) == 512 * 96 * 64 * 4  # 24 tiles: past hcspmm_weight_grad's 16
    assert L.hcspmm_weight_grad_workspace(70000, 96, 64) == 0 and _wgrad(F32, D=96, H=64) == capi.EINVAL
    assert L.hcspmm_weight_grad_typed_workspace(64, 144, 16) == 0 and L.hcspmm_weight_grad_typed_workspace(0, 32, 32) == 0
    for dtype in (F16, BF16):
        assert _wgrad(dtype, ws_bytes=32 * 32 * 4 - 1) == capi.EWORKSPACE and _wgrad(dtype, ws=0) == capi.EWORKSPACE
    assert _wgrad(3) == capi.EINVAL and _wgrad(-1) == capi.EINVAL


# waves per SIMD of every build (both element types agree): update kernels by T = 1 ... 8 with 16-byte and
# with masked dword row loads, weight-gradient kernels by HT with DT = 1 ... 8; the VGPR counts are the table's ceilings
UPDATE_OCC = {"1": "87655554", "0": "65544444"}
UPDATE_VGPRS = {"1": [64, 68, 74, 82, 84, 94, 94, 102], "0": [78, 86, 90, 98, 98, 98, 106, 114]}
WGRAD_OCC = {1: "88643322", 2: "86442222", 3: "54422222", 4: "44232211"}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_update16_kernels_keep_their_budgets():
    """2 types x 8 tile counts x 2 outputs x 2 row forms = 64 update kernels and 2 x 32 weight-gradient kernels: no scratch, the
    pinned occupancy, the update kernels no static LDS and no more VGPRs than recorded, the weight-gradient kernels their DT x HT
    accumulator tiles in AGPRs and at most 49 KiB of LDS"""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    extra = re.search(r"^update_kernels_h16\.o: HIPFLAGS \+= (.*)$", makefile, re.M).group(1).split()
    r = subprocess.run([HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", *extra, "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "update_kernels_h16.hip"), "-o",
                        os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-2000:]
    seen = {"update16": 0, "weight_grad16": 0}
    for b in re.split(r"Function Name: ", r.stdout)[1:]:
        v, a, scratch, occ, lds = (int(re.search(p, b).group(1)) for p in (
            r"\bVGPRs: (\d+)", r"AGPRs: (\d+)", r"ScratchSize \[bytes/lane\]: (\d+)", r"Occupancy \[waves/SIMD\]: (\d+)",
            r"LDS Size \[bytes/block\]: (\d+)"))
        name = b.split()[0]
        assert scratch == 0, name
        m = re.search(r"weight_grad16_partial_kernelINS_\w+?ELi(\d)ELi(\d)EE", name)
        if m:
            dt, ht = int(m.group(1)), int(m.group(2))
            assert occ == int(WGRAD_OCC[ht][dt - 1]) and a == 4 * dt * ht and lds <= 49 * 1024, (name, occ, a, lds)
            seen["weight_grad16"] += 1
        else:
            t, full8 = re.search(r"update16_kernelINS_\w+?ELi(\d)ELb[01]ELb([01])EE", name).groups()
            assert occ == int(UPDATE_OCC[full8][int(t) - 1]) and v <= UPDATE_VGPRS[full8][int(t) - 1] and lds == 0, (name, v, occ, lds)
            seen["update16"] += 1
    assert seen == {"update16": 64, "weight_grad16": 64}
