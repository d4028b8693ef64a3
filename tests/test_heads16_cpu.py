"""The 16-bit multi-head kernels without a GPU: the two typed symbols and the argument checks they make before they touch HIP, the
resource report of spmm_heads16.hip / sddmm_heads16.hip (cross-compiled for gfx950 with the build's flags), and the
activation_dtype surface of GATConv and the driver."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

from hcspmm import capi
from test_edge16_cpu import _resource_report
from test_gated_cpu import HIPCC, ROOT, _pkg_imports, _vp

F16, BF16 = 1, 2
FWD, SDDMM = "hcspmm_forward_weighted_heads_typed", "hcspmm_sddmm_heads_typed"


def _fwd(dtype=BF16, z_dtype=None, X=0x1000, Z=0x2000, rp=1, N=64, E=100, D=32, heads=4, ldx=None, ldz=None, values=1, vindex=0,
         num_values=None):
    return getattr(capi.lib(), FWD)(ctypes.c_void_p(X), 64, ldx or D, ctypes.c_void_p(Z), ldz or D, dtype, dtype if z_dtype is None else z_dtype,
                                    _vp(rp), _vp(1), _vp(1), _vp(1), _vp(1), _vp(1), ctypes.c_void_p(0), None, N, E, D,
                                    ctypes.c_void_p(0), 0, ctypes.c_void_p(0), _vp(values), heads, _vp(vindex),
                                    E if num_values is None else num_values)


def _sddmm(dtype=BF16, A=0x1000, B=0x2000, out=1, rp=1, N=64, E=100, D=32, heads=4, lda=None, ldb=None):
    return getattr(capi.lib(), SDDMM)(ctypes.c_void_p(A), lda or D, ctypes.c_void_p(B), 64, ldb or D, dtype, _vp(out), _vp(rp), _vp(1),
                                      ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), heads)


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("call,case", [(_fwd, c) for c in (
    dict(ldx=33), dict(ldz=33), dict(X=0x1002), dict(Z=0x2002), dict(D=24, heads=4), dict(D=30, heads=1), dict(z_dtype=3),
    dict(heads=0), dict(heads=5), dict(values=0), dict(num_values=50), dict(vindex=1, num_values=0), dict(vindex=1, num_values=-1),
    dict(ldx=16), dict(Z=0), dict(rp=0))]
    + [(_sddmm, c) for c in (dict(lda=33), dict(ldb=35), dict(A=0x1002), dict(B=0x2002), dict(D=24, heads=4), dict(heads=0),
                             dict(D=520, heads=1), dict(D=264, heads=22), dict(lda=16), dict(out=0), dict(rp=0))])
def test_sixteen_bit_refusals_come_before_hip(dtype, call, case):
    """never-dereferenced pointers: odd strides, bases off the dword grid, Dh % 4 != 0, a foreign z_dtype, the fp32 call's errors"""
    assert call(dtype, **case) == capi.EINVAL


def test_symbols_forwarding_and_nothing_to_do():
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    assert re.search(r"#define HCSPMM_ABI_VERSION 3\b", header) and capi.lib().hcspmm_abi_version() == 3
    for name, n_args in ((FWD, 25), (SDDMM, 16)):  # declared, listed, exported
        assert re.search(r"\bint %s\(" % name, header) and len(capi.SYMBOLS[name][1]) == n_args and getattr(capi.lib(), name)
    for call in (_fwd, _sddmm):
        assert call(-1) == capi.EINVAL and call(3) == capi.EINVAL
    assert _fwd(BF16, z_dtype=F16) == capi.EINVAL and _fwd(0, z_dtype=BF16) == capi.EINVAL
    # fp32 forwards: the fp32 calls' codes for the same defects, and an odd stride is served there
    assert _fwd(0, D=24, heads=4) == capi.EINVAL and _fwd(0, values=0) == capi.EINVAL and _fwd(0, vindex=1, num_values=0) == capi.EINVAL
    assert _sddmm(0, D=24, heads=4) == capi.EINVAL and _sddmm(0, lda=16) == capi.EINVAL
    for dtype in (0, F16, BF16):
        assert _fwd(dtype, N=0, E=0) == 0 and _fwd(dtype, N=0, E=0, z_dtype=0) == 0 and _fwd(dtype, N=0, E=0, vindex=1, num_values=7) == 0
        assert _sddmm(dtype, E=0) == 0 and _sddmm(dtype, N=0, E=0) == 0
    assert _fwd(0, ldx=33, N=0, E=0) == 0 and _fwd(BF16, ldx=33, N=0, E=0) == capi.EINVAL
    assert _fwd(BF16, z_dtype=0, ldz=33, N=0, E=0) == 0  # an fp32 Z may have an odd stride


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("unit", ["spmm_heads16", "sddmm_heads16"])
def test_kernels_keep_their_budgets(unit):
    """every kernel of the two units (all types, lanes, forms, the fix-up builds): no scratch, >= 4 waves per SIMD"""
    report = _resource_report(unit)
    assert len(report) >= 28
    for name, (scratch, occ) in report.items():
        assert scratch == 0 and occ >= 4, (name, scratch, occ)


def test_gatconv_activation_dtype_and_the_driver():
    _pkg_imports()
    import GNN_model
    conv = GNN_model.GATConv(16, 8, heads=4, concat=True, activation_dtype=torch.bfloat16)
    assert conv.activation_dtype is torch.bfloat16 and GNN_model.GATConv(16, 8, heads=4, concat=True).activation_dtype is None
    assert all(p.dtype == torch.float32 for p in conv.parameters())
    for bad in (dict(concat=False), dict(input_dim=15), dict(activation_dtype=torch.float64)):
        with pytest.raises(ValueError, match="activation_dtype"):
            GNN_model.GATConv(**dict(dict(input_dim=16, output_dim=8, heads=4, concat=True, activation_dtype=torch.float16), **bad))
    with pytest.raises(ValueError, match="activation_dtype"):
        GNN_model.edge_weighted_aggregate_heads(None, None, (None, None), activation_dtype=torch.float64)
    assert hasattr(GNN_model, "EdgeWeightedAggregateHeads16")
    spec = importlib.util.spec_from_file_location("hc_spmm_main_heads16", os.path.join(ROOT, "hc-spmm_amd", "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(["--model", "gat", "--gat-concat", "--heads", "4", "--activation-dtype", "bf16"])
    assert (args.model, args.gat_concat, args.activation_dtype) == ("gat", True, "bf16")
    for refused in (["--model", "gat"], ["--model", "gatv2", "--gat-concat"], ["--model", "gatv2"]):
        with pytest.raises(SystemExit):
            mod.parse_args(refused + ["--activation-dtype", "bf16"])
