"""Edge-feature messages on fp16 / bf16 operands without a GPU: the two typed symbols and the argument checks they make before they
touch HIP, the register budgets of spmm_edgevec16.hip / edgevec16_grad.hip (cross-compiled for gfx950 with the build's flags), and
the activation_dtype surface of GINEConv and the driver."""
import ctypes
import importlib.util
import os
import re
import subprocess

import pytest
import torch

from hcspmm import capi
from test_gated_cpu import CSRC, HIPCC, ROOT, _pkg_imports, _vp

F16, BF16 = 1, 2
FWD, GRAD = "hcspmm_forward_edge_messages_typed", "hcspmm_edge_messages_grad_typed"


def _fwd(dtype=BF16, op=1, X=0x1000, F=0x2000, Z=1, rp=1, N=64, E=100, D=32, x_rows=64, f_rows=100, ldx=None, ldf=None, ldz=None):
    return getattr(capi.lib(), FWD)(ctypes.c_void_p(X), x_rows, ldx or D, ctypes.c_void_p(F), f_rows, ldf or D, dtype, _vp(0), op, _vp(Z),
                                    ldz or D, _vp(rp), _vp(1), _vp(1), _vp(1), _vp(1), _vp(1), ctypes.c_void_p(0), None, N, E, D,
                                    ctypes.c_void_p(0), 0, ctypes.c_void_p(0))


def _grad(dtype=BF16, op=1, G=0x1000, X=0x2000, F=0x3000, out=0x4000, rp=1, N=64, E=100, D=32, ldg=None, ldx=None, ldf=None, ldgf=None):
    return getattr(capi.lib(), GRAD)(ctypes.c_void_p(G), ldg or D, ctypes.c_void_p(X), 64, ldx or D, ctypes.c_void_p(F), ldf or D, dtype,
                                     ctypes.c_void_p(out), ldgf or D, op, _vp(rp), _vp(1), N, E, D, ctypes.c_void_p(0))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("call,case", [(_fwd, c) for c in (dict(D=33), dict(D=2), dict(ldx=33), dict(ldf=35), dict(X=0x1002), dict(F=0x2002))]
                         + [(_grad, c) for c in (dict(D=33), dict(D=2), dict(ldg=33), dict(ldx=35), dict(ldf=37), dict(ldgf=39),
                                                 dict(G=0x1002), dict(X=0x2002), dict(F=0x3002), dict(out=0x4002))])
def test_sixteen_bit_refusals_come_before_hip(dtype, call, case):
    """never-dereferenced pointers: an odd width or stride, D = 2 and a base off the dword grid"""
    assert call(dtype, **case) == capi.EINVAL


def test_symbols_dtype_range_fp32_forwarding_and_nothing_to_do():
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    assert re.search(r"#define HCSPMM_ABI_VERSION 3\b", header) and capi.lib().hcspmm_abi_version() == 3
    for name, n_args in ((FWD, 25), (GRAD, 17)):  # declared, listed, exported
        assert re.search(r"\bint %s\(" % name, header) and len(capi.SYMBOLS[name][1]) == n_args and getattr(capi.lib(), name)
    for call in (_fwd, _grad):
        assert call(-1) == capi.EINVAL and call(3) == capi.EINVAL and call(3, N=0, E=0) == capi.EINVAL
        assert call(0, op=7) == capi.EINVAL and call(BF16, op=7) == capi.EINVAL
    # the fp32 call's code for the same defect; an odd width is served there, and copy reads no X: its base may sit anywhere
    assert _fwd(0, ldf=16) == capi.EINVAL and _fwd(0, F=0) == capi.EINVAL and _fwd(0, f_rows=50) == capi.EINVAL
    assert _grad(0, ldgf=16) == capi.EINVAL and _grad(0, X=0) == capi.EINVAL
    for dtype in (0, F16, BF16):
        assert _fwd(dtype, N=0) == 0 and _fwd(dtype, N=0, E=0, F=0) == 0 and _grad(dtype, E=0) == 0
        assert _fwd(dtype, F=0) == capi.EINVAL and _fwd(dtype, Z=0) == capi.EINVAL and _fwd(dtype, f_rows=50) == capi.EINVAL
        assert _grad(dtype, out=0) == capi.EINVAL and _grad(dtype, rp=0) == capi.EINVAL
    assert _fwd(0, D=33, N=0) == 0 and _fwd(BF16, D=33, N=0) == capi.EINVAL
    assert _fwd(BF16, op=2, X=0x1002, ldx=33, N=0) == 0 and _grad(BF16, op=2, X=0x2002, F=0x3002, ldf=33, E=0) == 0


def _resource_report(unit):
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^%s\.o: HIPFLAGS \+= (.*)$" % unit, makefile, re.M)
    r = subprocess.run([HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", *(m.group(1).split() if m else []),
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, unit + ".hip"), "-o", os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-2000:]
    fields = (r"ScratchSize \[bytes/lane\]: (\d+)", r"Occupancy \[waves/SIMD\]: (\d+)")
    return {b.split()[0]: tuple(int(re.search(p, b).group(1)) for p in fields) for b in re.split(r"Function Name: ", r.stdout)[1:]}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("unit,pattern,builds,extra", [
    ("spmm_edgevec16", r"edgevec16_(plan|window)_kernelINS_(3F16|4BF16)ELi([012])ELi(\d+)ELi(\d+)EE",
     [(4, 8), (8, 8), (16, 8), (32, 8), (64, 8), (4, 4), (8, 4)], 1),
    ("edgevec16_grad", r"edgevec16_grad_(kernel)INS_(3F16|4BF16)ELi([012])ELi(\d+)ELi(\d+)EE",
     [(4, 8), (8, 8), (16, 8), (32, 8), (64, 8), (1, 4), (2, 4), (4, 4), (8, 4)], 0)])
def test_kernels_keep_their_budgets(unit, pattern, builds, extra):
    """2 types x 3 ops x the (L, VEC) builds (x planned, plan-free, + the fp32 fix-up build in the forward): no scratch, >= 4 waves"""
    report = _resource_report(unit)
    seen = set()
    for name, (scratch, occ) in report.items():
        assert scratch == 0 and occ >= 4, (name, scratch, occ)
        m = re.search(pattern, name)
        if m:
            seen.add((m.group(1), m.group(2), int(m.group(3)), (int(m.group(4)), int(m.group(5)))))
    kinds = ("plan", "window") if extra else ("kernel",)
    assert seen == {(k, e, op, lv) for k in kinds for e in ("3F16", "4BF16") for op in range(3) for lv in builds}
    assert len(report) == len(seen) + extra and (not extra or any("fixup_kernelINS_3F32ELi4EE" in n for n in report))


def test_gineconv_activation_dtype_and_the_driver():
    _pkg_imports()
    import GNN_model
    conv = GNN_model.GINEConv(24, 15, 5, activation_dtype=torch.bfloat16)
    assert conv.activation_dtype is torch.bfloat16 and GNN_model.GINEConv(24, 15, 5).activation_dtype is None
    assert {n: tuple(p.shape) for n, p in conv.named_parameters()} == {"weights": (24, 15), "weights_edge": (5, 24)}
    assert all(p.dtype == torch.float32 for p in conv.parameters())
    for bad in (dict(input_dim=23), dict(input_dim=2), dict(activation_dtype=torch.float64)):
        with pytest.raises(ValueError, match="activation_dtype"):
            GNN_model.GINEConv(**dict(dict(input_dim=24, output_dim=16, edge_dim=5, activation_dtype=torch.float16), **bad))
    with pytest.raises(ValueError, match="gather_dtype"):
        GNN_model.edge_message_aggregate(None, torch.zeros(0, 8), (None, torch.zeros(0)), "copy", gather_dtype=torch.float64)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_edge16", os.path.join(ROOT, "hc-spmm_amd", "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(["--model", "gine", "--activation-dtype", "bf16"])
    assert (args.model, args.activation_dtype) == ("gine", "bf16")
