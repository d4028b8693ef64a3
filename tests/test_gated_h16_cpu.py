"""Gated aggregation on fp16 / bf16 operands without a GPU: the symbol and the argument checks hcspmm_forward_gated_typed makes
before it touches HIP, the register budgets of spmm_gate16.hip (cross-compiled for gfx950 with the build's flags), and the
gather_dtype backward recipe on a torch stand-in for the launch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from hcspmm import capi
from test_gated_cpu import CSRC, HIPCC, ROOT, _graph40, _vp, gnn  # noqa: F401  (gnn: the stand-in fixture)

F16, BF16 = 1, 2
# waves per SIMD of the builds (L, VEC) below, by (element type, kernel) and outputs 1 = gate, 2 = dgate,
# 3 = both
BUILDS = [(4, 8), (8, 8), (16, 8), (32, 8), (64, 8), (4, 4), (8, 4)]
OCC = {
    ("3F16", "plan"): {1: "5555588", 2: "5555688", 3: "4444477"}, ("3F16", "window"): {1: "4555788", 2: "5555788", 3: "4444677"},
    ("4BF16", "plan"): {1: "5444588", 2: "5555588", 3: "4444477"}, ("4BF16", "window"): {1: "4444778", 2: "5555788", 3: "4444677"},
}


def _typed(dtype=BF16, P=1, Q=1, V=1, zg=1, zd=1, rp=1, N=64, E=100, D=32, src_rows=64, ldp=None, ldq=None, ldv=None, ldz=None, at=0x1000):
    return capi.lib().hcspmm_forward_gated_typed(
        ctypes.c_void_p(at if P else 0), ldp or D, _vp(Q), ldq or D, _vp(V), ldv or D, src_rows, dtype, _vp(zg), _vp(zd), ldz or D,
        _vp(rp), _vp(1), _vp(1), _vp(1), _vp(1), _vp(1), ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), 0, ctypes.c_void_p(0))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("case", [dict(D=33), dict(D=2), dict(D=0), dict(ldp=33), dict(ldq=35), dict(ldv=37), dict(at=0x1002),
                                  dict(zg=0, zd=0), dict(ldp=16), dict(ldz=16), dict(P=0), dict(Q=0), dict(V=0), dict(rp=0),
                                  dict(src_rows=0), dict(N=-1)])
def test_argument_checks_come_before_hip(dtype, case):
    """never-dereferenced pointers: an odd width or stride, D = 2, a base off the dword grid and the fp32 entry's cases"""
    assert _typed(dtype, **case) == capi.EINVAL


def test_symbol_abi_dtype_range_and_nothing_to_do():
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    assert re.search(r"\bint hcspmm_forward_gated_typed\(", header) and re.search(r"#define HCSPMM_ABI_VERSION 3\b", header)
    assert len(capi.SYMBOLS["hcspmm_forward_gated_typed"][1]) == 25 and capi.lib().hcspmm_abi_version() == 3
    assert _typed(-1) == capi.EINVAL and _typed(3) == capi.EINVAL and _typed(3, N=0) == capi.EINVAL
    for dtype in (0, F16, BF16):
        assert _typed(dtype, N=0) == 0 and _typed(dtype, N=0, zd=0) == 0 and _typed(dtype, N=0, zg=0, zd=0) == capi.EINVAL
    assert _typed(0, D=33, ldz=16) == capi.EINVAL and _typed(0, D=33, N=0) == 0  # fp32 forwards: an odd width is served there
    assert _typed(BF16, D=33, N=0) == capi.EINVAL


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_gate16_kernels_keep_their_budgets():
    """2 element types x 3 output sets x 7 builds x (planned, plan-free) = 84 kernels and the one fix-up build they launch: no
    scratch, the pinned occupancy and at least four waves per SIMD everywhere; a single-output build takes no more registers than
    its two-output twin"""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    extra = re.search(r"^spmm_gate16\.o: HIPFLAGS \+= (.*)$", makefile, re.M).group(1).split()
    r = subprocess.run([HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", *extra, "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spmm_gate16.hip"), "-o",
                        os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-2000:]
    blocks = re.split(r"Function Name: ", r.stdout)[1:]
    vgprs = {}
    for b in blocks:
        v, scratch, occ = (int(re.search(p, b).group(1)) for p in (r"\bVGPRs: (\d+)", r"ScratchSize \[bytes/lane\]: (\d+)",
                                                                   r"Occupancy \[waves/SIMD\]: (\d+)"))
        assert scratch == 0 and occ >= 4, (b.split()[0], scratch, occ)
        m = re.search(r"gate16_(plan|window)_kernelINS_(\w+?)ELi(\d)ELi(\d+)ELi(\d+)EE", b.split()[0])
        if m:
            key = (m.group(2), m.group(1), int(m.group(3)), (int(m.group(4)), int(m.group(5))))
            print(key, v, occ)
            assert occ == int(OCC[key[:2]][key[2]][BUILDS.index(key[3])]), (key, occ)
            vgprs[key] = v
    assert len(vgprs) == 84 and len(blocks) == 85 and any("fixup_kernelINS_3F32ELi4EE" in b.split()[0] for b in blocks)
    assert all(v <= vgprs[(e, k, 3, lv)] for (e, k, out, lv), v in vgprs.items())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("symmetric", [True, False])
def test_gather_dtype_gradients_are_those_of_the_rounded_operands(gnn, monkeypatch, symmetric, dtype):
    """column blocks of one buffer and a dZ representable in dtype: the launches see 16-bit operands only, and Z and the gradients
    equal fp64 autograd of the dense formula at the rounded operands"""
    GNN_model, stand_in = gnn
    A, graph, graph_t = _graph40(symmetric, 11)
    stand_in.transposed[id(graph[0])] = graph_t

    def launch(*a):
        assert all(t.dtype == dtype for t in a[:3])
        return stand_in.forward_gated(*(t.double() for t in a[:3]), *a[3:])

    monkeypatch.setattr(GNN_model.HCSPMM, "forward_gated", launch)
    torch.manual_seed(12)
    D = 6
    proj = torch.randn(40, 3 * D, dtype=torch.float64, requires_grad=True)
    Z = GNN_model.gated_aggregate(proj[:, :D], proj[:, D:2 * D], proj[:, 2 * D:], graph, directed=not symmetric, gather_dtype=dtype)
    dZ = torch.randn(40, D).to(dtype).double()
    Z.backward(dZ)
    assert stand_in.asked == [("gate", "dgate"), ("gate", "dgate")]
    ref = proj.detach().to(dtype).double().requires_grad_(True)
    Zr = (A[:, :, None] * torch.sigmoid(ref[:, None, :D] + ref[None, :, D:2 * D]) * ref[None, :, 2 * D:]).sum(1)
    Zr.backward(dZ)
    torch.testing.assert_close(Z.detach(), Zr.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(proj.grad, ref.grad, rtol=1e-11, atol=1e-12)
