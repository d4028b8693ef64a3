"""Softmax neighbour aggregation without a GPU: the symbols and the argument checks hcspmm_forward_softmax / hcspmm_softmax_backward
make before they touch HIP, the register budgets of spmm_softmax.hip and softmax_aggr_grad.hip (cross-compiled for gfx950),
the driver's flags, and the arithmetic SoftmaxAggregate / GENConv compose around the two launches (the relu / eps pre-pass,
dt = sum dZ (Q - Z^2)) against torch autograd of the dense formula, with the launches replaced by a torch stand-in."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from hcspmm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hc-spmm_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# waves per SIMD by kernel and build: (L lanes per row, VEC floats per lane); every one without scratch
OCC = {
    "softmax_plan_kernel": {(4, 4): 6, (8, 4): 4, (16, 4): 5, (32, 4): 5, (64, 4): 5, (4, 2): 8, (4, 1): 8},
    "softmax_window_kernel": {(4, 4): 5, (8, 4): 4, (16, 4): 4, (32, 4): 5, (64, 4): 5, (4, 2): 8, (4, 1): 8},
    "softmax_fixup_kernel": {4: 7, 2: 8, 1: 8},
    "softmax_grad_plan_kernel": {(4, 4): 7, (8, 4): 6, (16, 4): 6, (32, 4): 6, (64, 4): 7, (4, 2): 8, (4, 1): 8},
    "softmax_grad_window_kernel": {(4, 4): 6, (8, 4): 6, (16, 4): 6, (32, 4): 6, (64, 4): 8, (4, 2): 8, (4, 1): 8},
    "fixup_kernel": {4: 7, 2: 8, 1: 8},  # the backward's: spmm_impl.h fixup_kernel<F32, VEC>
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


def _expected(name):
    """(pinned occupancy, floats per lane) of a kernel of either unit"""
    m = re.search(r"\d+(softmax(?:_grad)?_(?:plan|window)_kernel)ILi(\d+)ELi(\d+)ELi\d+EE", name)
    if m:
        return OCC[m.group(1)][(int(m.group(2)), int(m.group(3)))], int(m.group(3))
    m = re.search(r"\d+(softmax_fixup_kernel)ILi(\d+)EE", name) or re.search(r"\d+(fixup_kernel)INS_3F32ELi(\d+)EE", name)
    if m:
        return OCC[m.group(1)][int(m.group(2))], int(m.group(2))
    return None


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("src", ["spmm_softmax.hip", "softmax_aggr_grad.hip"])
def test_softmax_kernels_keep_their_budgets(src):
    """L = 4 ... 64 at 16-byte lanes and L = 4 at 8- / 4-byte lanes, planned and plan-free, and the three fix-up builds of each
    unit: no scratch anywhere, occupancy as pinned above and at least four waves per SIMD on every 16-byte-lane build"""
    usage = _usage(src)
    assert len(usage) == 17, sorted(usage)
    for name, v in usage.items():
        want = _expected(name)
        assert want is not None, name
        assert (v["scratch"], v["occupancy"]) == (0, want[0]), (name, v)
        if want[1] == 4:
            assert v["occupancy"] >= 4, (name, v)


def _vp(v):
    return ctypes.c_void_p(0x1000 if v else 0)  # never dereferenced: every case fails before HIP is touched


def _fs(X=1, dtype=0, beta=1, Z=1, M=1, L=1, Q=1, rp=1, col=1, bp=1, e2c=1, e2r=1, ht=1, N=64, E=100, D=32, ldx=None, ldz=None):
    return capi.lib().hcspmm_forward_softmax(_vp(X), N, ldx or D, dtype, _vp(beta), _vp(Z), _vp(M), _vp(L), _vp(Q), ldz or D, _vp(rp),
                                             _vp(col), _vp(bp), _vp(e2c), _vp(e2r), _vp(ht), ctypes.c_void_p(0), None, N, E, D,
                                             ctypes.c_void_p(0), 0, ctypes.c_void_p(0))


def _sb(G=1, Z=1, M=1, L=1, X=1, beta=1, gX=1, rp=1, col=1, bp=1, e2c=1, e2r=1, ht=1, N=64, E=100, D=32, src_rows=64, ld_in=None,
        ldx=None, ldgx=None):
    return capi.lib().hcspmm_softmax_backward(_vp(G), _vp(Z), _vp(M), _vp(L), ld_in or D, src_rows, _vp(X), ldx or D, _vp(beta),
                                              _vp(gX), ldgx or D, _vp(rp), _vp(col), _vp(bp), _vp(e2c), _vp(e2r), _vp(ht),
                                              ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), 0, ctypes.c_void_p(0))


@pytest.mark.parametrize("case", [dict(dtype=1), dict(dtype=2), dict(dtype=7), dict(dtype=-1), dict(X=0), dict(beta=0), dict(Z=0),
                                  dict(ldx=16), dict(ldz=16), dict(rp=0), dict(col=0), dict(bp=0), dict(ht=0), dict(e2c=0),
                                  dict(D=0), dict(D=-4), dict(N=-1), dict(E=-1)])
def test_forward_softmax_argument_checks(case):
    assert _fs(**case) == capi.EINVAL


@pytest.mark.parametrize("case", [dict(G=0), dict(Z=0), dict(M=0), dict(L=0), dict(X=0), dict(beta=0), dict(gX=0), dict(ld_in=16),
                                  dict(ldx=16), dict(ldgx=16), dict(rp=0), dict(col=0), dict(bp=0), dict(ht=0), dict(e2c=0),
                                  dict(D=0), dict(N=-1), dict(E=-1), dict(src_rows=-1), dict(src_rows=0)])
def test_softmax_backward_argument_checks(case):
    assert _sb(**case) == capi.EINVAL


def test_nothing_to_do_and_nullable_statistics():
    assert _fs(N=0) == 0  # no rows, no launch
    assert _fs(N=0, M=0, L=0, Q=0) == 0
    assert _sb(N=0) == 0
    # the required output and beta are looked at before the row count, as hcspmm_forward_multi looks at its outputs
    assert _fs(N=0, Z=0) == capi.EINVAL and _fs(N=0, beta=0) == capi.EINVAL
    assert _sb(N=0, gX=0) == capi.EINVAL and _sb(N=0, beta=0) == capi.EINVAL
    assert capi.lib().hcspmm_softmax_workspace_bytes(None, 32) == 0


def test_symbols_and_abi_version():
    for name in ("hcspmm_forward_softmax", "hcspmm_softmax_backward", "hcspmm_softmax_workspace_bytes"):
        assert name in capi.SYMBOLS
        assert getattr(capi.lib(), name) is not None
    with open(os.path.join(ROOT, "include", "hcspmm.h")) as f:
        header = f.read()
    assert re.search(r"\bint hcspmm_forward_softmax\(", header) and re.search(r"\bint hcspmm_softmax_backward\(", header)
    assert re.search(r"\bsize_t hcspmm_softmax_workspace_bytes\(", header)
    assert re.search(r"#define HCSPMM_ABI_VERSION 3\b", header)
    assert capi.lib().hcspmm_abi_version() == 3
    assert len(capi.SYMBOLS["hcspmm_forward_softmax"][1]) == 24
    assert len(capi.SYMBOLS["hcspmm_softmax_backward"][1]) == 25


def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _driver():
    _pkg_imports()
    spec = importlib.util.spec_from_file_location("hc_spmm_main_gen", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_gen_flags():
    mod = _driver()
    args = mod.parse_args(["--model", "gen"])
    assert (args.model, args.gen_t, args.gen_learn_t) == ("gen", 1.0, False)
    args = mod.parse_args(["--model", "gen", "--gen-t", "0.25", "--gen-learn-t", "--directed"])
    assert (args.gen_t, args.gen_learn_t, args.directed) == (0.25, True, True)
    for extra in (["--norm", "sym"], ["--norm", "mean"], ["--aggr", "max"], ["--aggr", "mean"]):
        with pytest.raises(SystemExit):
            mod.parse_args(["--model", "gen"] + extra)
    # the existing flags keep their behaviour
    assert mod.parse_args(["--model", "sage"]).aggr == "max"
    assert mod.parse_args(["--model", "gcn", "--norm", "sym"]).norm == "sym"
    with pytest.raises(SystemExit):
        mod.parse_args(["--model", "pna", "--aggr", "max"])


# ---- the arithmetic around the launches, with a torch stand-in for both ------------------------------------------------


def _rows(rp):
    n = rp.numel() - 1
    return torch.repeat_interleave(torch.arange(n), (rp[1:] - rp[:-1]).long())


class _StandIn:
    """HCSPMM.forward_softmax / softmax_backward from index_add / scatter_reduce, in the dtype of their inputs"""

    def __init__(self):
        self.stats = []

    def forward_softmax(self, X, beta, rp, col, *rest):
        stats = rest[-1]
        self.stats.append(tuple(stats))
        n, D = rp.numel() - 1, X.size(1)
        rows, V = _rows(rp), X[col.long()]
        b = torch.as_tensor(beta, dtype=X.dtype).reshape(-1).expand(D)
        s = V * b
        M = torch.full((n, D), -float("inf"), dtype=X.dtype).scatter_reduce(0, rows[:, None].expand_as(s), s, "amax")
        w = torch.exp(s - M[rows])
        zero = torch.zeros(n, D, dtype=X.dtype)
        L = zero.index_add(0, rows, w)
        safe = L.clamp(min=1.0)
        Z, Q = zero.index_add(0, rows, w * V) / safe, zero.index_add(0, rows, w * V * V) / safe
        return Z, M if "M" in stats else None, L if "L" in stats else None, Q if "Q" in stats else None

    def softmax_backward(self, G, Z, M, L, X, beta, rp, col, *rest):
        n, D = rp.numel() - 1, X.size(1)
        rows, i = _rows(rp), col.long()
        b = torch.as_tensor(beta, dtype=X.dtype).reshape(-1).expand(D)
        x = X[rows]
        term = torch.exp(b * x - M[i]) / L[i] * G[i] * (1.0 + b * (x - Z[i]))
        return torch.zeros(n, D, dtype=X.dtype).index_add(0, rows, term)


def _dense_reference(X, t, A):
    """sum_j softmax_j(t x_j) x_j over the neighbours A[i] (a dense 0/1 matrix with multiplicities), rows without entries 0"""
    s = (t * X)[None, :, :].expand(A.size(0), -1, -1)  # [i, j, d]
    mask = (A > 0)[:, :, None]
    m = torch.where(mask, s, torch.full_like(s, -float("inf"))).amax(1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    w = A[:, :, None] * torch.exp(torch.where(mask, s - m, torch.full_like(s, -float("inf"))))
    return (w * X[None]).sum(1) / w.sum(1).clamp(min=1e-300)


def _graph40(symmetric, seed):
    rng = np.random.default_rng(seed)
    n = 40
    A = (rng.random((n, n)) < 0.12).astype(np.float64)
    if symmetric:
        A = np.maximum(A, A.T)
    A[::9] = 0  # rows without entries
    if symmetric:
        A[:, ::9] = 0
    A[3, :] = (rng.random(n) < 0.8) * (A[:, 3] if symmetric else 1.0)  # a longer row
    if symmetric:
        A[:, 3] = A[3, :]

    def csr(B):
        r, c = np.nonzero(B)
        rp = np.zeros(n + 1, np.int32)
        np.add.at(rp, r + 1, 1)
        return torch.from_numpy(np.cumsum(rp).astype(np.int32)), torch.from_numpy(c.astype(np.int32))

    def tensors(B):
        rp, col = csr(B)
        return (rp, col) + (torch.zeros(1, dtype=torch.int32),) * 6

    return torch.from_numpy(A), tensors(A), tensors(A.T)


@pytest.fixture
def gnn(monkeypatch):
    _pkg_imports()
    import GNN_model
    stand_in = _StandIn()
    monkeypatch.setattr(GNN_model.HCSPMM, "forward_softmax", stand_in.forward_softmax, raising=True)
    monkeypatch.setattr(GNN_model.HCSPMM, "softmax_backward", stand_in.softmax_backward, raising=True)
    monkeypatch.setattr(GNN_model, "transpose_permutation_i32", lambda rp, col: None)
    stand_in.transposed = {}  # id(row_pointers of A) -> the graph tensors of A^T
    monkeypatch.setattr(GNN_model, "transposed_graph", lambda graph: stand_in.transposed[id(graph[0])])
    return GNN_model, stand_in


@pytest.mark.parametrize("t_shape", ["scalar", "vector"])
@pytest.mark.parametrize("symmetric", [True, False])
def test_softmax_aggregate_gradients_match_the_dense_formula(gnn, symmetric, t_shape):
    """dX (the backward launch on the walked graph) and dt = sum dZ (Q - Z^2) against autograd of the dense formula, fp64"""
    GNN_model, stand_in = gnn
    A, graph, graph_t = _graph40(symmetric, 11)
    torch.manual_seed(12)
    D = 5
    X = torch.randn(40, D, dtype=torch.float64, requires_grad=True)
    t = (torch.tensor(0.7, dtype=torch.float64) if t_shape == "scalar" else torch.linspace(-1.5, 2.0, D, dtype=torch.float64))
    t.requires_grad_(True)
    stand_in.transposed[id(graph[0])] = graph_t
    Z = GNN_model.softmax_aggregate(X, graph, t, directed=not symmetric)
    assert stand_in.stats[-1] == ("M", "L", "Q")
    dZ = torch.randn(40, D, dtype=torch.float64)
    Z.backward(dZ)
    Xr, tr = X.detach().clone().requires_grad_(True), t.detach().clone().requires_grad_(True)
    Zr = _dense_reference(Xr, tr, A)
    Zr.backward(dZ)
    torch.testing.assert_close(Z.detach(), Zr.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(X.grad, Xr.grad, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(t.grad, tr.grad, rtol=1e-11, atol=1e-12)
    assert t.grad.shape == t.shape
    # a t that needs no gradient does not ask for Q, and a float t works
    GNN_model.softmax_aggregate(X, graph, 0.7, directed=not symmetric)
    assert stand_in.stats[-1] == ("M", "L")


def test_genconv_matches_the_dense_formula(gnn):
    """out = (X + softmax_aggregate(relu(X) + eps, t)) W with a learnt scalar t: out, X.grad, weights.grad and t.grad"""
    GNN_model, _ = gnn
    A, graph, _ = _graph40(True, 13)
    torch.manual_seed(14)
    conv = GNN_model.GENConv(6, 4, t=0.8, learn_t=True).double()
    assert conv.t.shape == () and float(conv.t.detach()) == pytest.approx(0.8) and conv.weights.shape == (6, 4)
    X = torch.randn(40, 6, dtype=torch.float64, requires_grad=True)
    out = conv(X, *graph, None)
    dY = torch.randn_like(out)
    out.backward(dY)
    Xr, Wr, tr = (v.detach().clone().requires_grad_(True) for v in (X, conv.weights, conv.t))
    ref = (Xr + _dense_reference(torch.relu(Xr) + 1e-7, tr, A)) @ Wr
    ref.backward(dY)
    for got, want in ((out.detach(), ref.detach()), (X.grad, Xr.grad), (conv.weights.grad, Wr.grad), (conv.t.grad, tr.grad)):
        torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-11)
    assert not isinstance(GNN_model.GENConv(6, 4).t, torch.Tensor)  # a fixed t is a float
    with pytest.raises(ValueError):
        conv(X, *graph, None, edge_weight=torch.ones(3))
