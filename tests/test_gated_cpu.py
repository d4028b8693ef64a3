"""Gated neighbour aggregation without a GPU: the symbols, the argument checks hcspmm_forward_gated makes before it touches HIP,
the register budgets of spmm_gated.hip (cross-compiled for gfx950), the driver's flags and the layer's refusals."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

from hcspmm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hc-spmm_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# waves per SIMD by kernel and build: outputs (1 = gate, 2 = dgate, 3 = both) -> (L lanes per task, VEC
# floats per lane) -> occupancy; every one without scratch
BUILDS = [(4, 4), (8, 4), (16, 4), (32, 4), (64, 4), (4, 2), (4, 1)]
PLAN_OCC = {
    1: {(4, 4): 6, (8, 4): 6, (16, 4): 6, (32, 4): 6, (64, 4): 7, (4, 2): 8, (4, 1): 8},
    2: {(4, 4): 7, (8, 4): 6, (16, 4): 7, (32, 4): 7, (64, 4): 7, (4, 2): 8, (4, 1): 8},
    3: {(4, 4): 5, (8, 4): 5, (16, 4): 6, (32, 4): 6, (64, 4): 6, (4, 2): 8, (4, 1): 8},
}
WINDOW_OCC = {
    1: {(4, 4): 6, (8, 4): 6, (16, 4): 6, (32, 4): 6, (64, 4): 7, (4, 2): 8, (4, 1): 8},
    2: {(4, 4): 6, (8, 4): 6, (16, 4): 6, (32, 4): 7, (64, 4): 8, (4, 2): 8, (4, 1): 8},
    3: {(4, 4): 5, (8, 4): 5, (16, 4): 5, (32, 4): 6, (64, 4): 7, (4, 2): 8, (4, 1): 8},
}
FIXUP_OCC = {4: 7, 2: 8, 1: 8}  # fixup_kernel<F32, VEC>, the binary pass


# ------------------------------------------------------------------------------------------- symbols and ABI
def test_symbols_and_abi_version():
    for name in ("hcspmm_forward_gated", "hcspmm_gated_workspace_bytes"):
        assert name in capi.SYMBOLS
        assert getattr(capi.lib(), name) is not None
    with open(os.path.join(ROOT, "include", "hcspmm.h")) as f:
        header = f.read()
    assert re.search(r"\bint hcspmm_forward_gated\(", header) and re.search(r"\bsize_t hcspmm_gated_workspace_bytes\(", header)
    assert re.search(r"#define HCSPMM_ABI_VERSION 3\b", header)
    assert capi.lib().hcspmm_abi_version() == 3
    assert len(capi.SYMBOLS["hcspmm_forward_gated"][1]) == 24
    assert capi.lib().hcspmm_gated_workspace_bytes(None, 32) == 0


def test_the_library_exports_exactly_the_headers_symbols():
    with open(os.path.join(ROOT, "include", "hcspmm.h")) as f:
        declared = set(re.findall(r"\b(hcspmm_\w+)\(", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)))
    assert declared == set(capi.SYMBOLS), sorted(declared ^ set(capi.SYMBOLS))  # (capi.lib() resolves every one of them)
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("hcspmm_")}
        assert exported == declared, sorted(exported ^ declared)


# ------------------------------------------------------------------------------------------- argument checks
def _vp(v):
    return ctypes.c_void_p(0x1000 if v else 0)  # never dereferenced: every case fails before HIP is touched


def _fg(P=1, Q=1, V=1, zg=1, zd=1, rp=1, col=1, bp=1, e2c=1, e2r=1, ht=1, N=64, E=100, D=32, src_rows=64, ldp=None, ldq=None,
        ldv=None, ldz=None):
    return capi.lib().hcspmm_forward_gated(_vp(P), ldp or D, _vp(Q), ldq or D, _vp(V), ldv or D, src_rows, _vp(zg), _vp(zd),
                                           ldz or D, _vp(rp), _vp(col), _vp(bp), _vp(e2c), _vp(e2r), _vp(ht), ctypes.c_void_p(0), None,
                                           N, E, D, ctypes.c_void_p(0), 0, ctypes.c_void_p(0))


@pytest.mark.parametrize("case", [dict(P=0), dict(Q=0), dict(V=0), dict(zg=0, zd=0), dict(ldp=16), dict(ldq=16), dict(ldv=16),
                                  dict(ldz=16), dict(D=0), dict(D=-4), dict(N=-1), dict(E=-1), dict(src_rows=-1), dict(src_rows=0),
                                  dict(rp=0), dict(col=0), dict(bp=0), dict(ht=0), dict(e2c=0), dict(e2r=0)])
def test_forward_gated_argument_checks(case):
    assert _fg(**case) == capi.EINVAL


def test_forward_gated_nothing_to_do_and_nullable_outputs():
    assert _fg(N=0) == 0  # no rows, no launch
    assert _fg(N=0, zd=0) == 0 and _fg(N=0, zg=0) == 0  # either single output is a valid call
    assert _fg(N=0, zg=0, zd=0) == capi.EINVAL  # ... both NULL never is
    assert _fg(N=0, P=0, Q=0, V=0, E=0) == 0  # no rows to serve: the operands are not looked at


# ------------------------------------------------------------------------------------------- register budget
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
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def _expected(name):
    """(pinned occupancy, floats per lane, (kernel, outputs, L, VEC)) of a kernel of the unit"""
    for kernel, table in (("gated_plan_kernel", PLAN_OCC), ("gated_window_kernel", WINDOW_OCC)):
        m = re.search(r"\d+%sILi(\d+)ELi(\d+)ELi(\d+)ELi\d+EE" % kernel, name)
        if m:
            out, L, vec = (int(x) for x in m.groups())
            return table[out][(L, vec)], vec, (kernel, out, L, vec)
    m = re.search(r"\d+fixup_kernelINS_3F32ELi(\d+)EE", name)
    if m:
        return FIXUP_OCC[int(m.group(1))], int(m.group(1)), ("fixup_kernel", int(m.group(1)))
    return None


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_gated_kernels_keep_their_budgets():
    """three output sets x (L = 4 ... 64 at 16-byte lanes, L = 4 at 8- / 4-byte lanes) x (planned, plan-free) and the binary
    fix-up pass's three builds: no scratch anywhere, occupancy as pinned above, at least four waves per SIMD on every
    16-byte-lane build -- and an absent output costs no register: no single-output build takes more than the two-output one"""
    usage = _usage("spmm_gated.hip")
    assert len(usage) == 3 * len(BUILDS) * 2 + 3, sorted(usage)
    seen, vgprs = set(), {}
    for name, v in usage.items():
        want = _expected(name)
        assert want is not None, name
        print(want[2], v)
        assert (v["scratch"], v["occupancy"]) == (0, want[0]), (name, v)
        if want[1] == 4:
            assert v["occupancy"] >= 4, (name, v)
        seen.add(want[2])
        vgprs[want[2]] = v["vgprs"]
    assert seen == ({(k, o, L, vec) for k in ("gated_plan_kernel", "gated_window_kernel") for o in (1, 2, 3) for (L, vec) in BUILDS}
                    | {("fixup_kernel", vec) for vec in (4, 2, 1)})
    for k in ("gated_plan_kernel", "gated_window_kernel"):
        for (L, vec) in BUILDS:
            assert max(vgprs[(k, 1, L, vec)], vgprs[(k, 2, L, vec)]) <= vgprs[(k, 3, L, vec)], (k, L, vec)


def test_the_unit_walks_through_the_schedule_header():
    text = open(os.path.join(CSRC, "spmm_gated.hip")).read()
    assert "csr_plan_walk<" in text and "csr_window_walk<" in text and "csr_launch(" in text and "csr_dispatch(" in text
    assert "fixup_of_slot(" in text and "plan_launch_layout" not in text and "pick_L" not in text and not re.search(r"atomic\w*\(", text)
    assert "spmm_gated.o" in open(os.path.join(CSRC, "Makefile")).read()
    # the pinned units stay as they were: the new kernels live in their own unit
    for unit in os.listdir(CSRC):
        if unit.endswith((".hip", "_impl.h")) and unit not in ("spmm_gated.hip", "capi.hip"):
            body = open(os.path.join(CSRC, unit)).read()
            assert "GatedArgs" not in body and "gated_" not in body, unit


# ------------------------------------------------------------------------------------------- driver and layer
def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _driver():
    _pkg_imports()
    spec = importlib.util.spec_from_file_location("hc_spmm_main_resgated", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_resgated_flags():
    mod = _driver()
    args = mod.parse_args(["--model", "resgated"])
    assert (args.model, args.norm, args.heads, args.fp8, args.directed) == ("resgated", "none", 1, False, False)
    assert mod.parse_args(["--model", "resgated", "--directed"]).directed
    assert mod.parse_args(["--model", "resgated", "--heads", "1"]).heads == 1
    for extra in (["--norm", "sym"], ["--norm", "mean"], ["--aggr", "max"], ["--aggr", "mean"], ["--fp8"], ["--fp8", "--norm", "sym"],
                  ["--heads", "2"], ["--gat-concat"]):
        with pytest.raises(SystemExit):
            mod.parse_args(["--model", "resgated"] + extra)
    # the existing models parse as before
    for model in ("gcn", "gin", "gine", "gat", "gatv2", "sage", "pna", "gen"):
        assert mod.parse_args(["--model", model]).model == model
    assert mod.parse_args([]).model == "gcn"
    assert mod.parse_args(["--model", "sage"]).aggr == "max"
    assert mod.parse_args(["--model", "gcn", "--norm", "sym"]).norm == "sym"
    assert mod.parse_args(["--model", "gat", "--heads", "4"]).heads == 4
    assert mod.parse_args(["--model", "gen", "--gen-t", "0.25"]).gen_t == 0.25
    assert mod.parse_args(["--model", "gcn", "--norm", "sym", "--fp8", "--classes", "24"]).fp8
    with pytest.raises(SystemExit):
        mod.parse_args(["--model", "gen", "--aggr", "max"])
    with pytest.raises(SystemExit):
        mod.parse_args(["--model", "resgate"])


def test_resgatedgraphconv_parameters_and_refusals():
    _pkg_imports()
    import GNN_model
    conv = GNN_model.ResGatedGraphConv(24, 16)
    assert conv.weights.shape == (24, 64) and {n for n, _ in conv.named_parameters()} == {"weights"}
    assert conv.weights.abs().max() <= 1 / 4 and not conv.directed
    lean = GNN_model.ResGatedGraphConv(24, 16, directed=True, root_weight=False, bias=True)
    assert lean.weights.shape == (24, 48) and lean.bias.shape == (16,) and lean.directed
    assert {n for n, _ in lean.named_parameters()} == {"weights", "bias"} and (lean.bias == 0).all()
    placeholders = [torch.zeros(1, dtype=torch.int32)] * 8
    with pytest.raises(ValueError, match="edge_weight"):  # before anything is launched: CPU tensors never reach a kernel
        conv(torch.zeros(4, 24), *placeholders, None, edge_weight=torch.ones(3))


# ---- the arithmetic around the launches, with a torch stand-in for forward_gated ---------------------------------------------
def _rows(rp):
    n = rp.numel() - 1
    return torch.repeat_interleave(torch.arange(n), (rp[1:] - rp[:-1]).long())


class _StandIn:
    """HCSPMM.forward_gated from index_add, in the dtype of its inputs; records what each call asked for"""

    def __init__(self):
        self.asked = []

    def forward_gated(self, P, Q, V, rp, col, *rest):
        outputs = tuple(rest[-1])
        self.asked.append(outputs)
        n, D = rp.numel() - 1, Q.size(1)
        rows, c = _rows(rp), col.long()
        s = torch.sigmoid(P[rows] + Q[c])
        zero = torch.zeros(n, D, dtype=Q.dtype)
        return (zero.index_add(0, rows, s * V[c]) if "gate" in outputs else None,
                zero.index_add(0, rows, s * (1 - s) * V[c]) if "dgate" in outputs else None)


def _graph40(symmetric, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    n = 40
    A = (rng.random((n, n)) < 0.12).astype(np.float64)
    if symmetric:
        A = np.maximum(A, A.T)
    A[::9] = 0  # rows without entries
    if symmetric:
        A[:, ::9] = 0

    def tensors(B):
        r, c = np.nonzero(B)
        rp = np.zeros(n + 1, np.int32)
        np.add.at(rp, r + 1, 1)
        return (torch.from_numpy(np.cumsum(rp).astype(np.int32)), torch.from_numpy(c.astype(np.int32))) + \
            (torch.zeros(1, dtype=torch.int32),) * 6

    return torch.from_numpy(A), tensors(A), tensors(A.T)


@pytest.fixture
def gnn(monkeypatch):
    _pkg_imports()
    import GNN_model
    stand_in = _StandIn()
    monkeypatch.setattr(GNN_model.HCSPMM, "forward_gated", stand_in.forward_gated, raising=True)
    monkeypatch.setattr(GNN_model, "transpose_permutation_i32", lambda rp, col: None)
    stand_in.transposed = {}  # id(row_pointers of A) -> the graph tensors of A^T
    monkeypatch.setattr(GNN_model, "transposed_graph", lambda graph: stand_in.transposed[id(graph[0])])
    return GNN_model, stand_in


@pytest.mark.parametrize("needs", [(True, True, True), (False, True, True), (True, False, False), (False, False, True),
                                   (False, True, False)])
@pytest.mark.parametrize("symmetric", [True, False])
def test_gated_aggregate_gradients_match_the_dense_formula(gnn, symmetric, needs):
    """dP = G T, and dV = Y_gate, dQ = V Y_dgate of one call on the walked graph with own rows Q and gathered (P, G), against
    autograd of the dense formula in fp64 -- on strided column blocks of one buffer, as the layer passes them.  The forward asks
    for the second output only when P needs a gradient, the backward only for what is needed."""
    GNN_model, stand_in = gnn
    A, graph, graph_t = _graph40(symmetric, 11)
    stand_in.transposed[id(graph[0])] = graph_t
    torch.manual_seed(12)
    D = 5
    proj = torch.randn(40, 3 * D, dtype=torch.float64)
    ops = [proj[:, k * D:(k + 1) * D].clone().requires_grad_(n) for k, n in enumerate(needs)]
    Z = GNN_model.gated_aggregate(*ops, graph, directed=not symmetric)
    assert stand_in.asked[-1] == (("gate", "dgate") if needs[0] else ("gate",))
    dZ = torch.randn(40, D, dtype=torch.float64)
    Z.backward(dZ)
    if needs[1] or needs[2]:
        assert stand_in.asked[-1] == (("gate",) if needs[2] else ()) + (("dgate",) if needs[1] else ())
    else:
        assert len(stand_in.asked) == 1  # dP needs no launch
    ref = [o.detach().clone().requires_grad_(n) for o, n in zip(ops, needs)]
    Pr, Qr, Vr = ref
    Zr = (A[:, :, None] * torch.sigmoid(Pr[:, None, :] + Qr[None, :, :]) * Vr[None, :, :]).sum(1)
    Zr.backward(dZ)
    torch.testing.assert_close(Z.detach(), Zr.detach(), rtol=1e-12, atol=1e-12)
    for o, r, n in zip(ops, ref, needs):
        if n:
            torch.testing.assert_close(o.grad, r.grad, rtol=1e-11, atol=1e-12)
        else:
            assert o.grad is None


def test_resgatedgraphconv_is_the_stated_formula(gnn, monkeypatch):
    """out = X W_s + sum_j sigmoid(X_i W_k + X_j W_q) * X_j W_v (+ bias), the blocks of ONE product in that order; without
    root_weight the X W_s term is gone"""
    GNN_model, stand_in = gnn
    monkeypatch.setattr(GNN_model, "_mm", lambda a, b: a @ b)
    monkeypatch.setattr(GNN_model, "_weight_grad", lambda a, b: a.t() @ b)
    A, graph, _ = _graph40(True, 13)
    torch.manual_seed(14)
    X = torch.randn(40, 6, dtype=torch.float64)
    for root, bias in ((True, False), (False, True)):
        conv = GNN_model.ResGatedGraphConv(6, 4, root_weight=root, bias=bias).double()
        if bias:
            conv.bias.data.uniform_(-1, 1)
        out = conv(X, *graph, None)
        W = conv.weights.detach()
        K, Q, V = (X @ W[:, k * 4:(k + 1) * 4] for k in range(3))
        want = (A[:, :, None] * torch.sigmoid(K[:, None, :] + Q[None, :, :]) * V[None, :, :]).sum(1)
        if root:
            want = want + X @ W[:, 12:]
        if bias:
            want = want + conv.bias.detach()
        torch.testing.assert_close(out.detach(), want, rtol=1e-12, atol=1e-12)
