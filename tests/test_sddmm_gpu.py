"""SDDMM, edge softmax and the layers built on them (include/hcspmm.h hcspmm_sddmm, hcspmm_edge_softmax*; GNN_model
edge_weighted_aggregate, EdgeSoftmax, GATConv) on an MI355X, through both Python front-ends.

  * sddmm(A, B, *graph)[e] = <A[row(e)], B[col(e)]>: within (D + 1) 2^-24 sum |a b| of fp64 on the widened inputs, exact
    for small integers, the same bits on every call and through both front-ends, every entry written exactly once;
  * edge softmax forward and backward against fp64, on a graph with a 50 000-entry row and rows of one entry;
  * A_w X with the gradient for both operands, and a GAT layer, against fp64 autograd over dense matrices.
"""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import frontends
from hcspmm import capi, graphs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hc-spmm_amd")


@pytest.fixture(scope="module", params=["ctypes", "extension"])
def fe(request):
    return frontends.get(request.param)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _csr(N, rows, cols):
    """CSR of the unique (row, col) pairs, columns ascending"""
    key = np.unique(rows.astype(np.int64) * (1 << 31) + cols.astype(np.int64))
    r, c = key >> 31, key & ((1 << 31) - 1)
    rp = np.zeros(N + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=N), out=rp[1:])
    return rp, c.astype(np.int32)


def _symmetrized(rp, col):
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return _csr(len(rp) - 1, np.concatenate([rows, col]), np.concatenate([col, rows]))


def _graph(kind):
    """-> (row_pointers, column_index, b_rows)"""
    if kind == "powerlaw":  # hubs
        return graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3) + (3000,)
    if kind == "planted":
        return graphs.planted_dense_graph(2400, seed=4) + (2400,)
    if kind == "community":
        return graphs.community_graph(2500, 20000, seed=5)[:2] + (2500,)
    if kind == "molecule":
        return graphs.molecule_graph(3000, seed=6) + (3000,)
    if kind == "uniform":
        return graphs.uniform_graph(2000, 16000, seed=7) + (2000,)
    rng = np.random.default_rng(8)
    if kind == "rect":  # a row block: 1500 rows, columns index 5000 rows of B
        N, M = 1500, 5000
        rows = rng.integers(0, N, 30000)
        rows[:2000] = 7  # one long row
        return _csr(N, rows, rng.integers(0, M, 30000)) + (M,)
    # empty rows among the others and a trailing run of them
    N = 2000
    rows = rng.integers(0, 1500, 12000)
    rows = rows[(rows % 7) != 3]
    return _csr(N, rows, rng.integers(0, N, len(rows))) + (N,)


KINDS = ["powerlaw", "planted", "community", "molecule", "uniform", "rect", "empty_rows"]
WIDTHS = [1, 2, 3, 4, 7, 8, 16, 22, 32, 33, 64, 128, 256, 520]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]

_CACHE = {}


def _setup(fe, dev, kind):
    key = (fe.name, kind)
    if key not in _CACHE:
        rp, col, M = _graph(kind)
        N, E = len(rp) - 1, len(col)
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        pre = fe.preprocess(col_d, rp_d, N, E, (N + 15) // 16, rule=3, num_columns=M if M != N else None)
        rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).to(dev)
        _CACHE[key] = dict(rp=rp, col=col, N=N, E=E, M=M, args=(rp_d, col_d) + tuple(pre), rows=rows, cols=col_d.long())
    return _CACHE[key]


def _operand(rng, n, D, dt, dev, strided, integers):
    """[n, D] of dtype dt; strided: a column slice of a wider matrix (row stride D + 5, starting at column 2)"""
    w = D + 5 if strided else D
    if integers:
        full = rng.integers(-8, 9, (n, w)).astype(np.float32)
    else:
        full = rng.standard_normal((n, w)).astype(np.float32)
    t = torch.from_numpy(full).to(dev).to(dt)
    return t[:, 2:2 + D] if strided else t


def _fp64(g, A, B):
    A64, B64 = A.double(), B.double()
    prod = A64[g["rows"]] * B64[g["cols"]]
    return prod.sum(1), prod.abs().sum(1)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_sddmm_matches_fp64(fe, dev, kind, dt, strided):
    g = _setup(fe, dev, kind)
    other = frontends.get("extension" if fe.name == "ctypes" else "ctypes")
    rng = np.random.default_rng(KINDS.index(kind) * 10 + DTYPES.index(dt) * 2 + int(strided))
    for D in WIDTHS:
        A = _operand(rng, g["N"], D, dt, dev, strided, False)
        B = _operand(rng, g["M"], D, dt, dev, strided, False)
        got = fe.sddmm(A, B, *g["args"])
        assert got.dtype == torch.float32 and got.shape == (g["E"],)
        want, absum = _fp64(g, A, B)
        bound = (D + 1) * 2.0 ** -24 * absum
        assert bool(((got.double() - want).abs() <= bound).all()), (kind, dt, strided, D)
        again = fe.sddmm(A, B, *g["args"])
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (kind, dt, strided, D)
        theirs = other.sddmm(A, B, *g["args"])
        assert torch.equal(got.view(torch.int32), theirs.view(torch.int32)), (kind, dt, strided, D)
        Ai = _operand(rng, g["N"], D, dt, dev, strided, True)
        Bi = _operand(rng, g["M"], D, dt, dev, strided, True)
        assert torch.equal(fe.sddmm(Ai, Bi, *g["args"]).double(), _fp64(g, Ai, Bi)[0]), (kind, dt, strided, D)


def test_sddmm_plan_free_matches_planned(fe, dev):
    g = _setup(fe, dev, "powerlaw")
    placeholder = torch.zeros(1, dtype=torch.int32, device=dev)
    args = g["args"][:6] + (placeholder, g["args"][7])
    for D in (8, 128):
        A, B = torch.randn(g["N"], D, device=dev), torch.randn(g["N"], D, device=dev)
        assert torch.equal(fe.sddmm(A, B, *args), fe.sddmm(A, B, *g["args"]))


def _c_sddmm(A, B, out_ptr, g, dt):
    """plan-free C-ABI call into a caller's buffer"""
    rp_d, col_d = g["args"][0], g["args"][1]
    return capi.lib().hcspmm_sddmm(ctypes.c_void_p(A.data_ptr()), A.stride(0), ctypes.c_void_p(B.data_ptr()), B.size(0),
                                   B.stride(0), {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[dt], out_ptr,
                                   ctypes.c_void_p(rp_d.data_ptr()), ctypes.c_void_p(col_d.data_ptr()), ctypes.c_void_p(0),
                                   None, g["N"], g["E"], A.size(1),
                                   ctypes.c_void_p(torch.cuda.current_stream(A.device).cuda_stream))


@pytest.mark.parametrize("kind", ["powerlaw", "empty_rows", "rect"])
def test_sddmm_writes_every_entry_and_nothing_else(dev, kind):
    fe = frontends.get("ctypes")
    g = _setup(fe, dev, kind)
    E = g["E"]
    for D, dt in ((3, torch.float32), (22, torch.bfloat16), (128, torch.float32), (520, torch.float16)):
        A, B = torch.randn(g["N"], D, device=dev).to(dt), torch.randn(g["M"], D, device=dev).to(dt)
        buf = torch.full((E + 2,), float("nan"), device=dev)
        sentinel = buf.view(torch.int32)
        sentinel[0] = 0x7fc00123
        sentinel[E + 1] = 0x7fc00456
        rc = _c_sddmm(A, B, ctypes.c_void_p(buf.data_ptr() + 4), g, dt)
        torch.cuda.synchronize()
        assert rc == 0
        assert int(sentinel[0]) == 0x7fc00123 and int(sentinel[E + 1]) == 0x7fc00456, (kind, D, dt)
        assert not bool(torch.isnan(buf[1:E + 1]).any()), (kind, D, dt)
        assert torch.equal(buf[1:E + 1], fe.sddmm(A, B, *g["args"]))


def test_sddmm_replays_in_a_hip_graph(fe, dev):
    g = _setup(fe, dev, "powerlaw")
    A, B = torch.randn(g["N"], 64, device=dev), torch.randn(g["N"], 64, device=dev)
    ref = fe.sddmm(A, B, *g["args"])  # warm-up: plan registry and fingerprint checks happen here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fe.sddmm(A, B, *g["args"])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    A.copy_(torch.randn_like(A))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fe.sddmm(A, B, *g["args"]))


def test_sddmm_refuses_a_plan_that_gathers_rows_b_lacks(fe, dev):
    g = _setup(fe, dev, "rect")
    A = torch.randn(g["N"], 16, device=dev)
    B = torch.randn(g["M"] - 1, 16, device=dev)
    with pytest.raises(RuntimeError, match="rows but the plan gathers from"):
        fe.sddmm(A, B, *g["args"])
    h = frontends.get("ctypes").header(g["args"][6])
    if fe.name == "ctypes":
        rc = capi.lib().hcspmm_sddmm(ctypes.c_void_p(A.data_ptr()), 16, ctypes.c_void_p(B.data_ptr()), B.size(0), 16, 0,
                                     ctypes.c_void_p(B.data_ptr()), ctypes.c_void_p(g["args"][0].data_ptr()),
                                     ctypes.c_void_p(g["args"][1].data_ptr()), ctypes.c_void_p(g["args"][6].data_ptr()),
                                     ctypes.byref(h), g["N"], g["E"], 16, None)
        assert rc == capi.EINVAL


# ------------------------------------------------------------------------------------------- edge softmax
def _softmax_graph():
    """row 0: 50 000 entries; rows of one entry; empty rows; the rest 2-40 entries"""
    rng = np.random.default_rng(31)
    N = 60000
    rows = [np.zeros(50000, np.int64)]
    cols = [rng.permutation(N)[:50000]]
    lens = rng.integers(0, 41, N)
    lens[0] = 0
    lens[1:4000] = 1
    lens[5000:6000] = 0
    r = np.repeat(np.arange(N), lens)
    rows.append(r)
    cols.append(rng.integers(0, N, len(r)))
    return _csr(N, np.concatenate(rows), np.concatenate(cols))


def _segment_softmax64(x, rows, N):
    """fp64 per-row softmax of x [heads, E] with torch ops (autograd-able)"""
    idx = rows.expand_as(x)
    m = torch.full((x.size(0), N), -float("inf"), dtype=x.dtype, device=x.device).scatter_reduce(1, idx, x, "amax")
    ex = torch.exp(x - m.gather(1, idx))
    s = torch.zeros((x.size(0), N), dtype=x.dtype, device=x.device).scatter_add(1, idx, ex)
    return ex / s.gather(1, idx)


@pytest.fixture(scope="module")
def sm_graph(dev):
    rp, col = _softmax_graph()
    N = len(rp) - 1
    assert np.diff(rp).max() >= 50000 and (np.diff(rp) == 1).sum() > 1000
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).to(dev)
    return dict(rp=torch.from_numpy(rp).to(dev), N=N, E=len(col), rows=rows)


@pytest.mark.parametrize("heads", [1, 4])
def test_edge_softmax_matches_fp64(fe, dev, sm_graph, heads):
    g = sm_graph
    gen = torch.Generator(device=dev).manual_seed(heads)
    x = (torch.rand((heads, g["E"]), device=dev, generator=gen) * 160 - 80)
    logits = x[0] if heads == 1 else x
    alpha = fe.edge_softmax(logits, g["rp"])
    assert alpha.shape == logits.shape and alpha.dtype == torch.float32
    want = _segment_softmax64(x.double(), g["rows"], g["N"])
    err = (alpha.reshape(heads, -1).double() - want).abs()
    assert bool((err <= 1e-5 * want + 2.0 ** -126).all()), float((err / want.clamp_min(1e-300)).max())
    assert torch.equal(alpha, fe.edge_softmax(logits, g["rp"]))
    other = frontends.get("extension" if fe.name == "ctypes" else "ctypes")
    assert torch.equal(alpha, other.edge_softmax(logits, g["rp"]))

    grad_alpha = torch.randn((heads, g["E"]), device=dev, generator=gen)
    ga = grad_alpha[0] if heads == 1 else grad_alpha
    got = fe.edge_softmax_backward(alpha, ga, g["rp"])
    x64 = x.double().requires_grad_(True)
    a64 = _segment_softmax64(x64, g["rows"], g["N"])
    (a64 * grad_alpha.double()).sum().backward()
    idx = g["rows"].expand(heads, -1)
    dot = torch.zeros((heads, g["N"]), dtype=torch.float64, device=dev).scatter_add(1, idx, (a64 * grad_alpha.double()).abs())
    scale = a64.detach() * (grad_alpha.double().abs() + dot.gather(1, idx).detach())
    err = (got.reshape(heads, -1).double() - x64.grad).abs()
    assert bool((err <= 3e-5 * scale + 2.0 ** -126).all())
    assert torch.equal(got, fe.edge_softmax_backward(alpha, ga, g["rp"]))


# ------------------------------------------------------------------------------------------- autograd and layers
def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _layer_graph(dev, kind):
    import HCSPMM
    if kind == "powerlaw":
        rp, col = graphs.powerlaw_graph(1500, 20000, seed=21, max_degree_frac=0.2)
    else:
        rp, col = _symmetrized(*graphs.planted_dense_graph(1600, seed=22))
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    args = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16, -1))
    return rp, col, args


def _close(got, want):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    return bool(((got - want).abs() <= 1e-4 * want.abs().max()).all())


@pytest.mark.parametrize("kind", ["powerlaw", "planted"])
def test_edge_weighted_aggregate_gradients_match_fp64(dev, kind):
    _pkg_imports()
    import GNN_model
    import HCSPMM
    rp, col, args = _layer_graph(dev, kind)
    N, E = len(rp) - 1, len(col)
    X = torch.randn(N, 24, device=dev, requires_grad=True)
    w = torch.rand(E, device=dev, requires_grad=True)
    Y = GNN_model.edge_weighted_aggregate(X, w, args)
    G = torch.randn_like(Y)
    (Y * G).sum().backward()
    assert torch.equal(w.grad, HCSPMM.sddmm(G, X.detach(), *args))
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).long()
    X64 = X.detach().cpu().double().requires_grad_(True)
    w64 = w.detach().cpu().double().requires_grad_(True)
    A = torch.zeros(N, N, dtype=torch.float64).index_put((rows, torch.from_numpy(col).long()), w64)
    Y64 = A @ X64
    (Y64 * G.cpu().double()).sum().backward()
    for got, want in ((Y, Y64), (X.grad, X64.grad), (w.grad, w64.grad)):
        assert _close(got, want), kind


def _torch_gat64(X, W, a_src, a_dst, rows, cols, N, slope):
    outs = []
    for k in range(W.size(0)):
        h = X @ W[k]
        logit = torch.nn.functional.leaky_relu((h @ a_dst[k])[rows] + (h @ a_src[k])[cols], slope)
        alpha = _segment_softmax64(logit[None], rows, N)[0]
        outs.append(torch.zeros(N, h.size(1), dtype=h.dtype).index_add(0, rows, alpha[:, None] * h[cols]))
    return torch.stack(outs).mean(0)


@pytest.mark.parametrize("heads", [1, 4])
def test_gat_layer_matches_fp64_torch(dev, heads):
    _pkg_imports()
    import GNN_model
    rp, col, args = _layer_graph(dev, "powerlaw")
    N = len(rp) - 1
    torch.manual_seed(heads)
    conv = GNN_model.GATConv(24, 16, 0, heads=heads).to(dev)
    X = torch.randn(N, 24, device=dev, requires_grad=True)
    Y = conv(X, *args, None)
    assert Y.shape == (N, 16)
    G = torch.randn_like(Y)
    (Y * G).sum().backward()
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).long()
    cols = torch.from_numpy(col).long()
    leaves = [X.detach().cpu().double().requires_grad_(True)] + \
        [p.detach().cpu().double().requires_grad_(True) for p in (conv.weights, conv.a_src, conv.a_dst)]
    Y64 = _torch_gat64(*leaves, rows, cols, N, conv.negative_slope)
    (Y64 * G.cpu().double()).sum().backward()
    assert _close(Y, Y64)
    for got, want in zip((X.grad, conv.weights.grad, conv.a_src.grad, conv.a_dst.grad), leaves):
        assert _close(got, want.grad), heads
    with pytest.raises(ValueError):
        conv(X, *args, None, edge_weight=torch.ones(len(col), device=dev))


def test_gat_refuses_an_asymmetric_pattern(dev):
    _pkg_imports()
    import GNN_model
    import HCSPMM
    rp, col = graphs.uniform_graph(500, 3000, seed=6)
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    args = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16, -1))
    conv = GNN_model.GATConv(8, 8, 0, heads=2).to(dev)
    with pytest.raises(RuntimeError, match="symmetric"):
        conv(torch.randn(N, 8, device=dev), *args, None)
    with pytest.raises(RuntimeError, match="symmetric"):
        GNN_model.edge_weighted_aggregate(torch.randn(N, 8, device=dev), torch.rand(E, device=dev, requires_grad=True), args)


def _driver():
    _pkg_imports()
    spec = importlib.util.spec_from_file_location("hc_spmm_main_gat", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_trains_gat(capsys, monkeypatch):
    monkeypatch.chdir(PKG)
    mod = _driver()
    losses = []
    nll = mod.nll_loss

    def recording(log_probs, target):
        loss = nll(log_probs, target)
        losses.append(float(loss.detach()))
        return loss

    monkeypatch.setattr(mod, "nll_loss", recording)
    torch.manual_seed(0)
    net = mod.main(["--dataset", "example", "--dim", "16", "--num_layers", "3", "--hidden", "32", "--classes", "22",
                    "--epochs", "20", "--model", "gat", "--heads", "2"])
    assert "Train (ms/epoch):" in capsys.readouterr().out
    assert len(losses) == 29  # 9 warm-up epochs + 20
    assert losses[-1] < losses[0], losses
    assert all(np.isfinite(losses))
    for name, prm in net.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    with pytest.raises(SystemExit):
        mod.parse_args(["--model", "gat", "--norm", "sym"])
