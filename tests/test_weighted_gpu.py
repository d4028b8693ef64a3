"""Edge-weighted aggregation Z = A_w X (hcspmm_forward_weighted) on an MI355X, through both Python front-ends.

The contract (include/hcspmm.h): every step is acc = fmaf(values[e], x, acc) in the order the binary forward adds that row.
What follows from it, and what this file checks on every plan form:
  1. values == 1 gives forward's bits (fp32, fp16, bf16);
  2. values[e] = 2^(a_row + b_col) gives the bits of 2^a * forward(2^b * X) -- a wrong entry -> value mapping on any
     sub-path (wide, sliced, tiny segments, dense windows, panels) changes them;
  3. with exact products, rows summed in CSR order equal a sequential fp32 sum in CSR order, bit for bit;
  4. full-precision values stay within gamma_n * sum |v x| of the fp64 product.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import frontends
from hcspmm import graphs

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


def _graph(kind):
    if kind == "powerlaw":  # hubs: wide tasks, split rows
        return graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    if kind == "planted":  # dense-tile windows of every record kind
        return graphs.planted_dense_graph(2400, seed=4)
    if kind == "community":
        return graphs.community_graph(2500, 20000, seed=5)[:2]
    if kind == "molecule":  # short rows: tiny tasks
        return graphs.molecule_graph(3000, seed=6)
    return graphs.uniform_graph(2000, 16000, seed=7)


# plan forms, set by explicit plan parameters (never the environment)
PLANS = {
    "default": {},
    "no_slices": dict(slice_threshold=-1),
    "slices": dict(slice_threshold=16, n_slices=8),
    "sparse": dict(force=0),
    "dense": dict(force=1),
    "tiny_segments": dict(split_threshold=9, segment_len=7),  # rows of 8, 9, 15, 16 ... entries end in 1-2 entry segments
    "panel32": dict(panel_cols=32),
    "panel64": dict(panel_cols=64),
    "plan_free": dict(plan=False),
}

_CACHE = {}


def _setup(fe, dev, kind, form):
    key = (fe.name, kind, form)
    if key in _CACHE:
        return _CACHE[key]
    rp, col = _graph(kind)
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    bp, e2c, e2r, ht, row_nzr, col_nzr = fe.preprocess(col_d, rp_d, N, E, (N + 15) // 16, rule=3)
    p = dict(PLANS[form])
    force = p.pop("force", None)
    plan = p.pop("plan", True)
    if force is not None:
        ht = torch.full_like(ht, force)
    if not plan:
        row_nzr = torch.zeros(1, dtype=torch.int32, device=dev)
    elif force is not None or p:
        row_nzr = fe.build_plan(rp_d, col_d, bp, e2c, ht, **p)
    g = dict(rp=rp, col=col, N=N, E=E, ht=ht.cpu().numpy(), args=(rp_d, col_d, bp, e2c, e2r, ht, row_nzr, col_nzr), plan=plan,
             p=p)
    _CACHE[key] = g
    return g


def _rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


WIDTHS = [1, 2, 3, 4, 16, 22, 32, 64, 128, 256]
KINDS = ["powerlaw", "planted", "community", "molecule", "uniform"]


@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_ones_match_binary_forward_bitwise(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    ones = torch.ones(g["E"], dtype=torch.float32, device=dev)
    rng = np.random.default_rng(11)
    for D in WIDTHS:
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            if dt != torch.float32 and D not in (2, 3, 22, 64, 128):
                continue
            X = torch.from_numpy(rng.standard_normal((g["N"], D)).astype(np.float32)).to(dev).to(dt)
            want = fe.forward(X, *g["args"])[0]
            got = fe.forward_weighted(X, ones, *g["args"])[0]
            assert got.dtype == dt
            assert torch.equal(got.view(torch.int16 if dt != torch.float32 else torch.int32),
                               want.view(torch.int16 if dt != torch.float32 else torch.int32)), (kind, form, D, dt)


@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_power_of_two_values_map_every_entry(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    rng = np.random.default_rng(12)
    a = rng.integers(-3, 4, g["N"])
    b = rng.integers(-3, 4, g["N"])
    rows = _rows_of(g["rp"])
    vals = np.ldexp(np.ones(g["E"], np.float32), a[rows] + b[g["col"]]).astype(np.float32)
    vals_d = torch.from_numpy(vals).to(dev)
    sa = torch.from_numpy(np.ldexp(np.ones(g["N"]), a).astype(np.float32)).to(dev)[:, None]
    sb = torch.from_numpy(np.ldexp(np.ones(g["N"]), b).astype(np.float32)).to(dev)[:, None]
    for D in WIDTHS:
        for dt in ((torch.float32, torch.bfloat16) if D in (22, 128) else (torch.float32,)):
            X = torch.from_numpy(rng.standard_normal((g["N"], D)).astype(np.float32)).to(dev)
            want = (sa * fe.forward((sb * X).to(dt), *g["args"])[0].float()).to(dt)
            got = fe.forward_weighted(X.to(dt), vals_d, *g["args"])[0]
            assert torch.equal(got, want), (kind, form, D, dt, (got.float() - want.float()).abs().max().item())


def _short(rng, shape, bits):
    """values with at most `bits` significant bits, exponents in a narrow range (every product exact in fp32)"""
    m = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), shape)
    return np.ldexp(m.astype(np.float64), rng.integers(-bits - 2, -bits + 3, shape)).astype(np.float32)


@pytest.mark.parametrize("form", ["no_slices", "sparse", "dense", "panel32", "plan_free"])
@pytest.mark.parametrize("kind", KINDS)
def test_exact_products_sum_in_csr_order(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    rng = np.random.default_rng(13)
    rp, col, N = g["rp"], g["col"], g["N"]
    vals = _short(rng, g["E"], 8)
    deg = np.diff(rp)
    for D in (4, 32, 128):
        X = _short(rng, (N, D), 12)
        got = fe.forward_weighted(torch.from_numpy(X).to(dev), torch.from_numpy(vals).to(dev), *g["args"])[0].cpu().numpy()
        want = np.zeros((N, D), np.float32)
        for k in range(int(deg.max()) if len(deg) else 0):  # sequential fp32 sum, one CSR position at a time
            r = np.nonzero(deg > k)[0]
            e = rp[r] + k
            want[r] = (want[r] + vals[e][:, None] * X[col[e]]).astype(np.float32)  # products exact, one rounding per add
        # rows the kernels add in CSR order: not wide (whole-wave tree) and not split (fix-up)
        thr = fe.wide_threshold(g["args"][6], D) if g["plan"] else 64
        ordered = deg <= min(thr, 256)
        assert np.array_equal(got[ordered].view(np.int32), want[ordered].view(np.int32)), (kind, form, D)


@pytest.mark.parametrize("form", ["default", "slices", "tiny_segments", "plan_free"])
@pytest.mark.parametrize("kind", KINDS)
def test_full_precision_values_within_the_fma_bound(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    rng = np.random.default_rng(14)
    rp, col, N = g["rp"], g["col"], g["N"]
    vals = rng.standard_normal(g["E"]).astype(np.float32)
    rows = _rows_of(rp)
    deg = np.diff(rp).astype(np.float64)
    for D in (3, 32, 64):
        X = rng.standard_normal((N, D)).astype(np.float32)
        got = fe.forward_weighted(torch.from_numpy(X).to(dev), torch.from_numpy(vals).to(dev), *g["args"])[0].cpu().numpy()
        prod = vals.astype(np.float64)[:, None] * X[col].astype(np.float64)
        exact = np.zeros((N, D))
        absum = np.zeros((N, D))
        np.add.at(exact, rows, prod)
        np.add.at(absum, rows, np.abs(prod))
        u = 2.0 ** -24
        gamma = (deg * u / (1 - deg * u))[:, None]
        assert np.all(np.abs(got - exact) <= gamma * absum), (kind, form, D)


def test_values_are_read_on_every_call(fe, dev):
    g = _setup(fe, dev, "powerlaw", "default")
    X = torch.randn(g["N"], 32, device=dev)
    v1 = torch.rand(g["E"], device=dev)
    z1 = fe.forward_weighted(X, v1, *g["args"])[0].clone()
    v1.mul_(2.0)  # in place: the same tensor, the same plan
    z2 = fe.forward_weighted(X, v1, *g["args"])[0]
    assert torch.equal(z2, 2.0 * z1)
    v3 = torch.rand(g["E"], device=dev)
    z3 = fe.forward_weighted(X, v3, *g["args"])[0]
    assert torch.equal(z3, fe.forward_weighted(X, v3.clone(), *g["args"])[0]) and not torch.equal(z3, z1)


def test_weighted_forward_replays_in_a_hip_graph(fe, dev):
    g = _setup(fe, dev, "planted", "default")
    X = torch.randn(g["N"], 64, device=dev)
    vals = torch.rand(g["E"], device=dev)
    ref = fe.forward_weighted(X, vals, *g["args"])[0]  # warm-up: plan registry and fingerprint checks happen here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fe.forward_weighted(X, vals, *g["args"])[0]
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    vals.copy_(torch.rand(g["E"], device=dev))
    X.copy_(torch.randn(g["N"], 64, device=dev))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fe.forward_weighted(X, vals, *g["args"])[0])


def test_bad_values_are_refused(fe, dev):
    g = _setup(fe, dev, "uniform", "default")
    X = torch.randn(g["N"], 16, device=dev)
    E = g["E"]
    with pytest.raises(RuntimeError, match="values must be a CUDA tensor"):
        fe.forward_weighted(X, torch.ones(E), *g["args"])
    with pytest.raises(RuntimeError, match="values must be a float32 tensor"):
        fe.forward_weighted(X, torch.ones(E, dtype=torch.float64, device=dev), *g["args"])
    with pytest.raises(RuntimeError, match="values must hold one float32 per stored entry"):
        fe.forward_weighted(X, torch.ones(E - 1, device=dev), *g["args"])
    with pytest.raises(RuntimeError, match="values must be contiguous"):
        fe.forward_weighted(X, torch.ones(2 * E, device=dev)[::2], *g["args"])


def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


@pytest.mark.parametrize("norm", ["sym", "mean"])
@pytest.mark.parametrize("model", ["gcn", "gin"])
def test_weighted_layers_match_fp64_autograd(dev, model, norm):
    _pkg_imports()
    import GNN_model
    import HCSPMM
    rp, col = graphs.powerlaw_graph(1500, 20000, seed=21, max_degree_frac=0.2)
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    graph = HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16, -1)
    args = (rp_d, col_d) + tuple(graph)
    ew = HCSPMM.edge_norm(rp_d, col_d, norm)
    conv = (GNN_model.GCNConv if model == "gcn" else GNN_model.GINConv)(24, 16, 0).to(dev)
    X = torch.randn(N, 24, device=dev, requires_grad=True)
    Y = conv(X, *args, None, edge_weight=ew)
    G = torch.randn_like(Y)
    (Y * G).sum().backward()
    A = torch.sparse_csr_tensor(torch.from_numpy(rp).long(), torch.from_numpy(col).long(), ew.cpu().double(), (N, N)).to_dense()
    X64 = X.detach().cpu().double().requires_grad_(True)
    W64 = conv.weights.detach().cpu().double().requires_grad_(True)
    Y64 = (A @ X64) @ W64 if model == "gin" else A @ (X64 @ W64)
    (Y64 * G.cpu().double()).sum().backward()
    for got, want in ((Y, Y64), (X.grad, X64.grad), (conv.weights.grad, W64.grad)):
        got = got.detach().cpu().double()
        assert torch.allclose(got, want.detach(), rtol=1e-4, atol=1e-4 * want.abs().max().item()), (model, norm)


def test_values_gradient_is_refused(dev):
    _pkg_imports()
    import GNN_model
    import HCSPMM
    rp, col = graphs.powerlaw_graph(200, 1000, seed=2)  # (symmetric: the transpose permutation exists)
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    args = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16, -1))
    ew = torch.rand(E, device=dev, requires_grad=True)
    with pytest.raises(NotImplementedError, match="SDDMM"):
        GNN_model.weighted_aggregate(torch.randn(N, 8, device=dev), ew, args)


def test_edge_norm_on_the_device_matches_numpy(fe, dev):
    rp, col = graphs.powerlaw_graph(2000, 30000, seed=8)
    deg = np.diff(rp).astype(np.float64)
    rows = _rows_of(rp)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    sym = fe.edge_norm(rp_d, col_d, "sym").cpu().numpy()
    mean = fe.edge_norm(rp_d, col_d, "mean").cpu().numpy()
    assert np.array_equal(sym, (np.float32(1) / np.sqrt((deg[rows] * deg[col]).astype(np.float32))).astype(np.float32))
    assert np.array_equal(mean, (np.float32(1) / deg[rows].astype(np.float32)))


@pytest.mark.parametrize("norm", ["sym", "mean"])
def test_driver_trains_with_normalised_aggregation(norm, capsys, monkeypatch):
    _pkg_imports()
    monkeypatch.chdir(PKG)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_norm", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    net = mod.main(["--dataset", "example", "--dim", "16", "--num_layers", "3", "--hidden", "32", "--classes", "22",
                    "--epochs", "20", "--model", "gcn", "--norm", norm])
    out = capsys.readouterr().out
    assert "Train (ms/epoch):" in out
    for name, prm in net.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
