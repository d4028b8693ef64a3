"""Multi-head weighted SpMM and SDDMM (hcspmm_forward_weighted_heads, hcspmm_sddmm_heads) and the concatenating GAT layer
built on them, on an MI355X through both Python front-ends.

The contract (include/hcspmm.h): columns [h*Dh, (h+1)*Dh) of forward_weighted_heads(X, V) are bit for bit
forward_weighted(X, V[h]) at full width, and sddmm_heads(A, B)[h] is bit for bit sddmm on the head's column slices.
Checked on every plan form of test_weighted_gpu.py, at heads 1, 2, 3, 4, 8 and Dh 4 ... 64 (D <= 256).
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


PLANS = {
    "default": {},
    "slices": dict(slice_threshold=16, n_slices=8),
    "sparse": dict(force=0),
    "dense": dict(force=1),
    "tiny_segments": dict(split_threshold=9, segment_len=7),
    "panel32": dict(panel_cols=32),
    "plan_free": dict(plan=False),
}
KINDS = ["powerlaw", "planted", "community", "molecule", "uniform"]
SHAPES = [(h, dh) for h in (1, 2, 3, 4, 8) for dh in (4, 8, 16, 32, 64) if h * dh <= 256]

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
    g = dict(rp=rp, col=col, N=N, E=E, args=(rp_d, col_d, bp, e2c, e2r, ht, row_nzr, col_nzr), plan=plan)
    _CACHE[key] = g
    return g


def _rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_every_head_is_the_single_head_product(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    gen = torch.Generator(device="cpu").manual_seed(21)
    ones = torch.ones(g["E"], device=dev)
    for heads, dh in SHAPES:
        D = heads * dh
        X = torch.randn(g["N"], D, generator=gen).to(dev)
        V = torch.randn(heads, g["E"], generator=gen).to(dev)
        got = fe.forward_weighted_heads(X, V, *g["args"])[0]
        assert got.shape == (g["N"], D)
        for h in range(heads):
            want = fe.forward_weighted(X, V[h].contiguous(), *g["args"])[0]
            assert torch.equal(got[:, h * dh:(h + 1) * dh], want[:, h * dh:(h + 1) * dh]), (kind, form, heads, dh, h)
        if heads == 1:
            assert torch.equal(got, fe.forward_weighted(X, V[0].contiguous(), *g["args"])[0])
        got1 = fe.forward_weighted_heads(X, ones.expand(heads, -1).contiguous(), *g["args"])[0]
        assert torch.equal(got1, fe.forward(X, *g["args"])[0]), (kind, form, heads, dh)


@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_power_of_two_values_map_every_entry_and_head(fe, dev, kind, form):
    """V[h][e] = 2^(a_h[row] + b_h[col]) with other exponents per head: head h's columns are 2^a_h * forward(2^b_h * X) bit
    for bit (scaling by powers of two commutes with every rounding), and rows the kernels add in CSR order equal a
    sequential fp32 sum -- a wrong entry -> value or column -> head mapping on any sub-path changes them"""
    g = _setup(fe, dev, kind, form)
    rng = np.random.default_rng(22)
    rows, col, rp, N = _rows_of(g["rp"]), g["col"], g["rp"], g["N"]
    deg = np.diff(rp)
    for heads, dh in [(2, 4), (3, 8), (4, 16), (8, 8), (4, 32), (2, 64)]:
        D = heads * dh
        a = rng.integers(-3, 4, (heads, N))
        b = rng.integers(-3, 4, (heads, N))
        V = np.ldexp(np.ones((heads, g["E"]), np.float32), a[:, rows] + b[:, col]).astype(np.float32)
        X = rng.standard_normal((N, D)).astype(np.float32)
        got = fe.forward_weighted_heads(torch.from_numpy(X).to(dev), torch.from_numpy(V).to(dev), *g["args"])[0]
        for h in range(heads):
            sa = torch.from_numpy(np.ldexp(np.ones(N), a[h]).astype(np.float32)).to(dev)[:, None]
            sb = torch.from_numpy(np.ldexp(np.ones(N), b[h]).astype(np.float32)).to(dev)[:, None]
            want = sa * fe.forward(sb * torch.from_numpy(X).to(dev), *g["args"])[0]
            sl = slice(h * dh, (h + 1) * dh)
            assert torch.equal(got[:, sl], want[:, sl]), (kind, form, heads, dh, h)
        if form not in ("sparse", "dense", "panel32", "plan_free"):  # (forms whose rows may be split or sliced: skipped)
            continue
        # sequential CSR-order sum (products exact): rows neither wide nor split
        Xs = np.ldexp(np.round(np.ldexp(X, 10)), -10).astype(np.float32)
        got = fe.forward_weighted_heads(torch.from_numpy(Xs).to(dev), torch.from_numpy(V).to(dev), *g["args"])[0].cpu().numpy()
        want = np.zeros((N, D), np.float32)
        for k in range(int(deg.max()) if len(deg) else 0):
            r = np.nonzero(deg > k)[0]
            e = rp[r] + k
            for h in range(heads):
                sl = slice(h * dh, (h + 1) * dh)
                want[r, sl] = (want[r, sl] + V[h, e][:, None] * Xs[col[e], sl]).astype(np.float32)
        thr = fe.wide_threshold(g["args"][6], D) if g["plan"] else 64
        ordered = deg <= min(thr, 256)
        assert np.array_equal(got[ordered].view(np.int32), want[ordered].view(np.int32)), (kind, form, heads, dh)


@pytest.mark.parametrize("form", ["default", "plan_free"])
@pytest.mark.parametrize("kind", KINDS)
def test_sddmm_heads_is_sddmm_on_the_column_slices(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    gen = torch.Generator(device="cpu").manual_seed(23)
    rows = torch.from_numpy(_rows_of(g["rp"])).long()
    cols = torch.from_numpy(g["col"]).long()
    for heads, dh in SHAPES + [(1, 512), (2, 260)]:
        D = heads * dh
        A = torch.randn(g["N"], D + 4, generator=gen).to(dev)[:, 2:D + 2]  # strided views, unaligned base
        B = torch.randn(g["N"], D, generator=gen).to(dev)
        got = fe.sddmm_heads(A, B, *g["args"], heads)
        assert got.shape == (heads, g["E"])
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            assert torch.equal(got[h], fe.sddmm(A[:, sl], B[:, sl], *g["args"])), (kind, form, heads, dh, h)
        A64, B64 = A.cpu().double(), B.cpu().double()
        prod = (A64[rows].view(-1, heads, dh) * B64[cols].view(-1, heads, dh))
        exact = prod.sum(2).t()
        bound = (dh + 1) * 2.0 ** -24 * prod.abs().sum(2).t()
        assert bool(((got.cpu().double() - exact).abs() <= bound).all()), (kind, form, heads, dh)


def test_bad_operands_are_refused(fe, dev):
    g = _setup(fe, dev, "uniform", "default")
    N, E = g["N"], g["E"]
    X = torch.randn(N, 24, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        fe.forward_weighted_heads(X, torch.rand(4, E, device=dev), *g["args"])  # Dh = 6
    with pytest.raises(RuntimeError, match="multiple of 4"):
        fe.forward_weighted_heads(X, torch.rand(5, E, device=dev), *g["args"])  # 24 % 5
    with pytest.raises(RuntimeError, match="float32"):
        fe.forward_weighted_heads(X.half(), torch.rand(2, E, device=dev), *g["args"])
    with pytest.raises(RuntimeError, match=r"\[heads, E\]"):
        fe.forward_weighted_heads(X, torch.rand(E, device=dev), *g["args"])
    with pytest.raises(RuntimeError, match="multiple of 4"):
        fe.sddmm_heads(X, X, *g["args"], 4)
    with pytest.raises(RuntimeError, match="float32"):
        fe.sddmm_heads(X.bfloat16(), X.bfloat16(), *g["args"], 2)


def test_heads_forward_replays_in_a_hip_graph(fe, dev):
    g = _setup(fe, dev, "planted", "default")
    X = torch.randn(g["N"], 64, device=dev)
    V = torch.rand(8, g["E"], device=dev)
    ref = fe.forward_weighted_heads(X, V, *g["args"])[0]
    ref_s = fe.sddmm_heads(X, X, *g["args"], 8)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fe.forward_weighted_heads(X, V, *g["args"])[0]
        out_s = fe.sddmm_heads(X, X, *g["args"], 8)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and torch.equal(out_s, ref_s)
    V.copy_(torch.rand(8, g["E"], device=dev))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fe.forward_weighted_heads(X, V, *g["args"])[0])


# ---------------------------------------------------------------- the layer
def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _segment_softmax64(x, rows, N):
    idx = rows.expand_as(x)
    m = torch.full((x.size(0), N), -float("inf"), dtype=x.dtype).scatter_reduce(1, idx, x, "amax")
    ex = torch.exp(x - m.gather(1, idx))
    s = torch.zeros((x.size(0), N), dtype=x.dtype).scatter_add(1, idx, ex)
    return ex / s.gather(1, idx)


def _torch_gat_concat64(X, W, a_src, a_dst, rows, cols, N, slope):
    outs = []
    for k in range(W.size(0)):
        h = X @ W[k]
        logit = torch.nn.functional.leaky_relu((h @ a_dst[k])[rows] + (h @ a_src[k])[cols], slope)
        alpha = _segment_softmax64(logit[None], rows, N)[0]
        outs.append(torch.zeros(N, h.size(1), dtype=h.dtype).index_add(0, rows, alpha[:, None] * h[cols]))
    return torch.cat(outs, 1)


def _close(got, want):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    return bool(((got - want).abs() <= 1e-4 * want.abs().max()).all())


def _symmetric(rp, col):
    """the pattern of A + A^T (the layer's backward needs a symmetric pattern; planted windows are not)"""
    N = len(rp) - 1
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(rp))
    key = np.unique(np.concatenate([rows * N + col, col.astype(np.int64) * N + rows]))
    out = np.zeros(N + 1, np.int32)
    np.cumsum(np.bincount(key // N, minlength=N), out=out[1:])
    return out, (key % N).astype(np.int32)


def _layer_graph(dev, kind="powerlaw"):
    _pkg_imports()
    import HCSPMM
    rp, col = graphs.powerlaw_graph(1500, 20000, seed=21, max_degree_frac=0.2) if kind == "powerlaw" else \
        _symmetric(*graphs.planted_dense_graph(1200, seed=8))
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    args = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16, -1))
    return rp, col, N, args


@pytest.mark.parametrize("kind", ["powerlaw", "planted"])
@pytest.mark.parametrize("heads,dout", [(1, 16), (4, 8), (8, 8), (4, 16), (3, 4)])
def test_concat_layer_matches_fp64(dev, kind, heads, dout):
    rp, col, N, args = _layer_graph(dev, kind)
    import GNN_model
    torch.manual_seed(heads * 100 + dout)
    conv = GNN_model.GATConv(24, dout, 0, heads=heads, concat=True).to(dev)
    X = torch.randn(N, 24, device=dev, requires_grad=True)
    Y = conv(X, *args, None)
    assert Y.shape == (N, heads * dout)
    G = torch.randn_like(Y)
    (Y * G).sum().backward()
    rows = torch.from_numpy(_rows_of(rp)).long()
    cols = torch.from_numpy(col).long()
    leaves = [X.detach().cpu().double().requires_grad_(True)] + \
        [p.detach().cpu().double().requires_grad_(True) for p in (conv.weights, conv.a_src, conv.a_dst)]
    Y64 = _torch_gat_concat64(*leaves, rows, cols, N, conv.negative_slope)
    (Y64 * G.cpu().double()).sum().backward()
    assert _close(Y, Y64), (kind, heads, dout)
    for name, got, want in zip(("X", "weights", "a_src", "a_dst"), (X.grad, conv.weights.grad, conv.a_src.grad, conv.a_dst.grad),
                               leaves):
        assert _close(got, want.grad), (kind, heads, dout, name)


def test_concat_layer_runs_on_the_library_kernels(dev, monkeypatch):
    """one update for all heads, the scores as one update, one attention launch, one multi-head aggregation; its backward
    on the update / weight-gradient kernels and the multi-head kernels, no single-head aggregation anywhere"""
    rp, col, N, args = _layer_graph(dev)
    import GNN_model
    import HCSPMM
    calls = {}

    def counting(name):
        fn = getattr(HCSPMM, name)

        def wrapped(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **k)
        monkeypatch.setattr(HCSPMM, name, wrapped)

    for name in ("forward_weighted", "forward_weighted_heads", "sddmm", "sddmm_heads", "gat_attention",
                 "gat_attention_backward"):
        counting(name)
    mm = []
    monkeypatch.setattr(GNN_model, "_mm", lambda X, W, _f=GNN_model._mm: mm.append(tuple(W.shape)) or _f(X, W))
    conv = GNN_model.GATConv(24, 8, 0, heads=4, concat=True).to(dev)
    Y = conv(torch.randn(N, 24, device=dev, requires_grad=True), *args, None)
    assert calls == {"forward_weighted_heads": 1, "gat_attention": 1} and mm == [(24, 32), (32, 8)]
    Y.sum().backward()
    assert calls == {"forward_weighted_heads": 2, "sddmm_heads": 1, "gat_attention": 1, "gat_attention_backward": 1}
    assert len(mm) == 4  # the two products' input gradients


@pytest.mark.parametrize("heads", [1, 4])
def test_mean_layer_still_calls_what_it_called(dev, heads, monkeypatch):
    rp, col, N, args = _layer_graph(dev)
    import GNN_model
    import HCSPMM
    calls = {}

    for name in ("forward_weighted", "forward_weighted_heads", "sddmm", "sddmm_heads", "gat_attention"):
        def wrapped(*a, _n=name, _f=getattr(HCSPMM, name), **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(HCSPMM, name, wrapped)
    conv = GNN_model.GATConv(24, 16, 0, heads=heads).to(dev)
    assert conv.concat is False
    Y = conv(torch.randn(N, 24, device=dev, requires_grad=True), *args, None)
    assert Y.shape == (N, 16)
    Y.sum().backward()
    assert calls == {"gat_attention": 1, "forward_weighted": 2 * heads, "sddmm": heads}


def test_state_dict_loads_into_either_mode_and_widths_are_checked(dev):
    _pkg_imports()
    import GNN_model
    a = GNN_model.GATConv(24, 8, 0, heads=4, concat=True)
    b = GNN_model.GATConv(24, 8, 0, heads=4)
    b.load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="multiple of 4"):
        GNN_model.GATConv(24, 6, 0, heads=4, concat=True)
    GNN_model.GATConv(24, 6, 0, heads=4)  # (the mean of heads has no such limit)


def test_concat_layer_step_replays_in_a_hip_graph(dev):
    rp, col, N, args = _layer_graph(dev, "planted")
    import GNN_model
    torch.manual_seed(5)
    conv = GNN_model.GATConv(24, 8, 0, heads=4, concat=True).to(dev)
    X = torch.randn(N, 24, device=dev)
    G = torch.randn(N, 32, device=dev)

    def step():
        for p in conv.parameters():
            p.grad = None
        (conv(X, *args, None) * G).sum().backward()
        return [p.grad for p in conv.parameters()]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            ref = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(out, ref):
        assert torch.equal(got, want)


def _driver():
    _pkg_imports()
    spec = importlib.util.spec_from_file_location("hc_spmm_main_heads", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_trains_concat_gat(capsys, monkeypatch):
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
                    "--epochs", "20", "--model", "gat", "--heads", "4", "--gat-concat"])
    assert "Train (ms/epoch):" in capsys.readouterr().out
    assert net.conv1.concat and net.hidden_layers[0].concat and not net.conv2.concat
    assert net.conv1.weights.shape == (4, 16, 8)
    assert losses[-1] < losses[0], losses
    assert all(np.isfinite(losses))
    for name, prm in net.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    for bad in (["--hidden", "24"], ["--hidden", "32", "--heads", "3"]):
        with pytest.raises(SystemExit):
            mod.parse_args(["--model", "gat", "--heads", "4", "--gat-concat"] + bad)
    with pytest.raises(SystemExit):
        mod.parse_args(["--model", "gcn", "--gat-concat"])
