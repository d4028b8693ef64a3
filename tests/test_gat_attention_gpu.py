"""GAT attention (include/hcspmm.h hcspmm_gat_attention, hcspmm_gat_attention_backward; GNN_model.gat_attention,
GATConv) on an MI355X, through both Python front-ends.

  * forward: bit for bit edge_softmax(leaky_relu(s_dst[rows] + s_src[cols])) on every head, rows of 0, 1, 16, 17, 2048,
    2049 and 12 000 entries (all three row paths and both thresholds on each side), square and rectangular;
  * forward accuracy against fp64 with logits over +-80; backward against fp64 autograd, z == 0 included;
  * E = 0 and empty rows (zeros over NaN), HIP-graph replay, argument errors, and the layer.
"""
import ctypes
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
U = 2.0 ** -24


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


def _threshold_graph():
    """Symmetric: a star with 12 000 leaves (a hub row and rows of 1), complete bipartite blocks K(4, 16), K(3, 17),
    K(3, 2048), K(2, 2049) (rows of exactly 16, 17, 2048, 2049 and the short rows on their other side) and isolated
    nodes (rows of 0); node ids shuffled so that every workgroup mixes the paths."""
    rows, cols, nxt = [], [], 0

    def bipartite(a, b):
        nonlocal nxt
        left, right = np.arange(nxt, nxt + a), np.arange(nxt + a, nxt + a + b)
        nxt += a + b
        r, c = np.repeat(left, b), np.tile(right, a)
        rows.extend([r, c])
        cols.extend([c, r])

    bipartite(1, 12000)
    for a, b in ((4, 16), (3, 17), (3, 2048), (2, 2049)):
        bipartite(a, b)
    N = nxt + 300
    relabel = np.random.default_rng(41).permutation(N)
    rp, col = _csr(N, relabel[np.concatenate(rows)], relabel[np.concatenate(cols)])
    lens = set(np.diff(rp).tolist())
    assert {0, 1, 16, 17, 2048, 2049, 12000} <= lens
    return rp, col


def _graph(kind):
    if kind == "thresholds":
        return _threshold_graph()
    if kind == "powerlaw":
        return graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    raise KeyError(kind)


_CACHE = {}


def _setup(dev, kind):
    if kind not in _CACHE:
        rp, col = _graph(kind)
        N = len(rp) - 1
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).to(dev)
        perm = frontends.get("ctypes").transpose_permutation(rp_d, col_d)
        _CACHE[kind] = dict(N=N, E=len(col), rp=rp_d, col=col_d, rows=rows, cols=col_d.long(), perm=perm,
                            lens=torch.from_numpy(np.diff(rp)).to(dev))
    return _CACHE[kind]


def _scores(dev, n, heads, seed, spread=1.0, zeros=True):
    """[n] (heads = 1) or [n, heads] float32, with exact zeros (and, through s_dst = -s_src below, z == 0) when asked"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    s = (torch.rand((n, heads), device=dev, generator=gen) * 2 - 1) * spread
    if zeros:
        s[::7] = 0.0
    return s[:, 0].contiguous() if heads == 1 else s


def _heads_view(t, heads):
    return t.reshape(-1, heads) if t.dim() == 1 else t


def _torch_logits(s_dst, s_src, rows, cols, slope, heads):
    z = _heads_view(s_dst, heads)[rows] + _heads_view(s_src, heads)[cols]  # [E, heads], fp32 as the kernel adds
    return torch.nn.functional.leaky_relu(z, slope).t().contiguous()


def _segment_softmax64(x, rows, N):
    """fp64 per-row softmax of x [heads, E] with torch ops (autograd-able)"""
    idx = rows.expand_as(x)
    m = torch.full((x.size(0), N), -float("inf"), dtype=x.dtype, device=x.device).scatter_reduce(1, idx, x, "amax")
    ex = torch.exp(x - m.gather(1, idx))
    s = torch.zeros((x.size(0), N), dtype=x.dtype, device=x.device).scatter_add(1, idx, ex)
    return ex / s.gather(1, idx)


HEADS = [1, 3, 4]
SLOPES = [0.2, 0.0, 1.0]


# ------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("kind", ["thresholds", "powerlaw"])
def test_forward_is_the_edge_softmax_of_the_torch_logits_bit_for_bit(fe, dev, kind, heads, slope):
    g = _setup(dev, kind)
    s_dst = _scores(dev, g["N"], heads, 1 + heads, spread=8.0)
    s_src = _scores(dev, g["N"], heads, 2 + heads, spread=8.0)
    _heads_view(s_dst, heads)[3::11] = -_heads_view(s_src, heads)[3::11]
    alpha = fe.gat_attention(s_dst, s_src, g["rp"], g["col"], slope)
    assert alpha.dtype == torch.float32 and alpha.shape == ((g["E"],) if heads == 1 else (heads, g["E"]))
    logits = _torch_logits(s_dst, s_src, g["rows"], g["cols"], slope, heads)
    want = fe.edge_softmax(logits[0] if heads == 1 else logits, g["rp"])
    assert torch.equal(alpha, want)
    assert torch.equal(alpha, fe.gat_attention(s_dst, s_src, g["rp"], g["col"], slope))


@pytest.mark.parametrize("heads", HEADS)
def test_rectangular_forward(fe, dev, heads):
    """a row block: 700 rows of a uniform graph whose columns index all 2000 rows of s_src"""
    rp, col = graphs.uniform_graph(2000, 16000, seed=7)
    rp, col = rp[:701], col[:rp[700]]
    N, E = 700, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).to(dev)
    s_dst = _scores(dev, N, heads, 5, spread=4.0)
    s_src = _scores(dev, 2000, heads, 6, spread=4.0)
    alpha = fe.gat_attention(s_dst, s_src, rp_d, col_d, 0.2)
    logits = _torch_logits(s_dst, s_src, rows, col_d.long(), 0.2, heads)
    assert torch.equal(alpha, fe.edge_softmax(logits[0] if heads == 1 else logits, rp_d))
    assert E > 0 and int(col.max()) >= N


@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("kind", ["thresholds", "powerlaw"])
def test_forward_accuracy_with_logits_over_80(fe, dev, kind, heads):
    """scores over +-40, logits over +-80 (slope 1): relative error <= 1e-5 against the fp64 segment softmax of the
    logits (z rounded to fp32, as any fp32 formulation rounds it)"""
    g = _setup(dev, kind)
    s_dst = _scores(dev, g["N"], heads, 11, spread=40.0, zeros=False)
    s_src = _scores(dev, g["N"], heads, 12, spread=40.0, zeros=False)
    alpha = fe.gat_attention(s_dst, s_src, g["rp"], g["col"], 1.0)
    logits = _torch_logits(s_dst, s_src, g["rows"], g["cols"], 1.0, heads)
    assert float(logits.abs().max()) > 60
    want = _segment_softmax64(logits.double(), g["rows"], g["N"])
    err = (alpha.reshape(heads, -1).double() - want).abs()
    assert bool((err <= 1e-5 * want + 2.0 ** -126).all()), float((err / want.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------- backward
def _fp64_backward(g, s_dst, s_src, grad_alpha, slope, heads):
    """fp64 autograd of the same formulation from z (the fp32 sum, so that z's sign -- and the derivative at z == 0 --
    is the kernel's); -> (grad_s_dst, grad_s_src, grad_z [heads, E], per-entry scale sum |terms|)"""
    z32 = (_heads_view(s_dst, heads)[g["rows"]] + _heads_view(s_src, heads)[g["cols"]]).t()
    z = z32.double().requires_grad_(True)
    alpha = _segment_softmax64(torch.nn.functional.leaky_relu(z, slope), g["rows"], g["N"])
    ga = grad_alpha.reshape(heads, -1).double()
    (alpha * ga).sum().backward()
    gz = z.grad
    gd = torch.zeros((heads, g["N"]), dtype=torch.float64, device=z.device).index_add(1, g["rows"], gz)
    gs = torch.zeros((heads, g["N"]), dtype=torch.float64, device=z.device).index_add(1, g["cols"], gz)
    idx = g["rows"].expand(heads, -1)
    dot = torch.zeros((heads, g["N"]), dtype=torch.float64, device=z.device).scatter_add(1, idx, (alpha * ga).abs().detach())
    f = torch.where(z32 > 0, torch.ones_like(z32), torch.full_like(z32, slope)).double()
    scale = alpha.detach() * (ga.abs() + dot.gather(1, idx)) * f
    return gd, gs, gz, scale


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("kind", ["thresholds", "powerlaw"])
def test_backward_matches_fp64_autograd(fe, dev, kind, heads, slope):
    """componentwise: g within 4 (n + 2) 2^-24 sum |terms| (n = the row's length; alpha itself carries the softmax's
    rounding), each segment sum within the sum of its terms' bounds plus (m + 2) 2^-24 sum |g| (m = its length)"""
    g = _setup(dev, kind)
    s_dst = _scores(dev, g["N"], heads, 21 + heads, spread=3.0)
    s_src = _scores(dev, g["N"], heads, 22 + heads, spread=3.0)
    _heads_view(s_dst, heads)[3::11] = -_heads_view(s_src, heads)[3::11]
    alpha = fe.gat_attention(s_dst, s_src, g["rp"], g["col"], slope)
    gen = torch.Generator(device=dev).manual_seed(heads)
    grad_alpha = torch.randn(alpha.shape, device=dev, generator=gen)
    gd, gs, gsc = fe.gat_attention_backward(alpha, grad_alpha, s_dst, s_src, g["rp"], g["col"], g["perm"], slope)
    assert gd.shape == s_dst.shape and gs.shape == s_src.shape and gsc.shape == alpha.shape

    want_d, want_s, want_z, scale = _fp64_backward(g, s_dst, s_src, grad_alpha, slope, heads)
    z32 = (_heads_view(s_dst, heads)[g["rows"]] + _heads_view(s_src, heads)[g["cols"]]).t()
    assert bool((z32 == 0).any())  # the derivative at z == 0 is exercised (slope, as torch's leaky_relu_backward)
    n = g["lens"].double()[g["rows"]]
    b_e = 4 * (n + 2) * U * scale + 2.0 ** -126
    got_z = gsc.reshape(heads, -1).double()
    assert bool(((got_z - want_z).abs() <= b_e).all()), float(((got_z - want_z).abs() / b_e).max())
    lens = g["lens"].double()
    for got, want, idx in ((gd, want_d, g["rows"]), (gs, want_s, g["cols"])):
        zero = torch.zeros((heads, g["N"]), dtype=torch.float64, device=dev)
        bound = zero.index_add(1, idx, b_e) + (lens + 2) * U * zero.index_add(1, idx, want_z.abs()) + 2.0 ** -126
        got = _heads_view(got, heads).t().double()
        assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())

    # the gradient of l is edge_softmax_backward's, bit for bit; then the LeakyReLU derivative as torch applies it
    gl = fe.edge_softmax_backward(alpha, grad_alpha, g["rp"]).reshape(heads, -1)
    want_bits = torch.where(z32 > 0, gl, gl * slope)
    assert torch.equal(gsc.reshape(heads, -1), want_bits)
    again = fe.gat_attention_backward(alpha, grad_alpha, s_dst, s_src, g["rp"], g["col"], g["perm"].int(), slope)
    for a, b in zip((gd, gs, gsc), again):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- edge cases
def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _capi_backward(alpha, grad_alpha, s_dst, s_src, rp, col, perm, N, E, heads, out, gd, gs):
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)
    return capi.lib().hcspmm_gat_attention_backward(p(alpha), p(grad_alpha), p(s_dst), p(s_src), 0.2, p(rp), p(col), p(perm), N, E,
                                                   heads, p(out), p(gd), p(gs), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_without_entries_the_score_gradients_are_zeros(fe, dev):
    N, heads = 37, 3
    rp = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    col = torch.zeros(0, dtype=torch.int32, device=dev)
    s = torch.randn(N, heads, device=dev)
    alpha = fe.gat_attention(s, s, rp, col)
    assert alpha.shape == (heads, 0)
    gd, gs, gsc = fe.gat_attention_backward(alpha, alpha, s, s, rp, col, col)
    assert gsc.shape == (heads, 0) and bool((gd == 0).all()) and bool((gs == 0).all())
    gd, gs = _nan((N, heads), dev), _nan((N, heads), dev)
    assert _capi_backward(None, None, s, s, rp, col, col, N, 0, heads, None, gd, gs) == 0
    torch.cuda.synchronize()
    assert bool((gd == 0).all()) and bool((gs == 0).all())


def test_rows_without_entries_get_zeros(dev):
    g = _setup(dev, "thresholds")
    heads = 4
    s_dst, s_src = _scores(dev, g["N"], heads, 31), _scores(dev, g["N"], heads, 32)
    alpha = frontends.get("ctypes").gat_attention(s_dst, s_src, g["rp"], g["col"])
    grad_alpha = torch.randn_like(alpha)
    gd, gs, out = _nan((g["N"], heads), dev), _nan((g["N"], heads), dev), _nan((heads, g["E"]), dev)
    perm32 = g["perm"].int()
    assert _capi_backward(alpha, grad_alpha, s_dst, s_src, g["rp"], g["col"], perm32, g["N"], g["E"], heads, out, gd, gs) == 0
    torch.cuda.synchronize()
    empty = g["lens"] == 0
    assert int(empty.sum()) == 300
    assert bool((gd[empty] == 0).all()) and bool((gs[empty] == 0).all())
    assert not bool(torch.isnan(gd).any() or torch.isnan(gs).any() or torch.isnan(out).any())


def test_forward_and_backward_replay_in_a_hip_graph(fe, dev):
    g = _setup(dev, "thresholds")
    heads = 4
    s_dst, s_src = _scores(dev, g["N"], heads, 41), _scores(dev, g["N"], heads, 42)
    grad_alpha = torch.randn((heads, g["E"]), device=dev)
    perm32 = g["perm"].int()
    ref_alpha = fe.gat_attention(s_dst, s_src, g["rp"], g["col"])
    ref = fe.gat_attention_backward(ref_alpha, grad_alpha, s_dst, s_src, g["rp"], g["col"], perm32)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        alpha = fe.gat_attention(s_dst, s_src, g["rp"], g["col"])
        outs = fe.gat_attention_backward(alpha, grad_alpha, s_dst, s_src, g["rp"], g["col"], perm32)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(alpha, ref_alpha)
    for a, b in zip(outs, ref):
        assert torch.equal(a, b)
    s_src.copy_(torch.randn_like(s_src))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(alpha, fe.gat_attention(s_dst, s_src, g["rp"], g["col"]))


def test_argument_errors_raise(fe, dev):
    g = _setup(dev, "powerlaw")
    N, E = g["N"], g["E"]
    s = torch.randn(N, 2, device=dev)
    rp, col = g["rp"], g["col"]
    for bad in (s.double(), torch.randn(N - 1, 2, device=dev), torch.randn(N, 3, device=dev), s.cpu(), s.t()):
        with pytest.raises(RuntimeError):
            fe.gat_attention(bad, s, rp, col)
    with pytest.raises(RuntimeError):
        fe.gat_attention(s, torch.randn(N), rp, col)  # 1-D against 2-D scores
    alpha = fe.gat_attention(s, s, rp, col)
    ga = torch.randn_like(alpha)
    fe.gat_attention_backward(alpha, ga, s, s, rp, col, g["perm"])
    for args in ((alpha, ga, s, s, rp, col, g["perm"][:-1]),           # perm of the wrong length
                 (alpha, ga, s, s, rp, col, g["perm"].float()),        # perm of the wrong dtype
                 (alpha, ga, s, s, rp, col, g["perm"].cpu()),          # a CPU tensor
                 (alpha[:1], ga, s, s, rp, col, g["perm"]),            # alpha of the wrong shape
                 (alpha, ga.double(), s, s, rp, col, g["perm"]),       # wrong dtype
                 (alpha.cpu(), ga, s, s, rp, col, g["perm"]),
                 (alpha, ga, s, torch.randn(N + 5, 2, device=dev), rp, col, g["perm"])):  # rectangular backward
        with pytest.raises(RuntimeError):
            fe.gat_attention_backward(*args)
    with pytest.raises(RuntimeError):
        fe.gat_attention(s, s, rp, col, float("nan"))


# ------------------------------------------------------------------------------------------- the layer
def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _torch_gat64(X, W, a_src, a_dst, rows, cols, N, slope):
    outs = []
    for k in range(W.size(0)):
        h = X @ W[k]
        logit = torch.nn.functional.leaky_relu((h @ a_dst[k])[rows] + (h @ a_src[k])[cols], slope)
        alpha = _segment_softmax64(logit[None], rows, N)[0]
        outs.append(torch.zeros(N, h.size(1), dtype=h.dtype).index_add(0, rows, alpha[:, None] * h[cols]))
    return torch.stack(outs).mean(0)


def _close(got, want):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    return bool(((got - want).abs() <= 1e-4 * want.abs().max()).all())


@pytest.mark.parametrize("heads", [1, 4])
def test_gat_layer_uses_the_fused_attention(dev, heads, monkeypatch):
    _pkg_imports()
    import GNN_model
    import HCSPMM
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = HCSPMM.gat_attention, HCSPMM.gat_attention_backward

    def counting_fwd(*a, **k):
        calls["fwd"] += 1
        return fwd(*a, **k)

    def counting_bwd(*a, **k):
        calls["bwd"] += 1
        return bwd(*a, **k)

    monkeypatch.setattr(HCSPMM, "gat_attention", counting_fwd)
    monkeypatch.setattr(HCSPMM, "gat_attention_backward", counting_bwd)
    rp, col = graphs.powerlaw_graph(1500, 20000, seed=21, max_degree_frac=0.2)
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    args = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16, -1))
    torch.manual_seed(heads)
    conv = GNN_model.GATConv(24, 16, 0, heads=heads).to(dev)
    X = torch.randn(N, 24, device=dev, requires_grad=True)
    Y = conv(X, *args, None)
    assert calls == {"fwd": 1, "bwd": 0}
    G = torch.randn_like(Y)
    (Y * G).sum().backward()
    assert calls == {"fwd": 1, "bwd": 1}
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).long()
    cols = torch.from_numpy(col).long()
    leaves = [X.detach().cpu().double().requires_grad_(True)] + \
        [p.detach().cpu().double().requires_grad_(True) for p in (conv.weights, conv.a_src, conv.a_dst)]
    Y64 = _torch_gat64(*leaves, rows, cols, N, conv.negative_slope)
    (Y64 * G.cpu().double()).sum().backward()
    assert _close(Y, Y64)
    for got, want in zip((X.grad, conv.weights.grad, conv.a_src.grad, conv.a_dst.grad), leaves):
        assert _close(got, want.grad), heads

    # the asymmetric pattern is still refused, before any attention launch
    rp2, col2 = graphs.uniform_graph(500, 3000, seed=6)
    rp2_d, col2_d = torch.from_numpy(rp2).to(dev), torch.from_numpy(col2).to(dev)
    args2 = (rp2_d, col2_d) + tuple(HCSPMM.preprocess(col2_d, rp2_d, 500, len(col2), (500 + 15) // 16, -1))
    with pytest.raises(RuntimeError, match="symmetric"):
        conv(torch.randn(500, 24, device=dev), *args2, None)
    assert calls == {"fwd": 1, "bwd": 1}
