"""GATv2 attention on fp16 / bf16 node rows (gatv2_attention16.hip) and the 16-bit GATv2Conv on an MI355X, through both front-ends.
References are torch fp64 on the 16-bit-rounded operands (the exact sum's sign is the fp32 sum's).  Bounds, u = 2^-24: scores
(Dh + 2) u sum_k |att_k l_k|; grad_H_* (n_row + 1) u |att_j| sum_e |g_e|, plus half an ulp for a 16-bit output; grad_att
(E + 1) u sum_e |g l| per column.  The module's name sorts it behind every other one."""
import ctypes

import numpy as np
import pytest
import torch

import frontends
from hcspmm import capi, graphs
from test_gatv2_gpu import fe  # noqa: F401 (the front-end fixture: ctypes, extension)
from test_zzzzzzz_heads16_gpu import DTYPES, SUB16, U16, _gnn_model, _prep, _rel, dev  # noqa: F401 (dev: the device fixture)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 4), (1, 8), (3, 8), (4, 12), (2, 40), (8, 8), (4, 64), (1, 512)]  # one-lane heads, padded groups, 3 and 5 lanes per head, the cap
LENGTHS = (1, 31, 32, 33, 255, 256, 257, 1500)  # both sides of each backward tier, and one workgroup row
_CACHE = {}


def _hub_graph():
    """Symmetric, 1603 rows (no multiple of a tile): three rows of each length in LENGTHS, 26 empty ones, fillers of up to 24; shuffled"""
    N, hubs = 1603, [n for n in LENGTHS for _ in range(3)]
    first = len(hubs) + 6
    rows = np.concatenate([np.full(n, i) for i, n in enumerate(hubs)])
    cols = np.concatenate([first + np.arange(n) if n > 1 else [first + 1552] for n in hubs])
    relabel = np.random.default_rng(30).permutation(N)
    key = np.unique(np.concatenate([relabel[rows] * N + relabel[cols], relabel[cols] * N + relabel[rows]]))
    rp = np.zeros(N + 1, np.int32)
    np.cumsum(np.bincount(key // N, minlength=N), out=rp[1:])
    assert set(LENGTHS) | {0} <= set(np.diff(rp).tolist())
    return rp, (key % N).astype(np.int32)


def _graph(dev, kind):
    if kind not in _CACHE:
        rp, col = _hub_graph() if kind == "hub" else graphs.uniform_graph(1003, 8000, seed=30)
        N, ct = len(rp) - 1, frontends.get("ctypes")
        g = dict(N=N, E=len(col), rp=torch.from_numpy(rp).to(dev), col=torch.from_numpy(col).to(dev),
                 rows=torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).to(dev))
        g["cols"] = g["col"].long()
        if kind == "hub":
            g["perm"] = ct.transpose_permutation(g["rp"], g["col"]).int()
        else:
            g["t"] = ct.transpose_graph(g["rp"], g["col"])
        _CACHE[kind] = g
    return _CACHE[kind]


def _backward(fe, g, gl, hd, hs, att, slope, grad_dtype=None):
    if "perm" in g:
        return fe.gatv2_scores_backward16(gl, hd, hs, att, g["rp"], g["col"], g["perm"], slope, grad_dtype=grad_dtype)
    return fe.gatv2_scores_backward_directed16(gl, hd, hs, att, g["rp"], g["col"], *g["t"], slope, grad_dtype=grad_dtype)


def _case(dev, kind, dtype, heads, dh, integers):
    """operands and their fp64 results, once per case for both front-ends: logits, the gradients, the bounds' sums of absolute terms"""
    key = (kind, dtype, heads, dh, integers)
    if key in _CACHE:
        return _CACHE[key]
    g, D = _graph(dev, kind), heads * dh
    N, E, rows, cols = g["N"], g["E"], g["rows"], g["cols"]
    gen = torch.Generator(device=dev).manual_seed(3000 + 64 * heads + dh)
    if integers:  # every operation is exact in fp32
        draw = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, device=dev, generator=gen).float()
        hd, hs, att, gl, slope = draw(-3, 3, (N, D)), draw(-3, 3, (N, D)), draw(-2, 2, (heads, dh)), draw(-1, 1, (heads, E)), 0.5
    else:
        draw = lambda *shape: torch.randn(shape, device=dev, generator=gen)
        hd, hs, att, gl, slope = draw(N, D), draw(N, D), draw(heads, dh), draw(heads, E), 0.2
    hd, hs, s = hd.to(dtype), hs.to(dtype), float(np.float32(slope))
    z = hd.double()[rows] + hs.double()[cols]  # [E, D]
    l, a = torch.where(z > 0, z, z * s), att.double().view(1, D)
    al = (l * a).view(E, heads, dh)
    ge = gl.double().T.repeat_interleave(dh, 1)  # [E, D]: g of the column's head
    gd = ge * torch.where(z > 0, 1.0, s)
    rowsum = lambda idx, m: torch.zeros(N, D, dtype=torch.float64, device=dev).index_add(0, idx, m)
    c = dict(hd=hd, hs=hs, att=att, gl=gl, slope=slope, logits=al.sum(-1).T.contiguous(), mass=al.abs().sum(-1).T,
             d_dst=a * rowsum(rows, gd), d_src=a * rowsum(cols, gd), d_att=(ge * l).sum(0).view(heads, dh),
             m_dst=a.abs() * rowsum(rows, ge.abs()), m_src=a.abs() * rowsum(cols, ge.abs()), m_att=(ge * l).abs().sum(0).view(heads, dh),
             n_dst=torch.bincount(rows, minlength=N).double()[:, None], n_src=torch.bincount(cols, minlength=N).double()[:, None])
    _CACHE[key] = c
    return c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,dh", SHAPES)
def test_scores_of_integers_are_exact(fe, dev, heads, dh, dtype):
    g, c = _graph(dev, "hub"), _case(dev, "hub", dtype, heads, dh, True)
    got = fe.gatv2_scores16(c["hd"], c["hs"], c["att"], g["rp"], g["col"], c["slope"])
    assert got.dtype == torch.float32 and got.shape == (heads, g["E"]) and torch.equal(got.double(), c["logits"])
    assert torch.equal(got, fe.gatv2_scores(c["hd"].float(), c["hs"].float(), c["att"], g["rp"], g["col"], c["slope"]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,dh", SHAPES)
def test_scores_of_normal_data_within_the_summation_bound(fe, dev, heads, dh, dtype):
    g, c = _graph(dev, "hub"), _case(dev, "hub", dtype, heads, dh, False)
    got = fe.gatv2_scores16(c["hd"], c["hs"], c["att"], g["rp"], g["col"], c["slope"])
    assert bool(((got.double() - c["logits"]).abs() <= (dh + 2) * U * c["mass"]).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["hub", "uniform"])
@pytest.mark.parametrize("heads,dh", SHAPES)
def test_backward_of_integers_is_exact(fe, dev, heads, dh, kind, dtype):
    g, c = _graph(dev, kind), _case(dev, kind, dtype, heads, dh, True)
    args = (fe, g, c["gl"], c["hd"], c["hs"], c["att"], c["slope"])
    d32, s32, a32 = _backward(*args, grad_dtype=torch.float32)
    assert d32.dtype == s32.dtype == a32.dtype == torch.float32 and torch.equal(d32.double(), c["d_dst"]) and torch.equal(s32.double(), c["d_src"]) and torch.equal(a32.double(), c["d_att"])
    d16, s16, a16 = _backward(*args)  # the default: the operands' dtype, one rounding of the same fp32 value
    assert d16.dtype == s16.dtype == dtype and torch.equal(d16, d32.to(dtype)) and torch.equal(s16, s32.to(dtype)) and torch.equal(a16, a32)
    again = _backward(*args)
    assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip((d16, s16), again[:2])) and torch.equal(a16, again[2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["hub", "uniform"])
@pytest.mark.parametrize("heads,dh", SHAPES)
def test_backward_of_normal_data_within_the_bounds(fe, dev, heads, dh, kind, dtype):
    g, c = _graph(dev, kind), _case(dev, kind, dtype, heads, dh, False)
    for grad_dtype in (torch.float32, dtype):
        got = _backward(fe, g, c["gl"], c["hd"], c["hs"], c["att"], c["slope"], grad_dtype=grad_dtype)
        for name, t in zip(("dst", "src"), got):
            exact, bound = c["d_" + name], (c["n_" + name] + 1) * U * c["m_" + name]
            if grad_dtype != torch.float32:
                bound = bound + torch.clamp(U16[dtype] * exact.abs(), min=SUB16[dtype])
            assert t.dtype == grad_dtype and bool(((t.double() - exact).abs() <= bound).all()), (name, grad_dtype)
        assert bool(((got[2].double() - c["d_att"]).abs() <= (g["E"] + 1) * U * c["m_att"]).all()), grad_dtype


@pytest.mark.parametrize("dtype", DTYPES)
def test_views_aliases_overwritten_outputs_and_graph_replay(fe, dev, dtype):
    heads, dh = 4, 12
    g, c = _graph(dev, "hub"), _case(dev, "hub", dtype, heads, dh, False)
    N, E, W = g["N"], g["E"], heads * dh
    hd, hs, att, gl, slope = c["hd"], c["hs"], c["att"], c["gl"], c["slope"]
    run = lambda a, b: [fe.gatv2_scores16(a, b, att, g["rp"], g["col"], slope), *_backward(fe, g, gl, a, b, att, slope)]
    same = lambda xs, ys: all(x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
                              for x, y in zip(xs, ys))  # the same bits
    ref = run(hd, hs)
    both = torch.cat([hs, hd], 1)  # the halves of one projection
    padded = torch.full((N, W + 6), float("nan"), device=dev, dtype=dtype)  # a row-padded stride
    padded[:, 2:2 + W] = hd
    assert same(run(both[:, W:], both[:, :W]), ref) and same(run(padded[:, 2:2 + W], hs), ref)
    assert same(run(hs, hs), run(hs.clone(), hs))  # H_dst is H_src
    # the C entry points write every element of NaN-filled outputs (here with a padded 16-bit gradient stride)
    lib, dt = capi.lib(), {torch.float16: 1, torch.bfloat16: 2}[dtype]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out, ga = torch.full((heads, E), float("nan"), device=dev), torch.full((heads, dh), float("nan"), device=dev)
    gd, gs = (torch.full((N, W + 2), float("nan"), device=dev, dtype=dtype) for _ in range(2))
    ws = torch.empty(lib.hcspmm_gatv2_backward_workspace_bytes(N, E, W, heads) // 4, device=dev)
    assert lib.hcspmm_gatv2_scores_typed(p(hd), W, p(hs), N, W, dt, p(att), slope, p(out), p(g["rp"]), p(g["col"]), N, E, W, heads, None) == 0
    assert lib.hcspmm_gatv2_scores_backward_typed(p(gl), p(hd), W, p(hs), W, dt, p(att), slope, p(g["rp"]), p(g["col"]), p(g["rp"]),
                                                  p(g["col"]), p(g["perm"]), N, N, E, W, heads, p(gd), W + 2, p(gs), W + 2, dt, p(ga),
                                                  p(ws), ws.numel() * 4, None) == 0
    torch.cuda.synchronize()
    assert same([out, gd[:, :W], gs[:, :W], ga], ref) and bool(torch.isnan(gd[:, W:]).all() and torch.isnan(gs[:, W:]).all())
    rp0, col0 = torch.zeros(N + 1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    empty = fe.gatv2_scores16(hd, hs, att, rp0, col0, slope)
    assert empty.shape == (heads, 0) and all(  # no entries: the gradients are zeros
        bool((t == 0).all()) for t in fe.gatv2_scores_backward16(empty, hd, hs, att, rp0, col0, col0, slope))
    # one capture, several replays: the eager bits
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(hd, hs)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert same(outs, ref)


def test_bad_operands_are_refused(fe, dev):
    g = _graph(dev, "hub")
    N, E = g["N"], g["E"]
    h, att, gl = torch.zeros(N, 32, device=dev, dtype=torch.bfloat16), torch.ones(4, 8, device=dev), torch.zeros(4, E, device=dev)
    odd, wide = torch.zeros(N, 33, device=dev, dtype=torch.bfloat16), torch.zeros(N, 520, device=dev, dtype=torch.bfloat16)
    off = torch.zeros(N, 34, device=dev, dtype=torch.bfloat16)[:, 1:33]  # an even stride, two bytes off the dword grid
    back = lambda a, b, **kw: fe.gatv2_scores_backward16(gl, a, b, att, g["rp"], g["col"], g["perm"], **kw)
    pairs = ((odd[:, :32], h), (h, off), (h, h.half()), (h.float(), h.float()))  # odd stride, misaligned view, mixed dtypes, fp32
    for call in ([lambda a=a, b=b: fe.gatv2_scores16(a, b, att, g["rp"], g["col"]) for a, b in pairs] + [lambda a=a, b=b: back(a, b) for a, b in pairs]
                 + [lambda: fe.gatv2_scores16(wide, wide, torch.ones(1, 520, device=dev), g["rp"], g["col"]),
                    lambda: back(h, h, grad_dtype=torch.float16), lambda: fe.gatv2_scores(h, h, att, g["rp"], g["col"])]):
        with pytest.raises(RuntimeError):
            call()


# ---------------------------------------------------------------- the layer
def _layer_graph(dev):
    if "layer" not in _CACHE:
        rp, col = graphs.powerlaw_graph(4100, 40000, seed=5)
        graph = _prep(frontends.get("extension"), dev, rp, col, "default")
        _CACHE["layer"] = (graph, torch.from_numpy(np.repeat(np.arange(len(rp) - 1), np.diff(rp))).to(dev), graph[1].long())
    return _CACHE["layer"]


def _gatv2_reference(X, W, att, rows, cols, lo):
    """the concat GATv2 layer in torch fp64; lo: X, the weights' copy, h and the output are rounded to it where the 16-bit layer rounds
    them (the logits, the attention and every sum stay exact)"""
    r = (lambda t: t.to(lo).double()) if lo is not None else (lambda t: t)
    heads, dout = att.shape
    N, width = X.size(0), heads * dout
    h = r(r(X) @ r(W))
    h_src, h_dst = h[:, :width].view(N, heads, dout), h[:, width:].view(N, heads, dout)
    logit = (torch.nn.functional.leaky_relu(h_dst[rows] + h_src[cols], 0.2) * att).sum(-1)
    m = torch.full((N, heads), -float("inf"), dtype=logit.dtype, device=logit.device).scatter_reduce(
        0, rows[:, None].expand_as(logit), logit, "amax")
    p = torch.exp(logit - m[rows])
    alpha = p / torch.zeros_like(m).index_add(0, rows, p)[rows]
    return r(torch.zeros_like(h_src).index_add(0, rows, alpha[..., None] * h_src[cols]).reshape(N, width))


def test_gatv2conv_bf16_against_the_fp32_layer(dev):
    """forward and backward on 4100 rows (the 16-bit update kernels run from 4096) against the fp32 layer on the same state dict.
    Tolerance as for the 16-bit GATConv: four times the bf16-against-fp64 difference of _gatv2_reference on the test's own data"""
    GNN_model = _gnn_model()
    graph, rows, cols = _layer_graph(dev)
    N = graph[0].numel() - 1
    torch.manual_seed(30)
    lo = GNN_model.GATv2Conv(16, 8, heads=4, concat=True, activation_dtype=torch.bfloat16).to(dev)
    hi = GNN_model.GATv2Conv(16, 8, heads=4, concat=True).to(dev)
    hi.load_state_dict(lo.state_dict())
    X0, dY = torch.randn(N, 16, device=dev), torch.randn(N, 32, device=dev)
    results = []
    for layer in (lo, hi):
        X = X0.clone().requires_grad_()
        out = layer(X, *graph)
        out.backward(dY.to(out.dtype))
        results.append([out.detach(), X.grad, layer.weights.grad, layer.att.grad])
    assert results[0][0].dtype == torch.bfloat16 and results[1][0].dtype == torch.float32
    assert all(t.dtype == torch.float32 for t in results[0][1:])
    refs = []
    for dt in (torch.bfloat16, None):
        leaves = [t.detach().double().requires_grad_() for t in (X0, hi.weights, hi.att)]
        out = _gatv2_reference(*leaves, rows, cols, dt)
        out.backward(dY.double() if dt is None else dY.to(dt).double())
        refs.append([out.detach()] + [t.grad for t in leaves])
    for name, got, want, r_lo, r_hi in zip(("out", "dX", "dW", "datt"), *results, *refs):
        measured = _rel(r_lo, r_hi)
        print(name, "reference composition bf16 vs fp64 %.3g, layer bf16 vs fp32 %.3g" % (measured, _rel(got, want)))
        assert _rel(got, want) <= 4 * measured, name


@pytest.mark.parametrize("concat,share", [(False, False), (True, True)])
def test_gatv2conv_variants_equal_the_composed_calls(dev, concat, share):
    GNN_model, fe = _gnn_model(), frontends.get("extension")
    graph = _layer_graph(dev)[0]
    N, heads, dout, lo = graph[0].numel() - 1, 4, 8, torch.bfloat16
    torch.manual_seed(31)
    layer = GNN_model.GATv2Conv(16, dout, heads=heads, concat=concat, share_weights=share, activation_dtype=lo).to(dev)
    X = torch.randn(N, 16, device=dev)
    with torch.no_grad():
        out = layer(X, *graph)
        h = GNN_model._Update16.apply(X.to(lo), layer.weights)
        h_src = h[:, :heads * dout]
        h_dst = h_src if share else h[:, heads * dout:]
        alpha = fe.edge_softmax(fe.gatv2_scores16(h_dst, h_src, layer.att, graph[0], graph[1], 0.2), graph[0])
        want = fe.forward_weighted_heads16(h_src.contiguous(), alpha, *graph)[0]
        if not concat:
            want = want.float().view(N, heads, dout).mean(1).to(lo)
    assert out.dtype == lo and out.shape == (N, heads * dout if concat else dout) and torch.equal(out.view(torch.int16), want.view(torch.int16))
