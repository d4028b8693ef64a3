"""Multi-head weighted aggregation and SDDMM on fp16 / bf16 rows (hcspmm_forward_weighted_heads_typed / hcspmm_sddmm_heads_typed:
spmm_heads16.hip, sddmm_heads16.hip), EdgeWeightedAggregateHeads16 and the 16-bit concat GATConv, on an MI355X, through both
front-ends.  References are fp64 numpy / torch on the rounded operands.  The module's name sorts it behind every other one."""
import os
import sys

import numpy as np
import pytest
import torch

import frontends
from hcspmm import graphs

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
# below the smallest normal number a format's spacing is absolute, so its rounding error is no longer u |x| but half that spacing
# (fp16: 2^-24 / 2; bf16: 2^-133 / 2): low-degree rows of N(0, 1) products do land there in fp16
SUB16 = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}


def _round16(exact, dtype):
    return np.maximum(U16[dtype] * np.abs(exact), SUB16[dtype])


GRAPHS = {"powerlaw": lambda: graphs.powerlaw_graph(1003, 20000), "planted": lambda: graphs.planted_dense_graph(640),
          "uniform": lambda: graphs.uniform_graph(2048, 30000)}
FORMS = {"default": {}, "plan_free": None, "split": dict(split_threshold=64, segment_len=32),
         "slices": dict(slice_threshold=32, n_slices=8), "panel16": dict(panel_cols=16)}
PAIRS = [(1, 8), (2, 4), (4, 8), (3, 12), (8, 16)]
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _gnn_model():
    frontends.get("extension")  # (puts the extension module, which GNN_model imports, on the path)
    pkg = os.path.dirname(frontends.EXT_DIR)
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import GNN_model
    return GNN_model


def _graph(kind):
    if kind not in _CACHE:
        _CACHE[kind] = GRAPHS[kind]()
    return _CACHE[kind]


def _prep(fe, dev, rp, col, form, num_columns=None):
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    bp, e2c, e2r, ht, row_nzr, col_nzr = fe.preprocess(col_d, rp_d, N, E, (N + 15) // 16, num_columns=num_columns)
    if FORMS[form] is None:
        row_nzr = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
        row_nzr = fe.build_plan(rp_d, col_d, bp, e2c, ht, num_columns=num_columns, **FORMS[form])
    return (rp_d, col_d, bp, e2c, e2r, ht, row_nzr, col_nzr)


def _args(fe, dev, kind, form):
    if (fe.name, kind, form) not in _CACHE:
        _CACHE[(fe.name, kind, form)] = _prep(fe, dev, *_graph(kind), form)
    return _CACHE[(fe.name, kind, form)]


def _row_sums(rp, M):
    out, nz = np.zeros((len(rp) - 1,) + M.shape[1:]), np.diff(rp) > 0
    if nz.any():
        out[nz] = np.add.reduceat(M, rp[:-1][nz].astype(np.int64), axis=0)
    return out


def _products(V, X, col, dh):
    """per entry and column, v[head of the column][e] * X[col(e)][column]: V [heads, E] already gathered through the index"""
    return np.repeat(V.T.astype(np.float64), dh, axis=1) * X.astype(np.float64)[col]


def _head_dots(A, B, rows, col, heads):
    return (A.astype(np.float64)[rows] * B.astype(np.float64)[col]).reshape(len(col), heads, -1)


def _t16(a, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).to(dtype)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,form", [(k, f) for k in GRAPHS for f in FORMS])
def test_integer_sums_are_exact(dev, kind, form, dtype):
    """X in [-4, 4], values in {-1, 0.5, 1, 2}: every partial sum is exact, so fp32 Z equals the fp64 sum and 16-bit Z its one
    rounding, whatever the order -- identity values, a many-to-one index with num_values != E, and the SDDMM on integers"""
    rp, col = _graph(kind)
    N, E = len(rp) - 1, len(col)
    rows = np.repeat(np.arange(N), np.diff(rp))
    for fe in (frontends.get("extension"), frontends.get("ctypes")):
        args = _args(fe, dev, kind, form)
        for heads, dh in PAIRS:
            rng = np.random.default_rng(2900 + 16 * heads + dh)
            D, nv = heads * dh, max(E // 5, 1)
            X, B = rng.integers(-4, 5, (N, D)), rng.integers(-4, 5, (N, D))
            V = rng.choice([-1.0, 0.5, 1.0, 2.0], (heads, E)).astype(np.float32)
            many = rng.integers(0, nv, E).astype(np.int32)
            Xd, Vd, idx = _t16(X, dev, dtype), torch.from_numpy(V).to(dev), torch.from_numpy(many).to(dev)
            for name, want, kw in (("identity", _row_sums(rp, _products(V, X, col, dh)), {}),
                                   ("indexed", _row_sums(rp, _products(V[:, :nv][:, many], X, col, dh)), dict(value_index=idx))):
                vals = Vd if name == "identity" else Vd[:, :nv].contiguous()
                z32 = fe.forward_weighted_heads16(Xd, vals, *args, out_dtype=torch.float32, **kw)[0]
                z16 = fe.forward_weighted_heads16(Xd, vals, *args, **kw)[0]
                tag = (kind, form, fe.name, heads, dh, name)
                assert z32.dtype == torch.float32 and torch.equal(z32.cpu().double(), torch.from_numpy(want)), tag
                # (values, not bits: numpy's sum of one product -1 * 0 is -0, an fma chain that starts at +0 gives +0)
                assert z16.dtype == dtype and torch.equal(z16.cpu(), torch.from_numpy(want).to(dtype)), tag
            if form in ("default", "plan_free"):
                got = fe.sddmm_heads16(Xd, _t16(B, dev, dtype), *args, heads)
                want = _head_dots(X, B, rows, col, heads).sum(-1).T
                assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), torch.from_numpy(want)), (kind, form, fe.name, heads, dh)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,form", [("powerlaw", "default"), ("planted", "plan_free"), ("powerlaw", "split"), ("uniform", "slices"),
                                       ("planted", "panel16")])
def test_normal_data_within_the_rounding_bound(dev, kind, form, dtype):
    """N(0, 1) data against the fp64 product of the rounded operands.  fp32 Z: the order-free bound (n_r + 1) 2^-24 sum |v x| of a
    chain or tree of n_r fmas; 16-bit Z adds its one rounding, u |exact| (_round16: half the subnormal spacing below fp16's normal
    range); SDDMM: (Dh + 1) 2^-24 sum |a_k b_k|.  Values of 1 with one head: forward_typed on the same X lies within the 16-bit bound of the same sum, so the two differ by at most twice that bound"""
    rp, col = _graph(kind)
    N, E = len(rp) - 1, len(col)
    rows, deg = np.repeat(np.arange(N), np.diff(rp)), np.diff(rp).astype(np.float64)[:, None]
    for fe in (frontends.get("extension"), frontends.get("ctypes")):
        args = _args(fe, dev, kind, form)
        for heads, dh in PAIRS:
            rng = np.random.default_rng(2950 + 16 * heads + dh)
            D = heads * dh
            Xd, Bd = (_t16(rng.standard_normal((N, D)), dev, dtype) for _ in range(2))
            V = rng.standard_normal((heads, E)).astype(np.float32)
            X64, B64 = Xd.double().cpu().numpy(), Bd.double().cpu().numpy()
            prod = _products(V, X64, col, dh)
            exact, b32 = _row_sums(rp, prod), (deg + 1) * 2.0 ** -24 * _row_sums(rp, np.abs(prod))
            z32 = fe.forward_weighted_heads16(Xd, torch.from_numpy(V).to(dev), *args, out_dtype=torch.float32)[0].double().cpu().numpy()
            z16 = fe.forward_weighted_heads16(Xd, torch.from_numpy(V).to(dev), *args)[0].double().cpu().numpy()
            e32, e16 = np.abs(z32 - exact), np.abs(z16 - exact)
            assert np.all(e32 <= b32) and np.all(e16 <= b32 + _round16(exact, dtype)), (kind, form, fe.name, heads, dh)
            dots = _head_dots(X64, B64, rows, col, heads)
            got = fe.sddmm_heads16(Xd, Bd, *args, heads).double().cpu().numpy()
            assert np.all(np.abs(got - dots.sum(-1).T) <= (dh + 1) * 2.0 ** -24 * np.abs(dots).sum(-1).T), (kind, form, fe.name, heads, dh)
        Xd = _t16(np.random.default_rng(2990).standard_normal((N, 32)), dev, dtype)
        ones = _row_sums(rp, Xd.double().cpu().numpy()[col])
        bound = (deg + 1) * 2.0 ** -24 * _row_sums(rp, np.abs(Xd.double().cpu().numpy()[col])) + _round16(ones, dtype)
        ours = fe.forward_weighted_heads16(Xd, torch.ones(1, E, device=dev), *args)[0].double().cpu().numpy()
        binary = fe.forward(Xd, *args)[0].double().cpu().numpy()
        assert np.all(np.abs(ours - ones) <= bound) and np.all(np.abs(ours - binary) <= 2 * bound), (kind, form, fe.name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_views_rectangular_rows_repeats_and_graph_replay(dev, dtype):
    fe = frontends.get("extension")
    rp, col = _graph("powerlaw")
    N, E, heads, D = len(rp) - 1, len(col), 4, 32
    args = _args(fe, dev, "powerlaw", "default")
    rng = np.random.default_rng(2960)
    Xd, V = _t16(rng.standard_normal((N, D)), dev, dtype), torch.from_numpy(rng.standard_normal((heads, E)).astype(np.float32)).to(dev)
    idx = torch.from_numpy(rng.permutation(E).astype(np.int32)).to(dev)
    ref, ref_i, ref_s = (fe.forward_weighted_heads16(Xd, V, *args)[0], fe.forward_weighted_heads16(Xd, V, *args, value_index=idx)[0],
                         fe.sddmm_heads16(Xd, Xd, *args, heads))
    assert _same_bits(fe.forward_weighted_heads16(Xd, V, *args)[0], ref) and torch.equal(fe.sddmm_heads16(Xd, Xd, *args, heads), ref_s)
    # a column block of a wider NaN-filled buffer (ldx > D), through both front-ends
    buf = torch.full((N, D + 10), float("nan"), device=dev, dtype=dtype)
    buf[:, 2:2 + D] = Xd
    for f in (fe, frontends.get("ctypes")):
        a = _args(f, dev, "powerlaw", "default")
        assert _same_bits(f.forward_weighted_heads16(buf[:, 2:2 + D], V, *a, value_index=idx)[0], ref_i)
        assert torch.equal(f.sddmm_heads16(buf[:, 2:2 + D], buf[:, 2:2 + D], *a, heads), ref_s)
    # a row block whose column ids index a taller X
    cut = 401
    rp_r, col_r = rp[:cut + 1].copy(), col[:rp[cut]].copy()
    for form in ("default", "plan_free"):
        a = _prep(fe, dev, rp_r, col_r, form, num_columns=N)
        Vr = V[:, :len(col_r)].contiguous()
        got = fe.forward_weighted_heads16(Xd, Vr, *a, out_dtype=torch.float32)[0].double().cpu().numpy()
        prod = _products(Vr.cpu().numpy(), Xd.double().cpu().numpy(), col_r, D // heads)
        assert got.shape == (cut, D) and np.all(np.abs(got - _row_sums(rp_r, prod)) <=
                                                (np.diff(rp_r)[:, None] + 1.0) * 2.0 ** -24 * _row_sums(rp_r, np.abs(prod)))
    # a captured HIP graph replays the eager bits, also after the operands change
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fe.forward_weighted_heads16(Xd, V, *args, value_index=idx)[0]
        out_s = fe.sddmm_heads16(Xd, Xd, *args, heads)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, ref_i) and torch.equal(out_s, ref_s)
    Xd.copy_(_t16(rng.standard_normal((N, D)), dev, dtype))
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out, fe.forward_weighted_heads16(Xd, V, *args, value_index=idx)[0])
    assert torch.equal(out_s, fe.sddmm_heads16(Xd, Xd, *args, heads))


@pytest.mark.parametrize("name", ["extension", "ctypes"])
def test_bad_operands_are_refused(dev, name):
    fe = frontends.get(name)
    args = _args(fe, dev, "powerlaw", "default")
    N, E = args[0].numel() - 1, args[1].numel()
    X, V = torch.zeros(N, 32, device=dev, dtype=torch.bfloat16), torch.ones(4, E, device=dev)
    idx = torch.zeros(E, dtype=torch.int32, device=dev)
    wide = torch.zeros(N, 34, device=dev, dtype=torch.bfloat16)
    for bad in (lambda: fe.forward_weighted_heads16(X.float(), V, *args), lambda: fe.forward_weighted_heads16(X, V.half(), *args),
                lambda: fe.forward_weighted_heads16(X, V[:, :-1].contiguous(), *args),
                lambda: fe.forward_weighted_heads16(X, V, *args, value_index=idx.long()),
                lambda: fe.forward_weighted_heads16(X, V, *args, out_dtype=torch.float16),
                lambda: fe.forward_weighted_heads16(X[:, :24], V, *args), lambda: fe.forward_weighted_heads16(wide[:, 1:33], V, *args),
                lambda: fe.sddmm_heads16(X, X.half(), *args, 4), lambda: fe.sddmm_heads16(X.float(), X.float(), *args, 4),
                lambda: fe.sddmm_heads16(X, X, *args, 3), lambda: fe.sddmm_heads16(wide[:, 1:33], X, *args, 4)):
        with pytest.raises(RuntimeError):
            bad()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("directed", [False, True])
def test_autograd_matches_fp64_on_the_rounded_operands(dev, directed, dtype):
    """EdgeWeightedAggregateHeads16: Z and dX (16-bit: the fp32 bound of their own row of A / A^T plus one rounding) and dw (the
    SDDMM bound) against numpy fp64 on X16, w and dY16"""
    GNN_model = _gnn_model()
    kind = "uniform" if directed else "powerlaw"
    rp, col = _graph(kind)
    N, E, heads, dh = len(rp) - 1, len(col), 3, 12
    rows = np.repeat(np.arange(N), np.diff(rp))
    rng = np.random.default_rng(2970)
    X = _t16(rng.standard_normal((N, heads * dh)), dev, dtype).requires_grad_()
    w = torch.from_numpy(rng.standard_normal((heads, E)).astype(np.float32)).to(dev).requires_grad_()
    dY = _t16(rng.standard_normal((N, heads * dh)), dev, dtype)
    out = GNN_model.edge_weighted_aggregate_heads(X, w, _args(frontends.get("extension"), dev, kind, "default"), directed)
    out.backward(dY)
    assert out.dtype == dtype and X.grad.dtype == dtype and w.grad.dtype == torch.float32
    X64, Y64, w64 = X.detach().double().cpu().numpy(), dY.double().cpu().numpy(), w.detach().cpu().numpy()
    prod = _products(w64, X64, col, dh)
    exact = _row_sums(rp, prod)
    assert np.all(np.abs(out.detach().double().cpu().numpy() - exact) <=
                  (np.diff(rp)[:, None] + 1.0) * 2.0 ** -24 * _row_sums(rp, np.abs(prod)) + _round16(exact, dtype))
    back = np.repeat(w64.T.astype(np.float64), dh, axis=1) * Y64[rows]  # A_w^T dY: entry e adds w[e] dY[row(e)] to row col(e)
    dx, mass, indeg = np.zeros_like(X64), np.zeros_like(X64), np.bincount(col, minlength=N).astype(np.float64)[:, None]
    np.add.at(dx, col, back)
    np.add.at(mass, col, np.abs(back))
    assert np.all(np.abs(X.grad.double().cpu().numpy() - dx) <= (indeg + 1) * 2.0 ** -24 * mass + _round16(dx, dtype))
    dots = _head_dots(Y64, X64, rows, col, heads)
    assert np.all(np.abs(w.grad.double().cpu().numpy() - dots.sum(-1).T) <= (dh + 1) * 2.0 ** -24 * np.abs(dots).sum(-1).T)


def _gat_reference(X, W, a_src, a_dst, rows, col, lo):
    """the concat GAT layer in torch fp64; lo: the dtype X, the parameters' copies, h and the output are rounded to where the
    16-bit layer rounds them (the scores, the attention and every sum stay exact)"""
    r = (lambda t: t.to(lo).double()) if lo is not None else (lambda t: t)
    heads, din, dout = W.shape
    N = X.size(0)
    h = r(r(X) @ r(W.permute(1, 0, 2).reshape(din, heads * dout))).view(N, heads, dout)
    s_dst, s_src = (h * r(a_dst)).sum(-1), (h * r(a_src)).sum(-1)
    logit = torch.nn.functional.leaky_relu(s_dst[rows] + s_src[col], 0.2)
    m = torch.full((N, heads), -float("inf"), dtype=logit.dtype, device=logit.device).scatter_reduce(
        0, rows[:, None].expand_as(logit), logit, "amax")
    p = torch.exp(logit - m[rows])
    alpha = p / torch.zeros_like(m).index_add(0, rows, p)[rows]
    return r(torch.zeros_like(h).index_add(0, rows, alpha[..., None] * h[col]).reshape(N, heads * dout))


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_gatconv_bf16_against_the_fp32_layer(dev):
    """GATConv(16, 8, heads=4, concat=True, activation_dtype=bfloat16), forward and backward on 4100 rows (the 16-bit update and
    weight-gradient kernels run from 4096), against the fp32 layer on the same parameters.  Tolerance: the bf16-against-fp64
    difference of the reference composition (_gat_reference: torch fp64 with X, the weights, h, the output and dY rounded where the
    layer rounds them), as max |a - b| / max |b| per tensor, times four for the accumulation orders of the library against torch.
    Measured differences of the reference composition on this graph and these parameter ranges (three seeds): out 3.4e-3 ... 4.2e-3,
    dX 3.1e-2 ... 4.3e-2, dW 0.9e-2 ... 1.2e-2, da_src 1.6e-2 ... 3.3e-2, da_dst 4.0e-2 ... 5.1e-2, i.e. tolerances of about
    1.5e-2, 0.15, 4e-2, 0.1 and 0.18; the test measures the difference again on its own data and allows four times that."""
    GNN_model = _gnn_model()
    fe = frontends.get("extension")
    rp, col = graphs.powerlaw_graph(4100, 40000, seed=5)
    N = len(rp) - 1
    graph = _prep(fe, dev, rp, col, "default")
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).to(dev)
    cl = torch.from_numpy(col.astype(np.int64)).to(dev)
    torch.manual_seed(29)
    lo = GNN_model.GATConv(16, 8, heads=4, concat=True, activation_dtype=torch.bfloat16).to(dev)
    hi = GNN_model.GATConv(16, 8, heads=4, concat=True).to(dev)
    hi.load_state_dict(lo.state_dict())
    X0, dY = torch.randn(N, 16, device=dev), torch.randn(N, 32, device=dev)
    results = []
    for layer in (lo, hi):
        X = X0.clone().requires_grad_()
        out = layer(X, *graph)
        out.backward(dY.to(out.dtype))
        results.append([out.detach(), X.grad, layer.weights.grad, layer.a_src.grad, layer.a_dst.grad])
    assert results[0][0].dtype == torch.bfloat16 and results[1][0].dtype == torch.float32
    refs = []
    for dt in (torch.bfloat16, None):
        leaves = [t.detach().double().requires_grad_() for t in (X0, hi.weights, hi.a_src, hi.a_dst)]
        out = _gat_reference(*leaves, rows, cl, dt)
        out.backward(dY.double() if dt is None else dY.to(dt).double())
        refs.append([out.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad, leaves[3].grad])
    for name, got, want, r_lo, r_hi in zip(("out", "dX", "dW", "da_src", "da_dst"), *results, *refs):
        measured = _rel(r_lo, r_hi)
        print(name, "reference composition bf16 vs fp64 %.3g, layer bf16 vs fp32 %.3g" % (measured, _rel(got, want)))
        assert _rel(got, want) <= 4 * measured, name
