"""Gated neighbour aggregation in one gather pass (hcspmm_forward_gated), the GatedAggregate function and the ResGatedGraphConv
layer built on it, on an MI355X through both Python front-ends.

The contract (include/hcspmm.h): with z = fl32(P[r] + Q[c]) over the entries (r, c) of row r,
  Z_gate[r] = sum sigma(z) V[c],  Z_dgate[r] = sum sigma'(z) V[c],
sigma from t = exp(-|z|), r = 1 / (1 + t): where t underflows sigma is exactly 1 or 0 and sigma' exactly 0, which makes +-200
in P or Q an exact row / column selector on integer V.  Either output may be left out and the other keeps its bits; a fixed
order, so two calls give the same bits; rows without entries give +0.

Continuous data follow the project's rule for order-dependent fp32 results: the reference is the formula in fp64 on the fp32 z, the
yardstick the same formula in fp32 numpy with rows summed entry after entry in CSR order, and the library may err by at most
4 x the yardstick's own maximum error plus 1e-6 * max|ref| -- taken separately over rows of at most 64 entries and over longer
rows.  On the CPU a re-ordered fp32 sum with +-1 ulp on exp and rcp stays below 0.25 of that bound for both outputs.

The module's name sorts it behind every other one on purpose: the modules that were here before keep their places in the
suite's run order.
"""
import ctypes

import numpy as np
import pytest
import torch

import frontends
from hcspmm import graphs
from test_softmax_aggr_gpu import (PLANS, _asymmetric, _bits_equal, _bounds, _check_bound, _csr, _hub_graph, _np, _pkg_imports,
                                   _prepare, _setup, _sum_rows, _transpose)
from test_width_edges_gpu import _setup as _ragged_setup

pytestmark = pytest.mark.gpu

KINDS = ["powerlaw", "planted", "molecule", "uniform"]
WIDTHS = [1, 3, 4, 22, 32, 64, 128, 256]
RAGGED_WIDTHS = [2, 5, 33, 70, 130, 260]
RAGGED_FORMS = ["one_pass", "one_pass_slices", "one_pass_segments", "one_pass_dense", "panel32", "plan_free"]
EXACT_WIDTHS = [3, 22, 128]
KIND_FORM = [(k, f) for k in KINDS for f in PLANS]
FRONTENDS = ["ctypes", "extension"]
BOTH = ("gate", "dgate")

_REFS = {}
_WORST = {}  # output name -> the largest error / bound seen by this module's continuous-data checks


@pytest.fixture(scope="module", params=FRONTENDS)
def fe(request):
    return frontends.get(request.param)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def gated_reference(rp, col, P, Q, V, dtype):
    """(Z_gate, Z_dgate) of the formula in `dtype` arithmetic on the fp32 z (float64: the reference; float32: the yardstick,
    sequential sums in CSR order)"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    z = (P[rows] + Q[col]).astype(dtype)  # one fp32 add, then widened
    one = dtype(1)
    t = np.exp(-np.abs(z))
    r = one / (one + t)
    tr = t * r
    v = V[col].astype(dtype)
    return _sum_rows(np.where(z >= 0, r, tr) * v, rp), _sum_rows(tr * r * v, rp)


def _operands(rng, n, rows, D):
    return ((2.0 * rng.standard_normal((n, D))).astype(np.float32), (2.0 * rng.standard_normal((rows, D))).astype(np.float32),
            rng.standard_normal((rows, D)).astype(np.float32))


def _refs(key, rp, col, D, seed, rows=None):
    """operands, fp64 references and bounds of a graph, computed once and shared by every plan form and front-end"""
    key = key + (D,)
    if key not in _REFS:
        n = len(rp) - 1
        P, Q, V = _operands(np.random.default_rng(seed + D), n, rows or n, D)
        r64 = gated_reference(rp, col, P, Q, V, np.float64)
        y32 = gated_reference(rp, col, P, Q, V, np.float32)
        lens = np.diff(rp)
        _REFS[key] = (P, Q, V, r64, [_bounds(r, y, lens) for r, y in zip(r64, y32)])
    return _REFS[key]


def _check_both(out, r64, bounds, tag):
    for o, ref, bd, name in zip(out, r64, bounds, BOTH):
        _check_bound(_np(o), ref, bd, tag + (name,), _WORST)
    print("largest error / bound so far: %s" % {k: round(v, 3) for k, v in _WORST.items()})


# ------------------------------------------------------------------------------------------- continuous data
@pytest.mark.parametrize("fe_name", FRONTENDS)
@pytest.mark.parametrize("kind,form", KIND_FORM)
def test_both_outputs_on_continuous_data(fe_name, dev, kind, form):
    """randn V, 2 randn P and Q: both outputs within 4 x the fp32 yardstick's error + 1e-6 max|ref| of fp64, per row group; two
    calls give the same bits"""
    fe = frontends.get(fe_name)
    g = _setup(fe, dev, kind, form)
    for D in WIDTHS:
        P, Q, V, r64, bounds = _refs(("cont", kind), g["rp"], g["col"], D, 7000 + 100 * KINDS.index(kind))
        ops = [_t(a, dev) for a in (P, Q, V)]
        out = fe.forward_gated(*ops, *g["args"], outputs=BOTH)
        assert len(out) == 2 and all(o.shape == (g["N"], D) and o.is_contiguous() and o.dtype == torch.float32 for o in out)
        _check_both(out, r64, bounds, (kind, form, D))
        if D in (3, 128):
            again = fe.forward_gated(*ops, *g["args"], outputs=BOTH)
            assert _same_bits(out[0], again[0]) and _same_bits(out[1], again[1]), (kind, form, D)


@pytest.mark.parametrize("fe_name", FRONTENDS)
@pytest.mark.parametrize("form", RAGGED_FORMS)
def test_ragged_widths(fe_name, dev, form):
    """widths that are no multiple of the lanes' four columns, on rows of length 0 ... 257 and hubs of 513, 770 and 1100"""
    fe = frontends.get(fe_name)
    g = _ragged_setup(fe, dev, form)
    for D in RAGGED_WIDTHS:
        P, Q, V, r64, bounds = _refs(("ragged",), g["rp"], g["col"], D, 7700)
        out = fe.forward_gated(*(_t(a, dev) for a in (P, Q, V)), *g["args"], outputs=BOTH)
        _check_both(out, r64, bounds, ("ragged", form, D))
        empty = g["lens"] == 0
        for o in out:
            assert _bits_equal(_np(o)[empty], np.zeros((int(empty.sum()), D), np.float32)), (form, D)


# ------------------------------------------------------------------------------------------- exact cases
def _checker(n, D, offset=0):
    i, d = np.arange(n)[:, None], np.arange(D)[None, :]
    return np.where((i + d + offset) % 2 == 0, 200.0, -200.0).astype(np.float32)


@pytest.mark.parametrize("fe_name", FRONTENDS)
@pytest.mark.parametrize("kind,form", KIND_FORM)
def test_saturated_gates_select_exactly(fe_name, dev, kind, form):
    """integer V and gates of +-200.  In P (Q = 0): Z_gate[i][d] is the integer neighbour sum where P is +200 and exactly +0
    where it is -200 -- the own-row lookup of every task kind, the tiny task of a split row's last segment included.  In Q
    (P = 0): the integer sum over the selected neighbours -- the gathered-row lookup.  Z_dgate is exactly +0 both times."""
    fe = frontends.get(fe_name)
    g = _setup(fe, dev, kind, form)
    rp, col, N = g["rp"], g["col"], g["N"]
    for D in EXACT_WIDTHS:
        V = np.random.default_rng(7100 + D).integers(-3, 4, (N, D)).astype(np.float32)
        zero = np.zeros((N, D), np.float32)
        sums = _sum_rows(V[col].astype(np.float64), rp).astype(np.float32)
        own = _checker(N, D)
        Zg, Zd = fe.forward_gated(_t(own, dev), _t(zero, dev), _t(V, dev), *g["args"], outputs=BOTH)
        assert _bits_equal(_np(Zg), np.where(own > 0, sums, 0.0).astype(np.float32) + 0.0), (kind, form, D, "P")
        assert _bits_equal(_np(Zd), zero), (kind, form, D, "P")
        sel = _checker(N, D, 1)
        want = _sum_rows(np.where(sel[col] > 0, V[col], 0.0).astype(np.float64), rp).astype(np.float32)
        Zg, Zd = fe.forward_gated(_t(zero, dev), _t(sel, dev), _t(V, dev), *g["args"], outputs=BOTH)
        assert _bits_equal(_np(Zg), want + 0.0), (kind, form, D, "Q")
        assert _bits_equal(_np(Zd), zero), (kind, form, D, "Q")


def test_special_values(fe, dev):
    """NaN propagates, +-inf behaves as the limit, |z| >= 104 saturates exactly, z = 0 gives 1/2 and 1/4"""
    rp, col = _csr(np.arange(8), np.arange(8), 8)
    g = _prepare(fe, dev, rp, col, "plan_free")
    p = np.array([np.nan, np.inf, -np.inf, 104.0, -104.0, 0.0, 1e30, -1e30], np.float32)
    P = np.repeat(p[:, None], 5, 1)
    V = np.full((8, 5), 3.0, np.float32)
    Zg, Zd = (_np(o) for o in fe.forward_gated(_t(P, dev), _t(np.zeros_like(P), dev), _t(V, dev), *g["args"], outputs=BOTH))
    assert np.isnan(Zg[0]).all() and np.isnan(Zd[0]).all()
    assert _bits_equal(Zg[[1, 3, 6]], np.full((3, 5), 3.0, np.float32)) and _bits_equal(Zg[[2, 4, 7]], np.zeros((3, 5), np.float32))
    assert _bits_equal(Zd[[1, 2, 3, 4, 6, 7]], np.zeros((6, 5), np.float32))
    assert (np.abs(Zg[5] - 1.5) <= 1e-6).all() and (np.abs(Zd[5] - 0.75) <= 1e-6).all()


# ------------------------------------------------------------------------------------------- single versus double output
@pytest.mark.parametrize("form", list(PLANS))
def test_an_output_keeps_its_bits_without_the_other(fe, dev, form):
    g = _setup(fe, dev, "powerlaw", form)
    for D in WIDTHS:
        ops = [_t(a, dev) for a in _refs(("cont", "powerlaw"), g["rp"], g["col"], D, 7000)[:3]]
        both = fe.forward_gated(*ops, *g["args"], outputs=BOTH)
        gate = fe.forward_gated(*ops, *g["args"])  # the default: Z_gate alone
        dgate = fe.forward_gated(*ops, *g["args"], outputs=("dgate",))
        assert gate[1] is None and dgate[0] is None and len(gate) == 2 and len(dgate) == 2
        assert _same_bits(both[0], gate[0]) and _same_bits(both[1], dgate[1]), (form, D)
        assert _same_bits(both[0], fe.forward_gated(*ops, *g["args"], outputs="gate")[0]), (form, D)


# ------------------------------------------------------------------------------------------- the transposed call
@pytest.mark.parametrize("form", ["default", "plan_free"])
def test_backward_recipe_has_the_forwards_gates_on_a_permutation(fe, dev, form):
    """every row of A has exactly one entry (i, perm[i]), so no sum is involved: with V = 1 the forward returns the gates
    themselves, and the backward recipe -- dP = G T; one two-output call on A^T with own rows Q and gathered (P, G) for dV and
    dQ = V Y_dgate -- must equal the per-entry formula in torch fp32 on those gates, bit for bit"""
    _pkg_imports()
    import GNN_model
    rng = np.random.default_rng(43)
    N = 1500
    perm = rng.permutation(N)
    rp, col = _csr(np.arange(N), perm, N)
    rp_t, col_t = _transpose(rp, col, N)
    g, gt = _prepare(fe, dev, rp, col, form), _prepare(fe, dev, rp_t, col_t, form)
    pl = torch.from_numpy(perm).to(dev)
    for D in (3, 22, 64):
        P, Q, V = (_t(a, dev) for a in _operands(rng, N, N, D))
        G = torch.randn(N, D, device=dev)
        S, dS = fe.forward_gated(P, Q, torch.ones_like(V), *g["args"], outputs=BOTH)  # sigma and sigma' of every entry
        Z, T = fe.forward_gated(P, Q, V, *g["args"], outputs=BOTH)
        assert _same_bits(Z, S * V[pl]) and _same_bits(T, dS * V[pl]), (form, D)
        dV, Y = fe.forward_gated(Q, P, G, *gt["args"], outputs=BOTH)
        want_dV, want_dQ = torch.empty_like(dV), torch.empty_like(dV)
        want_dV[pl] = S * G
        want_dQ[pl] = V[pl] * (dS * G)
        assert _same_bits(dV, want_dV) and _same_bits(V * Y, want_dQ), (form, D)
        if fe.name == "extension":  # ... and through the autograd function, which launches on that front-end
            ops = [x.clone().requires_grad_(True) for x in (P, Q, V)]
            out = GNN_model.gated_aggregate(*ops, g["args"], directed=True)
            assert _same_bits(out, Z), (form, D)
            out.backward(G)
            assert _same_bits(ops[0].grad, G * T) and _same_bits(ops[1].grad, want_dQ) and _same_bits(ops[2].grad, want_dV), (form, D)


# ------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_empty_rows_duplicate_columns_and_a_hub(fe, dev, form):
    """rows without entries give +0 in both outputs; a column stored twice in a row counts twice (the reference reads the stored
    entries as they are); one row of 600 entries is split into segments"""
    rp, col = _hub_graph(np.random.default_rng(33))
    N = len(rp) - 1
    g = _prepare(fe, dev, rp, col, form)
    lens = np.diff(rp)
    empty = lens == 0
    assert empty.any() and (np.diff(col)[np.diff(np.repeat(np.arange(N), lens)) == 0] == 0).any() and lens.max() == 600
    for D in (3, 32, 64):
        P, Q, V, r64, bounds = _refs(("hub",), rp, col, D, 7300)
        out = fe.forward_gated(*(_t(a, dev) for a in (P, Q, V)), *g["args"], outputs=BOTH)
        _check_both(out, r64, bounds, ("hub", form, D))
        for o in out:
            assert _bits_equal(_np(o)[empty], np.zeros((int(empty.sum()), D), np.float32)), (form, D)


@pytest.mark.parametrize("form", ["default", "slices", "plan_free"])
def test_rectangular_block(fe, dev, form):
    """a row block of a graph whose column ids index taller Q and V"""
    rp_full, col_full = graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    n = 1200
    rp, col = rp_full[:n + 1].copy(), col_full[:rp_full[n]].copy()
    g = _prepare(fe, dev, rp, col, form, num_columns=3000)
    for D in (3, 22, 64):
        P, Q, V, r64, bounds = _refs(("rect",), rp, col, D, 7400, rows=3000)
        out = fe.forward_gated(*(_t(a, dev) for a in (P, Q, V)), *g["args"], outputs=BOTH)
        assert all(o.shape == (n, D) for o in out)
        _check_both(out, r64, bounds, ("rect", form, D))
    with pytest.raises(RuntimeError):  # P has the block's rows, not the gathered operands'
        fe.forward_gated(_t(Q, dev), _t(Q, dev), _t(V, dev), *g["args"])
    if form != "plan_free":
        with pytest.raises(RuntimeError, match="plan gathers from"):
            fe.forward_gated(_t(P, dev), _t(Q[:n], dev), _t(V[:n], dev), *g["args"])


SENTINEL = -777.0


def _direct(g, P, Q, V, D, ptrs, ldz):
    """hcspmm_forward_gated through ctypes directly: ptrs = data pointers (or None) of Z_gate, Z_dgate"""
    import hcspmm
    from hcspmm import capi
    c = hcspmm._planned_call(g["args"][:6], g["args"][6], D, Q.size(0), Q.device, ws_fn=hcspmm._ws_bytes_gated)
    vp = [ctypes.c_void_p(p or 0) for p in ptrs]
    with c:
        rc = capi.lib().hcspmm_forward_gated(ctypes.c_void_p(P.data_ptr()), P.stride(0), ctypes.c_void_p(Q.data_ptr()), Q.stride(0),
                                             ctypes.c_void_p(V.data_ptr()), V.stride(0), Q.size(0), *vp, ldz, *c.graph, *c.ws)
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["default", "tiny_segments", "panel32", "plan_free"])
def test_strided_operands_and_framed_outputs(fe, dev, form):
    """P, Q, V as column blocks of one [N, 4 D + 9] buffer, 5 elements in, everything around them NaN: the contiguous call's
    bits, so nothing outside the views is read.  Then (through the C entry point: the front-ends allocate their own outputs)
    the outputs inside sentinel frames, ldz = D + 9, which come back untouched -- with one output left NULL as well"""
    g = _setup(fe, dev, "powerlaw", form)
    N = g["N"]
    for D in (3, 7, 22, 64, 130):
        P, Q, V = (_t(a, dev) for a in _operands(np.random.default_rng(7500 + D), N, N, D))
        full = fe.forward_gated(P, Q, V, *g["args"], outputs=BOTH)
        buf = torch.full((N, 4 * D + 9), float("nan"), device=dev)
        views = [buf[:, 5 + k * D:5 + (k + 1) * D] for k in range(3)]
        for v, src in zip(views, (P, Q, V)):
            v.copy_(src)
        out = fe.forward_gated(*views, *g["args"], outputs=BOTH)
        assert _same_bits(out[0], full[0]) and _same_bits(out[1], full[1]), (form, D)
        if fe.name != "ctypes":
            continue
        ldz = D + 9
        for subset in ((0, 1), (0,), (1,)):
            frames = [torch.full((N, ldz), SENTINEL, device=dev) for _ in range(2)]
            _direct(g, *views, D, [frames[k][:, 5:].data_ptr() if k in subset else None for k in range(2)], ldz)
            for k in range(2):
                if k in subset:
                    assert _same_bits(frames[k][:, 5:5 + D], full[k]), (form, D, subset, k)
                    assert (frames[k][:, :5] == SENTINEL).all() and (frames[k][:, 5 + D:] == SENTINEL).all(), (form, D, subset, k)
                else:
                    assert (frames[k] == SENTINEL).all(), (form, D, subset, k)


# ------------------------------------------------------------------------------------------- layer
def _torch_resgated(X, W, rp, col, H):
    """ResGatedGraphConv from index_add, in X's dtype"""
    N = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(N, device=X.device), (rp[1:] - rp[:-1]).long())
    proj = X @ W
    P, Q, V, S = (proj[:, k * H:(k + 1) * H] for k in range(4))
    c = col.long()
    msg = torch.sigmoid(P[rows] + Q[c]) * V[c]
    return S + torch.zeros(N, H, dtype=X.dtype, device=X.device).index_add(0, rows, msg)


@pytest.mark.parametrize("kind", ["powerlaw", "planted", "molecule", "asymmetric"])
def test_resgatedgraphconv_matches_a_torch_layer(dev, kind):
    """forward, X.grad and weights.grad against the same layer in torch.  The reference is that layer in fp64; the yardstick is
    the fp32 torch layer's own maximum error against it: the library layer may err by at most 4 x that plus 1e-6 * max|ref|
    (the rule of test_genconv_matches_a_torch_layer)."""
    _pkg_imports()
    import GNN_model
    ext = frontends.get("extension")
    directed = kind == "asymmetric"
    g = _prepare(ext, dev, *_asymmetric(), "default") if directed else _setup(ext, dev, kind, "default", sym=True)
    torch.manual_seed(35)
    conv = GNN_model.ResGatedGraphConv(24, 16, directed=directed).to(dev)
    X = torch.randn(g["N"], 24, device=dev, requires_grad=True)
    out = conv(X, *g["args"], None)
    assert out.shape == (g["N"], 16)
    dY = torch.randn_like(out)
    out.backward(dY)
    rp, col = g["args"][0], g["args"][1]
    results = {}
    for dtype in (torch.float64, torch.float32):
        Xr, Wr = (v.detach().to(dtype).requires_grad_(True) for v in (X, conv.weights))
        o = _torch_resgated(Xr, Wr, rp, col, 16)
        o.backward(dY.to(dtype))
        results[dtype] = (o.detach(), Xr.grad, Wr.grad)
    mine = (out.detach(), X.grad, conv.weights.grad)
    for name, m, t32, t64 in zip(("out", "X.grad", "weights.grad"), mine, results[torch.float32], results[torch.float64]):
        yard = float((t32.double() - t64).abs().max())
        err = float((m.double() - t64).abs().max())
        bound = 4.0 * yard + 1e-6 * float(t64.abs().max())
        print("%s %s: library error %.3e, fp32 torch error %.3e, bound %.3e, error / bound %.3f" % (kind, name, err, yard, bound,
                                                                                                   err / bound))
        assert err <= bound, (kind, name, err, yard, bound)


def test_refusals(fe, dev):
    _pkg_imports()
    import GNN_model
    g = _prepare(frontends.get("extension"), dev, *_asymmetric(200, 3, 36), "default")
    X = torch.randn(200, 8, device=dev)
    with pytest.raises(RuntimeError, match="symmetric"):
        GNN_model.ResGatedGraphConv(8, 8).to(dev)(X, *g["args"], None)
    with pytest.raises(RuntimeError, match="symmetric"):
        GNN_model.gated_aggregate(X, X, X, g["args"])
    with pytest.raises(ValueError):
        GNN_model.ResGatedGraphConv(8, 8, directed=True).to(dev)(X, *g["args"], None, edge_weight=torch.ones(len(g["col"]), device=dev))
    h = _setup(fe, dev, "uniform", "default")
    A = torch.randn(h["N"], 8, device=dev)
    for bad in ((A.cpu(), A, A), (A, A.cpu(), A), (A, A, A.cpu()), (A.half(), A, A), (A, A.half(), A.half()), (A, A, A.double()),
                (A[:, :4], A, A), (A, A, A[:, :4]), (A, A[:, :4], A), (A[:-1], A, A), (A, A, A[:-1]), (A, A[:, ::2], A[:, ::2])):
        with pytest.raises(RuntimeError):
            fe.forward_gated(*bad, *h["args"])
    for bad in ((), ("gates",), ("gate", "T"), "both"):
        with pytest.raises(ValueError):
            fe.forward_gated(A, A, A, *h["args"], outputs=bad)


def test_hip_graph_capture(fe, dev):
    """one forward + backward pair (two two-output launches) captured on a side stream and replayed once: the eager bits"""
    g = _setup(fe, dev, "powerlaw", "default", sym=True)
    D = 32
    P, Q, V, G = (torch.randn(g["N"], D, device=dev) for _ in range(4))
    eager = tuple(fe.forward_gated(P, Q, V, *g["args"], outputs=BOTH)) + tuple(fe.forward_gated(Q, P, G, *g["args"], outputs=BOTH))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = tuple(fe.forward_gated(P, Q, V, *g["args"], outputs=BOTH)) + tuple(fe.forward_gated(Q, P, G, *g["args"], outputs=BOTH))
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert _same_bits(a, b)
