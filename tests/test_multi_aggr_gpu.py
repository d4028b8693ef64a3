"""Sum, sum of squares, max and min of each row's neighbours in one gather pass (hcspmm_forward_multi), the MultiAggregate
function and the PNAConv layer built on it, on an MI355X through both Python front-ends.

The contract (include/hcspmm.h): max / min / both args are the bits of a sequential scan of each row, exactly as
hcspmm_forward_extremum gives them; sum and sumsq are summed in a fixed order (CSR order in a lane group, a shuffle tree on wide
tasks, slot order in the fix-up), the square rounded before it is added; rows without entries give +0 and -1; a NULL output
is not written.  Integer inputs make every sum exact in any order, so there all six outputs are compared bit for bit.
"""
import ctypes
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


def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


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


def _csr(rows, cols, N):
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rp = np.zeros(N + 1, np.int32)
    np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp).astype(np.int32), cols.astype(np.int32)


def _symmetric(rp, col):
    """the pattern of A + A^T (the backward walks A^T through the transpose permutation)"""
    N = len(rp) - 1
    rows = np.repeat(np.arange(N), np.diff(rp))
    pairs = np.unique(np.stack([np.concatenate([rows, col]), np.concatenate([col, rows])], 1), axis=0)
    return _csr(pairs[:, 0], pairs[:, 1], N)


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
WIDTHS = [1, 3, 4, 22, 32, 64, 128, 256]

_CACHE = {}
_REFS = {}  # (graph kind, D, data kind) -> (X, the references): computed once, shared by every plan form and front-end


def _prepare(fe, dev, rp, col, form, num_columns=None):
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    bp, e2c, e2r, ht, row_nzr, col_nzr = fe.preprocess(col_d, rp_d, N, E, (N + 15) // 16, rule=3, num_columns=num_columns)
    p = dict(PLANS[form])
    force = p.pop("force", None)
    plan = p.pop("plan", True)
    if force is not None:
        ht = torch.full_like(ht, force)
    if not plan:
        row_nzr = torch.zeros(1, dtype=torch.int32, device=dev)
    elif force is not None or p or num_columns is not None:
        row_nzr = fe.build_plan(rp_d, col_d, bp, e2c, ht, num_columns=num_columns, **p)
    return dict(rp=rp, col=col, N=N, E=E, args=(rp_d, col_d, bp, e2c, e2r, ht, row_nzr, col_nzr))


def _setup(fe, dev, kind, form, sym=False):
    key = (fe.name, kind, form, sym)
    if key not in _CACHE:
        rp, col = _graph(kind)
        if sym:
            rp, col = _symmetric(rp, col)
        _CACHE[key] = _prepare(fe, dev, rp, col, form)
    return _CACHE[key]


def _tie_features(rng, rows, D, specials=True):
    """small integers (many ties), half of the zeros negative, and (specials) about 2 % NaN and 2 % +-inf"""
    X = rng.integers(-3, 4, (rows, D)).astype(np.float32)
    X[(X == 0) & (rng.random((rows, D)) < 0.5)] = -0.0
    if specials:
        u = rng.random((rows, D))
        X[u < 0.02] = np.nan
        X[(u >= 0.02) & (u < 0.03)] = np.inf
        X[(u >= 0.03) & (u < 0.04)] = -np.inf
    return X


def reference(rp, col, X, reduce):
    """sequential-scan semantics, vectorised: NaN first, then the largest (smallest) value, ties to the lowest entry"""
    N, E, D = len(rp) - 1, len(col), X.shape[1]
    Z = np.zeros((N, D), np.float32)
    arg = np.full((N, D), -1, np.int32)
    if E == 0:
        return Z, arg
    V = X[col]
    key = V if reduce == "max" else -V
    isn = np.isnan(key)
    nonempty = np.diff(rp) > 0
    starts = rp[:-1][nonempty]
    rows = np.repeat(np.arange(N), np.diff(rp))
    anyn = np.zeros((N, D), bool)
    anyn[nonempty] = np.logical_or.reduceat(isn, starts, axis=0)
    kf = np.where(isn, -np.inf, key)
    m = np.full((N, D), -np.inf, np.float32)
    m[nonempty] = np.maximum.reduceat(kf, starts, axis=0)
    cand = np.where(anyn[rows], isn, ~isn & (kf == m[rows]))
    pos = np.where(cand, np.arange(E, dtype=np.int64)[:, None], np.int64(E))
    win = np.full((N, D), E, np.int64)
    win[nonempty] = np.minimum.reduceat(pos, starts, axis=0)
    ok = win < E
    dd = np.broadcast_to(np.arange(D), (N, D))
    Z[ok] = V[win[ok], dd[ok]]
    arg[ok] = win[ok]
    return Z, arg


def reference_sums(rp, col, X):
    """fp64 row sums of x, fl32(x * x), |x| and x^2 (the last two are the bounds' yardsticks); rows without entries give +0.
    A device sum never holds -0 (it starts at +0), hence the + 0.0"""
    N, D = len(rp) - 1, X.shape[1]
    out = [np.zeros((N, D), np.float64) for _ in range(4)]
    if len(col) == 0:
        return out
    V = X[col]
    nonempty = np.diff(rp) > 0
    starts = rp[:-1][nonempty]
    V64 = V.astype(np.float64)
    for o, term in zip(out, (V64, (V * V).astype(np.float64), np.abs(V64), V64 * V64)):
        o[nonempty] = np.add.reduceat(term, starts, axis=0) + 0.0
    return out


def _refs(kind, g, D, data):
    """X and its references for one graph and width: data = "int" (small integers, signed zeros), "special" (the same with
    NaN and +-inf) or "randn" """
    key = (kind, D, data)
    if key not in _REFS:
        rng = np.random.default_rng(1000 * KINDS.index(kind) + D + {"int": 0, "special": 300, "randn": 600}[data])
        rows = g["N"]
        X = rng.standard_normal((rows, D)).astype(np.float32) if data == "randn" else _tie_features(rng, rows, D, data == "special")
        r = dict(max=reference(g["rp"], g["col"], X, "max"), min=reference(g["rp"], g["col"], X, "min"))
        if data != "special":
            r["sum"], r["sumsq"], r["abs"], r["sq"] = reference_sums(g["rp"], g["col"], X)
        _REFS[key] = (X, r)
    return _REFS[key]


def _bits_equal(got, want):
    return np.array_equal(got.view(np.int32), want.view(np.int32))


def _np(t):
    return t.cpu().numpy()


def _check_extrema(out, r, tag):
    for k, name in ((2, "max"), (3, "min")):
        assert np.array_equal(_np(out[k + 2]), r[name][1]), tag + (name, "arg")
        assert _bits_equal(_np(out[k]), r[name][0]), tag + (name,)


@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_all_six_outputs_bit_for_bit_on_integer_data(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    for D in WIDTHS:
        X, r = _refs(kind, g, D, "int")
        out = fe.forward_multi(torch.from_numpy(X).to(dev), *g["args"])
        assert len(out) == 6 and all(o.shape == (g["N"], D) and o.is_contiguous() for o in out)
        assert [o.dtype for o in out] == [torch.float32] * 4 + [torch.int32] * 2
        _check_extrema(out, r, (kind, form, D))
        assert _bits_equal(_np(out[0]), r["sum"].astype(np.float32)), (kind, form, D, "sum")
        assert _bits_equal(_np(out[1]), r["sumsq"].astype(np.float32)), (kind, form, D, "sumsq")


@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_specials_keep_the_extremum_contract(fe, dev, kind, form):
    """NaN and +-inf among the inputs: max, min and both args stay bit-exact (the sums are not compared here)"""
    g = _setup(fe, dev, kind, form)
    for D in WIDTHS:
        X, r = _refs(kind, g, D, "special")
        out = fe.forward_multi(torch.from_numpy(X).to(dev), *g["args"])
        _check_extrema(out, r, (kind, form, D))


@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_continuous_data_bounds_determinism_and_the_existing_launches(fe, dev, kind, form):
    """randn: max / min / args bit-exact and equal to forward_max / forward_min; sum within 1e-5 * sum|x_e| and sumsq within
    1e-5 * sum x_e^2 of fp64, per element; two calls give the same bits"""
    g = _setup(fe, dev, kind, form)
    for D in WIDTHS:
        X, r = _refs(kind, g, D, "randn")
        Xd = torch.from_numpy(X).to(dev)
        out = fe.forward_multi(Xd, *g["args"])
        _check_extrema(out, r, (kind, form, D))
        for k, name, bar in ((0, "sum", "abs"), (1, "sumsq", "sq")):
            err = np.abs(_np(out[k]).astype(np.float64) - r[name])
            assert (err <= 1e-5 * r[bar]).all(), (kind, form, D, name, float((err / np.maximum(r[bar], 1e-300)).max()))
        again = fe.forward_multi(Xd, *g["args"])
        for a, b in zip(out, again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (kind, form, D)
        zx, ax = fe.forward_max(Xd, *g["args"])
        zn, an = fe.forward_min(Xd, *g["args"])
        for a, b in ((out[2], zx), (out[3], zn), (out[4], ax), (out[5], an)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (kind, form, D)


NAMES = ("sum", "sumsq", "max", "min")


@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_subsets_of_the_aggregates(fe, dev, form):
    """each single aggregate, with and without args, is the corresponding output of the all-outputs call; the rest is None"""
    g = _setup(fe, dev, "powerlaw", form)
    for D in (3, 32):
        Xd = torch.from_numpy(_refs("powerlaw", g, D, "randn")[0]).to(dev)
        full = fe.forward_multi(Xd, *g["args"])
        for k, name in enumerate(NAMES):
            for return_arg in (True, False):
                out = fe.forward_multi(Xd, *g["args"], aggregates=(name,), return_arg=return_arg)
                assert len(out) == 6
                have = {k} | ({k + 2} if (k >= 2 and return_arg) else set())
                for i in range(6):
                    if i in have:
                        assert torch.equal(out[i].view(torch.int32), full[i].view(torch.int32)), (form, D, name, return_arg, i)
                    else:
                        assert out[i] is None, (form, D, name, return_arg, i)
        pair = fe.forward_multi(Xd, *g["args"], aggregates=("min", "sum"), return_arg=True)
        assert [o is None for o in pair] == [False, True, True, False, True, False]
        assert torch.equal(pair[5], full[5]) and torch.equal(pair[0].view(torch.int32), full[0].view(torch.int32))


def _direct(g, Xd, D, zs, ldz, args, ldarg):
    """hcspmm_forward_multi through ctypes directly: zs / args = data pointers (or None) of the six outputs"""
    import hcspmm
    from hcspmm import capi
    c = hcspmm._planned_call(g["args"][:6], g["args"][6], D, Xd.size(0), Xd.device, ws_fn=hcspmm._ws_bytes_multi)
    vp = [ctypes.c_void_p(p or 0) for p in list(zs) + list(args)]
    with c:
        rc = capi.lib().hcspmm_forward_multi(ctypes.c_void_p(Xd.data_ptr()), Xd.size(0), Xd.stride(0), 0, *vp[:4], ldz, *vp[4:], ldarg,
                                             *c.graph, *c.ws)
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["default", "plan_free"])
def test_null_outputs_and_guard_columns(dev, form):
    """outputs inside wider buffers (row strides beyond D, bases off the 16-byte grid): the columns around them keep their
    sentinel, and an output left NULL changes nothing of the others.  Through ctypes only: the test hands raw pointers to the
    C entry point (both front-ends allocate their own contiguous outputs)"""
    fe = frontends.get("ctypes")
    g = _setup(fe, dev, "powerlaw", form)
    N = g["N"]
    for D in (3, 22, 64):
        Xd = torch.from_numpy(_refs("powerlaw", g, D, "randn")[0]).to(dev)
        full = fe.forward_multi(Xd, *g["args"])
        for subset in ((0, 1, 2, 3), (0,), (1, 3), (2,)):
            ldz, ldarg = D + 9, D + 6
            Zb = [torch.full((N, ldz), -777.0, device=dev) for _ in range(4)]
            Ab = [torch.full((N, ldarg), -777, dtype=torch.int32, device=dev) for _ in range(2)]
            zs = [Zb[k][:, 5:].data_ptr() if k in subset else None for k in range(4)]
            ar = [Ab[k - 2][:, 3:].data_ptr() if k in subset else None for k in (2, 3)]
            _direct(g, Xd, D, zs, ldz, ar, ldarg)
            for k in range(4):
                inner = Zb[k][:, 5:5 + D]
                if k in subset:
                    assert torch.equal(inner.contiguous().view(torch.int32), full[k].view(torch.int32)), (form, D, subset, k)
                    assert (Zb[k][:, :5] == -777.0).all() and (Zb[k][:, 5 + D:] == -777.0).all(), (form, D, subset, k)
                else:
                    assert (Zb[k] == -777.0).all(), (form, D, subset, k)
            for k in (2, 3):
                inner = Ab[k - 2][:, 3:3 + D]
                if k in subset:
                    assert torch.equal(inner, full[k + 2]), (form, D, subset, k)
                    assert (Ab[k - 2][:, :3] == -777).all() and (Ab[k - 2][:, 3 + D:] == -777).all(), (form, D, subset, k)
                else:
                    assert (Ab[k - 2] == -777).all(), (form, D, subset, k)


@pytest.mark.parametrize("form", ["default", "slices", "plan_free"])
def test_concatenated_layout(dev, form):
    """one [N, 4 D] buffer with ldz = 4 D (and one [N, 2 D] buffer of args) is the same call with pointers D apart.
    Through ctypes only: the test hands raw pointers to the C entry point"""
    fe = frontends.get("ctypes")
    g = _setup(fe, dev, "powerlaw", form)
    N = g["N"]
    for D in (3, 22, 64):
        Xd = torch.from_numpy(_refs("powerlaw", g, D, "randn")[0]).to(dev)
        full = fe.forward_multi(Xd, *g["args"])
        Z = torch.empty((N, 4 * D), device=dev)
        A = torch.empty((N, 2 * D), dtype=torch.int32, device=dev)
        _direct(g, Xd, D, [Z.data_ptr() + 4 * D * k for k in range(4)], 4 * D, [A.data_ptr() + 4 * D * k for k in range(2)], 2 * D)
        assert torch.equal(Z.view(torch.int32), torch.cat(full[:4], 1).view(torch.int32)), (form, D)
        assert torch.equal(A, torch.cat(full[4:], 1)), (form, D)


@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_empty_rows_duplicate_columns_and_a_hub(fe, dev, form):
    """rows without entries give +0 in all four values and -1 in both args; a column stored twice in a row counts twice in
    the sums and ties with itself in the extrema (the first copy wins); one row of 600 entries is split into segments"""
    rng = np.random.default_rng(33)
    N = 700
    deg = rng.integers(0, 12, N)
    deg[::7] = 0
    deg[5] = 600  # a hub: split into segments
    rows = np.repeat(np.arange(N), deg)
    cols = rng.integers(0, N, rows.size)
    cols[::5] = cols[np.maximum(np.arange(0, rows.size, 5) - 1, 0)]  # duplicates of the previous entry's column
    rp, col = _csr(rows, cols, N)
    g = _prepare(fe, dev, rp, col, form)
    empty = np.diff(rp) == 0
    for D in (3, 32, 64):
        X = _tie_features(rng, N, D, specials=False)
        out = fe.forward_multi(torch.from_numpy(X).to(dev), *g["args"])
        r = dict(max=reference(rp, col, X, "max"), min=reference(rp, col, X, "min"))
        _check_extrema(out, r, (form, D))
        s, q, _, _ = reference_sums(rp, col, X)
        assert _bits_equal(_np(out[0]), s.astype(np.float32)) and _bits_equal(_np(out[1]), q.astype(np.float32)), (form, D)
        for k in range(4):
            assert _bits_equal(_np(out[k])[empty], np.zeros((empty.sum(), D), np.float32)), (form, D, k)
        assert (_np(out[4])[empty] == -1).all() and (_np(out[5])[empty] == -1).all()
        Xs = _tie_features(rng, N, D)  # with NaN and +-inf
        out = fe.forward_multi(torch.from_numpy(Xs).to(dev), *g["args"])
        _check_extrema(out, dict(max=reference(rp, col, Xs, "max"), min=reference(rp, col, Xs, "min")), (form, D, "specials"))


@pytest.mark.parametrize("form", ["default", "slices", "plan_free"])
def test_rectangular_and_strided_input(fe, dev, form):
    """a row block of a graph whose column ids index a taller X, read through a column-slice view of a wider matrix"""
    rp_full, col_full = graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    n = 1200
    rp, col = rp_full[:n + 1].copy(), col_full[:rp_full[n]].copy()
    g = _prepare(fe, dev, rp, col, form, num_columns=3000)
    rng = np.random.default_rng(34)
    for D in (3, 22, 64):
        X = _tie_features(rng, 3000, D, specials=False)
        wide = torch.zeros(3000, D + 13, device=dev)
        wide[:, 5:5 + D] = torch.from_numpy(X).to(dev)
        out = fe.forward_multi(wide[:, 5:5 + D], *g["args"])
        assert all(o.shape == (n, D) for o in out)
        _check_extrema(out, dict(max=reference(rp, col, X, "max"), min=reference(rp, col, X, "min")), (form, D))
        s, q, _, _ = reference_sums(rp, col, X)
        assert _bits_equal(_np(out[0]), s.astype(np.float32)) and _bits_equal(_np(out[1]), q.astype(np.float32)), (form, D)


def _torch_pna(X, W_root, W_neigh, rp, col):
    """PNAConv with its default aggregators and scalers from index_add / scatter_reduce, in X's dtype"""
    N, D = rp.numel() - 1, X.size(1)
    lens = (rp[1:] - rp[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(N, device=X.device), lens)
    src = X.index_select(0, col.long())
    idx = rows[:, None].expand_as(src)
    zero = torch.zeros(N, D, dtype=X.dtype, device=X.device)
    s = zero.index_add(0, rows, src)
    q = zero.index_add(0, rows, src * src)
    mx = zero.scatter_reduce(0, idx, src, "amax", include_self=False)
    mn = zero.scatter_reduce(0, idx, src, "amin", include_self=False)
    deg = lens.clamp(min=1).to(X.dtype)[:, None]
    log_deg = torch.log(deg + 1)
    delta = log_deg.mean()
    mean = s / deg
    std = torch.sqrt(torch.relu(q / deg - mean * mean) + 1e-5)
    base = torch.cat([mean, mn, mx, std], 1)
    S = torch.cat([base, base * (log_deg / delta), base * (delta / log_deg)], 1)
    return X @ W_root + S @ W_neigh


def _asymmetric(n=1500, per_row=6, seed=37):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row)
    pairs = np.unique(np.stack([rows, (rows + rng.integers(1, n // 2, rows.size)) % n], 1), axis=0)
    return _csr(pairs[:, 0], pairs[:, 1], n)


@pytest.mark.parametrize("kind", ["powerlaw", "planted", "molecule", "asymmetric"])
def test_pnaconv_matches_a_torch_layer(dev, kind):
    """forward, X.grad and both weight gradients against the same layer in torch.  The reference is that layer in fp64; the
    yardstick is the fp32 torch layer's own maximum error against it: the library layer may err by at most 4 x that plus
    1e-6 * max|ref| (two fp32 evaluations that differ in summation order err alike; 4 allows for an unlucky order)."""
    _pkg_imports()
    import GNN_model
    ext = frontends.get("extension")
    directed = kind == "asymmetric"
    g = _prepare(ext, dev, *_asymmetric(), "default") if directed else _setup(ext, dev, kind, "default", sym=True)
    torch.manual_seed(35)
    conv = GNN_model.PNAConv(24, 16, directed=directed).to(dev)
    X = torch.randn(g["N"], 24, device=dev, requires_grad=True)
    out = conv(X, *g["args"], None)
    dY = torch.randn_like(out)
    out.backward(dY)
    rp, col = g["args"][0], g["args"][1]
    results = {}
    for dtype in (torch.float64, torch.float32):
        Xr, Wr, Wn = (t.detach().to(dtype).requires_grad_(True) for t in (X, conv.weights_root, conv.weights_neigh))
        o = _torch_pna(Xr, Wr, Wn, rp, col)
        o.backward(dY.to(dtype))
        results[dtype] = (o.detach(), Xr.grad, Wr.grad, Wn.grad)
    mine = (out.detach(), X.grad, conv.weights_root.grad, conv.weights_neigh.grad)
    for name, m, t32, t64 in zip(("out", "X.grad", "W_root.grad", "W_neigh.grad"), mine, results[torch.float32], results[torch.float64]):
        yard = float((t32.double() - t64).abs().max())
        err = float((m.double() - t64).abs().max())
        bound = 4.0 * yard + 1e-6 * float(t64.abs().max())
        print("%s %s: library error %.3e, fp32 torch error %.3e, bound %.3e" % (kind, name, err, yard, bound))
        assert err <= bound, (kind, name, err, yard, bound)


def test_refusals(fe, dev):
    _pkg_imports()
    import GNN_model
    g = _prepare(frontends.get("extension"), dev, *_asymmetric(200, 3, 36), "default")
    X = torch.randn(200, 8, device=dev)
    with pytest.raises(RuntimeError, match="symmetric"):
        GNN_model.PNAConv(8, 8).to(dev)(X, *g["args"], None)
    with pytest.raises(RuntimeError, match="symmetric"):
        GNN_model.multi_aggregate(X, g["args"])
    with pytest.raises(ValueError):
        GNN_model.PNAConv(8, 8, directed=True).to(dev)(X, *g["args"], None, edge_weight=torch.ones(len(g["col"]), device=dev))
    h = _setup(fe, dev, "uniform", "default")
    Xu = torch.randn(h["N"], 8, device=dev)
    with pytest.raises(RuntimeError):
        fe.forward_multi(Xu.cpu(), *h["args"])
    with pytest.raises(RuntimeError):
        fe.forward_multi(Xu.half(), *h["args"])
    with pytest.raises(ValueError):
        fe.forward_multi(Xu, *h["args"], aggregates=("sum", "median"))
    with pytest.raises(ValueError):
        fe.forward_multi(Xu, *h["args"], aggregates=())
