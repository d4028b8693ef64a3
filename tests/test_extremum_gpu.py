"""Max / min neighbour aggregation with its argmax (hcspmm_forward_extremum), its backward and the SAGEConv layer built on
them, on an MI355X through both Python front-ends.

The contract (include/hcspmm.h): Z and arg are the bits of a sequential scan of each row -- ties to the lowest entry (-0 ==
+0), NaN beats every number for max and min alike, rows without entries give +0 and -1 -- on every plan form and split.
Checked with torch.equal against a numpy reference on inputs built to tie: small integers, signed zeros, NaN and +-inf.
"""
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


def reference_backward(rp, col, G, arg):
    N, D = G.shape
    out = np.zeros((N, D), np.float32)
    i, d = np.nonzero(arg >= 0)
    np.add.at(out, (col[arg[i, d]], d), G[i, d])
    return out


def _bits_equal(got, want):
    return np.array_equal(got.view(np.int32), want.view(np.int32))


def _fn(fe, reduce):
    return fe.forward_max if reduce == "max" else fe.forward_min


@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_forward_bits_and_arg(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    rng = np.random.default_rng(31)
    for D in WIDTHS:
        X = _tie_features(rng, g["N"], D)
        Xd = torch.from_numpy(X).to(dev)
        for reduce in ("max", "min"):
            Z, arg = _fn(fe, reduce)(Xd, *g["args"])
            wz, wa = reference(g["rp"], g["col"], X, reduce)
            assert torch.equal(arg.cpu(), torch.from_numpy(wa)), (kind, form, D, reduce)
            assert _bits_equal(Z.cpu().numpy(), wz), (kind, form, D, reduce)
            Z1 = _fn(fe, reduce)(Xd, *g["args"], return_arg=False)
            assert len(Z1) == 1 and _bits_equal(Z1[0].cpu().numpy(), wz), (kind, form, D, reduce)


@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_backward_bits_and_determinism(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form, sym=True)
    perm = fe.transpose_permutation(g["args"][0], g["args"][1]).to(torch.int32)
    rng = np.random.default_rng(32)
    for D in WIDTHS:
        X = _tie_features(rng, g["N"], D)
        G = rng.integers(-8, 9, (g["N"], D)).astype(np.float32)
        Gd = torch.from_numpy(G).to(dev)
        for reduce in ("max", "min"):
            _, arg = _fn(fe, reduce)(torch.from_numpy(X).to(dev), *g["args"])
            got = fe.forward_extremum_backward(Gd, arg, perm, *g["args"])
            want = reference_backward(g["rp"], g["col"], G, arg.cpu().numpy())
            assert _bits_equal(got.cpu().numpy(), want), (kind, form, D, reduce)
            again = fe.forward_extremum_backward(Gd, arg, perm, *g["args"])
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (kind, form, D, reduce)


@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_empty_rows_and_duplicate_columns(fe, dev, form):
    """rows without entries give +0 / -1; a column stored twice in a row (preprocess accepts non-decreasing rows) ties
    with itself, and the first copy wins"""
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
    for D in (3, 32, 64):
        X = _tie_features(rng, N, D)
        for reduce in ("max", "min"):
            Z, arg = _fn(fe, reduce)(torch.from_numpy(X).to(dev), *g["args"])
            wz, wa = reference(rp, col, X, reduce)
            assert torch.equal(arg.cpu(), torch.from_numpy(wa)), (form, D, reduce)
            assert _bits_equal(Z.cpu().numpy(), wz), (form, D, reduce)
            empty = np.diff(rp) == 0
            assert (wa[empty] == -1).all() and _bits_equal(Z.cpu().numpy()[empty], np.zeros((empty.sum(), D), np.float32))


@pytest.mark.parametrize("form", ["default", "slices", "plan_free"])
def test_rectangular_and_strided_input(fe, dev, form):
    """a row block of a graph whose column ids index a taller X, read through a column-slice view of a wider matrix"""
    rp_full, col_full = graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    n = 1200
    rp, col = rp_full[:n + 1].copy(), col_full[:rp_full[n]].copy()
    g = _prepare(fe, dev, rp, col, form, num_columns=3000)
    rng = np.random.default_rng(34)
    for D in (3, 22, 64):
        X = _tie_features(rng, 3000, D)
        wide = torch.zeros(3000, D + 13, device=dev)
        wide[:, 5:5 + D] = torch.from_numpy(X).to(dev)
        view = wide[:, 5:5 + D]
        for reduce in ("max", "min"):
            Z, arg = _fn(fe, reduce)(view, *g["args"])
            wz, wa = reference(rp, col, X, reduce)
            assert Z.shape == (n, D)
            assert torch.equal(arg.cpu(), torch.from_numpy(wa)), (form, D, reduce)
            assert _bits_equal(Z.cpu().numpy(), wz), (form, D, reduce)


def _torch_sage(X, W_root, W_neigh, rp, col, reduce):
    N = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(N, device=X.device), (rp[1:] - rp[:-1]).long())
    src = X.index_select(0, col.long())
    agg = torch.zeros(N, X.size(1), device=X.device).scatter_reduce(0, rows[:, None].expand_as(src), src,
                                                                     "amax" if reduce == "max" else "amin", include_self=False)
    return X @ W_root + agg @ W_neigh


@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("kind", ["powerlaw", "planted", "molecule"])
def test_sageconv_matches_a_torch_layer(dev, kind, reduce):
    _pkg_imports()
    import GNN_model
    g = _setup(frontends.get("extension"), dev, kind, "default", sym=True)
    torch.manual_seed(35)
    conv = GNN_model.SAGEConv(24, 16, aggr=reduce).to(dev)
    X = torch.randn(g["N"], 24, device=dev, requires_grad=True)  # continuous data: no ties
    out = conv(X, *g["args"], None)
    rp, col = g["args"][0], g["args"][1]
    Xr = X.detach().clone().requires_grad_(True)
    Wr = conv.weights_root.detach().clone().requires_grad_(True)
    Wn = conv.weights_neigh.detach().clone().requires_grad_(True)
    ref = _torch_sage(Xr, Wr, Wn, rp, col, reduce)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
    dY = torch.randn_like(out)
    out.backward(dY)
    ref.backward(dY)
    torch.testing.assert_close(X.grad, Xr.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(conv.weights_root.grad, Wr.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(conv.weights_neigh.grad, Wn.grad, rtol=1e-5, atol=1e-5)


def test_sageconv_refuses_an_asymmetric_pattern_and_edge_weight(dev):
    _pkg_imports()
    import GNN_model
    rng = np.random.default_rng(36)
    rows = np.repeat(np.arange(200), 3)
    rp, col = _csr(rows, (rows + rng.integers(1, 50, rows.size)) % 200, 200)
    g = _prepare(frontends.get("extension"), dev, rp, col, "default")
    conv = GNN_model.SAGEConv(8, 8).to(dev)
    X = torch.randn(200, 8, device=dev)
    with pytest.raises(RuntimeError, match="symmetric"):
        conv(X, *g["args"], None)
    with pytest.raises(ValueError):
        conv(X, *g["args"], None, edge_weight=torch.ones(len(col), device=dev))
