"""Per-channel softmax aggregation in one gather pass (hcspmm_forward_softmax), its backward (hcspmm_softmax_backward), the
SoftmaxAggregate function and the GENConv layer built on them, on an MI355X through both Python front-ends.

The contract (include/hcspmm.h): Z = sum_e p_e x_e with p the softmax over a row's entries of s_e = fl(beta x_e); M = max s_e bit
for bit, L = sum exp(s_e - M), Q = sum p_e fl(x_e x_e); rows without entries give +0, -inf, 0, +0; a NULL statistic is not
written; a fixed order, so two calls give the same bits.  Integer data make several cases exact: beta = +-1000 is the max / min
(every weight is 0 or 1), beta = 0 the mean of an exact sum, a row of one entry its own entry.

Continuous data follow the project's rule for order-dependent fp32 results: the reference is the formula in fp64, the yardstick
the same formula in fp32 numpy (two passes, sequential sums), and the library may err by at most 4 x the yardstick's own maximum
error plus 1e-6 * max|ref| -- taken separately over rows of at most 64 entries and over longer rows.
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
KIND_FORM = [(k, f) for k in KINDS for f in PLANS]  # kind-major: the references of one graph are computed once and then dropped
FRONTENDS = ["ctypes", "extension"]  # (the innermost parameter of the tests that share those references)

_CACHE = {}
_REFS = {}  # (what, graph kind, D, beta name) -> references of the CURRENT graph kind (a new kind evicts the previous one's)


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


def _np(t):
    return t.cpu().numpy()


def _bits_equal(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32))


BETAS = ("0.5", "2", "-3", "vector")


def _beta(name, D):
    """float32 [D]: one of the scalars, or a seeded per-column vector in [-2, 2]"""
    if name == "vector":
        return np.random.default_rng(900 + D).uniform(-2.0, 2.0, D).astype(np.float32)
    return np.full(D, float(name), np.float32)


def _beta_arg(name, b, dev):
    """what the front-ends are handed: a Python float, or the float32 [D] device tensor"""
    return torch.from_numpy(b).to(dev) if name == "vector" else float(name)


def _segments(rp):
    lens = np.diff(rp)
    nonempty = lens > 0
    return lens, nonempty, rp[:-1][nonempty], np.repeat(np.arange(len(rp) - 1), lens)


def _sum_rows(term, rp):
    """row sums of the per-entry terms.  float64 (the reference): np.add.reduceat.  float32 (the yardstick): entry after entry
    in CSR order, each partial sum rounded to fp32 -- reduceat is NOT that (it comes out closer to the exact sum), so the k-th
    entries of all rows that have one are added in step k"""
    N = len(rp) - 1
    lens = np.diff(rp)
    out = np.zeros((N, term.shape[1]), term.dtype)
    if term.dtype == np.float64:
        nonempty = lens > 0
        if nonempty.any():
            out[nonempty] = np.add.reduceat(term, rp[:-1][nonempty], axis=0)
        return out
    order = np.argsort(-lens, kind="stable")  # longest rows first: the rows that still have a k-th entry are a prefix
    starts, sorted_lens = rp[:-1][order].astype(np.int64), lens[order]
    acc = np.zeros_like(out)
    for k in range(int(lens.max()) if N else 0):
        n = int(np.searchsorted(-sorted_lens, -k, side="left"))  # rows with more than k entries
        acc[:n] = acc[:n] + term[starts[:n] + k]
    out[order] = acc
    return out


def row_max(rp, col, X, b):
    """M: max over each row of fl32(beta x), -inf on rows without entries (exact: no rounding beyond the product's)"""
    N = len(rp) - 1
    _, nonempty, starts, _ = _segments(rp)
    s = X[col] * b[None, :]
    M = np.full((N, X.shape[1]), -np.inf, np.float32)
    if len(starts):
        M[nonempty] = np.maximum.reduceat(s, starts, axis=0)
    return M, s


def forward_reference(rp, col, X, b, dtype, Ms=None):
    """(Z, L, Q) of the formula in `dtype` arithmetic (float64: the reference; float32: the yardstick, two passes with sequential
    sums); rows without entries give 0.  Ms: row_max's result, when the caller has it"""
    N = len(rp) - 1
    _, nonempty, starts, rows = _segments(rp)
    M, s = Ms if Ms is not None else row_max(rp, col, X, b)
    V = X[col].astype(dtype)
    w = np.exp(s.astype(dtype) - M[rows].astype(dtype))
    L = _sum_rows(w, rp)
    safe = np.where(L > 0, L, 1).astype(dtype)
    return _sum_rows(w * V, rp) / safe, L, _sum_rows(w * (V * V), rp) / safe


def backward_reference(rp, col, G, Z, M, L, X, b, dtype):
    """dX of the formula in `dtype` arithmetic on the walked graph (rp, col): row j sums over its entries (j, i)"""
    N = len(rp) - 1
    _, nonempty, starts, rows = _segments(rp)
    bt = b.astype(dtype)[None, :]
    x = X.astype(dtype)[rows]
    s = (X * b[None, :])[rows].astype(dtype)  # fl32(beta x), as the kernels and the forward form it
    term = np.exp(s - M[col].astype(dtype)) / L[col].astype(dtype) * G[col].astype(dtype) * (1 + bt * (x - Z[col].astype(dtype)))
    return _sum_rows(term, rp)


def _bounds(ref64, yard32, lens):
    """per row group (0: at most 64 entries, 1: longer): (group, mask, 4 x the yardstick's maximum error + 1e-6 * max|ref|, that error)"""
    out = []
    floor = 1e-6 * float(np.abs(ref64).max()) if ref64.size else 0.0
    yerr = np.abs(yard32.astype(np.float64) - ref64)
    for k, mask in enumerate((lens <= 64, lens > 64)):
        if mask.any():
            y = float(yerr[mask].max())
            out.append((k, mask, 4.0 * y + floor, y))
    return out


def _check_bound(got, ref64, bounds, tag, worst):
    err = np.abs(got.astype(np.float64) - ref64)
    for k, mask, bound, yard in bounds:
        e = float(err[mask].max())
        worst[tag[-1]] = max(worst.get(tag[-1], 0.0), e / bound if bound > 0 else 0.0)
        print("library error %.3e, yardstick %.3e, bound %.3e: %s %s" % (e, yard, bound, tag, ("rows <= 64", "rows > 64")[k]))
        assert e <= bound, (tag, e, yard, bound)


def _evict(kind):
    for k in [k for k in _REFS if k[1] != kind]:
        del _REFS[k]


def _forward_refs(kind, g, D, bname):
    key = ("fwd", kind, D, bname)
    if key not in _REFS:
        _evict(kind)
        rng = np.random.default_rng(2000 * KINDS.index(kind) + D)
        X = rng.standard_normal((g["N"], D)).astype(np.float32)
        b = _beta(bname, D)
        lens = np.diff(g["rp"])
        Ms = row_max(g["rp"], g["col"], X, b)
        r64 = forward_reference(g["rp"], g["col"], X, b, np.float64, Ms)
        y32 = forward_reference(g["rp"], g["col"], X, b, np.float32, Ms)
        _REFS[key] = (X, b, Ms[0], r64, [_bounds(r, y, lens) for r, y in zip(r64, y32)])
    return _REFS[key]


def _backward_refs(kind, g, D, bname):
    """synthetic operands of the backward launch on the walked graph g: any G and Z, L >= 1, and M at or above every beta x of
    its column (as the forward's maxima are for the entries that reach them), so the exponent is never positive"""
    key = ("bwd", kind, D, bname)
    if key not in _REFS:
        _evict(kind)
        rng = np.random.default_rng(3000 * KINDS.index(kind) + D)
        n = g["N"]
        X = rng.standard_normal((n, D)).astype(np.float32)
        b = _beta(bname, D)
        G = rng.standard_normal((n, D)).astype(np.float32)
        Z = rng.standard_normal((n, D)).astype(np.float32)
        L = rng.uniform(1.0, 20.0, (n, D)).astype(np.float32)
        M = ((X * b[None, :]).max(0, keepdims=True) + rng.uniform(0.0, 0.5, (n, D))).astype(np.float32)
        lens = np.diff(g["rp"])
        r64 = backward_reference(g["rp"], g["col"], G, Z, M, L, X, b, np.float64)
        y32 = backward_reference(g["rp"], g["col"], G, Z, M, L, X, b, np.float32)
        _REFS[key] = (X, b, G, Z, M, L, r64, _bounds(r64, y32, lens))
    return _REFS[key]


@pytest.mark.parametrize("fe_name", FRONTENDS)
@pytest.mark.parametrize("kind,form", KIND_FORM)
def test_forward_on_continuous_data(fe_name, dev, kind, form):
    """randn features, beta in {0.5, 2, -3} and a per-column vector: M numerically equal to max fl32(beta x) everywhere; Z, L, Q
    within 4 x the fp32 yardstick's error + 1e-6 max|ref| of fp64, per row group; two calls give the same bits"""
    fe = frontends.get(fe_name)
    g = _setup(fe, dev, kind, form)
    worst = {}
    for D in WIDTHS:
        for bname in BETAS:
            X, b, M, (Z64, L64, Q64), bounds = _forward_refs(kind, g, D, bname)
            Xd = torch.from_numpy(X).to(dev)
            out = fe.forward_softmax(Xd, _beta_arg(bname, b, dev), *g["args"])
            assert len(out) == 4 and all(o.shape == (g["N"], D) and o.is_contiguous() and o.dtype == torch.float32 for o in out)
            tag = (kind, form, D, bname)
            assert np.array_equal(_np(out[1]), M), tag
            for o, ref, bd, name in ((out[0], Z64, bounds[0], "Z"), (out[2], L64, bounds[1], "L"), (out[3], Q64, bounds[2], "Q")):
                _check_bound(_np(o), ref, bd, tag + (name,), worst)
            if bname == "vector":
                again = fe.forward_softmax(Xd, _beta_arg(bname, b, dev), *g["args"])
                for x, y in zip(out, again):
                    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), tag
    print("largest error / bound: %s" % {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("fe_name", FRONTENDS)
@pytest.mark.parametrize("kind,form", KIND_FORM)
def test_backward_on_continuous_data(fe_name, dev, kind, form):
    """softmax_backward as the function of its operands that hcspmm.h states, on every graph and plan form as the walked graph:
    dX within the same bound; two calls give the same bits"""
    fe = frontends.get(fe_name)
    g = _setup(fe, dev, kind, form)
    worst = {}
    for D in WIDTHS:
        for bname in BETAS:
            X, b, G, Z, M, L, r64, bounds = _backward_refs(kind, g, D, bname)
            Gd, Zd, Md, Ld, Xd = (torch.from_numpy(v).to(dev) for v in (G, Z, M, L, X))
            dX = fe.softmax_backward(Gd, Zd, Md, Ld, Xd, _beta_arg(bname, b, dev), *g["args"])
            assert dX.shape == (g["N"], D) and dX.dtype == torch.float32 and dX.is_contiguous()
            _check_bound(_np(dX), r64, bounds, (kind, form, D, bname, "dX"), worst)
            if bname == "vector":
                again = fe.softmax_backward(Gd, Zd, Md, Ld, Xd, _beta_arg(bname, b, dev), *g["args"])
                assert torch.equal(dX.view(torch.int32), again.view(torch.int32)), (kind, form, D)
    print("largest error / bound: %s" % {k: round(v, 3) for k, v in worst.items()})


def _integers(rng, rows, D):
    return rng.integers(-3, 4, (rows, D)).astype(np.float32)


@pytest.mark.parametrize("fe_name", FRONTENDS)
@pytest.mark.parametrize("kind,form", KIND_FORM)
def test_exact_cases_on_integer_data(fe_name, dev, kind, form):
    """integers in [-3, 3]: beta = 1000 gives forward_max's values and beta = -1000 forward_min's, everything finite (without
    the running maximum this overflows); beta = 0 gives L = the row length and M = 0 exactly and Z within 1 ulp of
    fl(sum / n); rows of one entry give Z = x and Q = fl(x x) bit for bit and L = 1"""
    fe = frontends.get(fe_name)
    g = _setup(fe, dev, kind, form)
    lens, nonempty, starts, _ = _segments(g["rp"])
    one = lens == 1
    for D in WIDTHS:
        rng = np.random.default_rng(4000 * KINDS.index(kind) + D)
        X = _integers(rng, g["N"], D)
        Xd = torch.from_numpy(X).to(dev)
        for beta, ext in ((1000.0, fe.forward_max), (-1000.0, fe.forward_min)):
            Z, M, L, Q = (_np(o) for o in fe.forward_softmax(Xd, beta, *g["args"]))
            tag = (kind, form, D, beta)
            assert np.array_equal(Z, _np(ext(Xd, *g["args"], return_arg=False)[0])), tag
            assert np.isfinite(Z).all() and np.isfinite(L).all() and np.isfinite(Q).all() and np.isfinite(M[nonempty]).all(), tag
            assert np.array_equal(M[nonempty], beta * Z[nonempty]) and np.array_equal(Q, Z * Z), tag
        Z, M, L, Q = (_np(o) for o in fe.forward_softmax(Xd, 0.0, *g["args"]))
        tag = (kind, form, D, 0.0)
        assert np.array_equal(L, np.broadcast_to(lens[:, None].astype(np.float32), L.shape)), tag
        assert (M[nonempty] == 0).all() and np.isneginf(M[~nonempty]).all(), tag
        mean = (_sum_rows(X[g["col"]].astype(np.float64), g["rp"]) / np.maximum(lens, 1)[:, None]).astype(np.float32)
        assert (np.abs(Z - mean) <= np.spacing(np.abs(mean))).all(), tag
        # rows of one entry, on data without zeros (a sum never holds -0)
        Xr = rng.standard_normal((g["N"], D)).astype(np.float32)
        b = _beta("vector", D)
        Z, M, L, Q = (_np(o) for o in fe.forward_softmax(torch.from_numpy(Xr).to(dev), torch.from_numpy(b).to(dev), *g["args"]))
        x1 = Xr[g["col"][g["rp"][:-1][one]]]
        assert _bits_equal(Z[one], x1) and _bits_equal(Q[one], x1 * x1) and (L[one] == 1).all(), (kind, form, D, "one entry")
        assert _bits_equal(M[one], x1 * b[None, :]), (kind, form, D, "one entry")
    if kind in ("molecule", "uniform"):
        assert one.any()


def _hub_graph(rng, N=700):
    deg = rng.integers(0, 12, N)
    deg[::7] = 0
    deg[5] = 600  # a hub: split into segments
    rows = np.repeat(np.arange(N), deg)
    cols = rng.integers(0, N, rows.size)
    cols[::5] = cols[np.maximum(np.arange(0, rows.size, 5) - 1, 0)]  # duplicates of the previous entry's column
    return _csr(rows, cols, N)


@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_empty_rows_duplicate_columns_and_a_hub(fe, dev, form):
    """rows without entries give +0, -inf, 0, +0; a column stored twice in a row counts twice (L = the row length at beta = 0, and
    the bound against a reference that reads the stored entries as they are); one row of 600 entries is split into segments"""
    rng = np.random.default_rng(33)
    rp, col = _hub_graph(rng)
    N = len(rp) - 1
    g = _prepare(fe, dev, rp, col, form)
    lens = np.diff(rp)
    empty = lens == 0
    assert empty.any() and (lens == 1).any() and (np.diff(col)[np.diff(np.repeat(np.arange(N), lens)) == 0] == 0).any()
    worst = {}
    for D in (3, 32, 64):
        X = rng.standard_normal((N, D)).astype(np.float32)
        Xd = torch.from_numpy(X).to(dev)
        for bname in BETAS:
            b = _beta(bname, D)
            Z, M, L, Q = (_np(o) for o in fe.forward_softmax(Xd, _beta_arg(bname, b, dev), *g["args"]))
            zero = np.zeros((int(empty.sum()), D), np.float32)
            assert _bits_equal(Z[empty], zero) and _bits_equal(L[empty], zero) and _bits_equal(Q[empty], zero), (form, D, bname)
            assert np.isneginf(M[empty]).all() and np.array_equal(M, row_max(rp, col, X, b)[0]), (form, D, bname)
            r64 = forward_reference(rp, col, X, b, np.float64)
            y32 = forward_reference(rp, col, X, b, np.float32)
            for got, ref, yard, name in zip((Z, L, Q), r64, y32, "ZLQ"):
                _check_bound(got, ref, _bounds(ref, yard, lens), (form, D, bname, name), worst)
        L0 = _np(fe.forward_softmax(Xd, 0.0, *g["args"])[2])
        assert np.array_equal(L0, np.broadcast_to(lens[:, None].astype(np.float32), L0.shape)), (form, D)


@pytest.mark.parametrize("form", ["default", "slices", "plan_free"])
def test_rectangular_and_strided_input(fe, dev, form):
    """a row block of a graph whose column ids index a taller X, read through a column-slice view of a wider matrix"""
    rp_full, col_full = graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    n = 1200
    rp, col = rp_full[:n + 1].copy(), col_full[:rp_full[n]].copy()
    g = _prepare(fe, dev, rp, col, form, num_columns=3000)
    rng = np.random.default_rng(34)
    lens = np.diff(rp)
    worst = {}
    for D in (3, 22, 64):
        X = rng.standard_normal((3000, D)).astype(np.float32)
        b = _beta("vector", D)
        wide = torch.zeros(3000, D + 13, device=dev)
        wide[:, 5:5 + D] = torch.from_numpy(X).to(dev)
        out = fe.forward_softmax(wide[:, 5:5 + D], torch.from_numpy(b).to(dev), *g["args"])
        assert all(o.shape == (n, D) for o in out)
        assert np.array_equal(_np(out[1]), row_max(rp, col, X, b)[0]), (form, D)
        r64 = forward_reference(rp, col, X, b, np.float64)
        y32 = forward_reference(rp, col, X, b, np.float32)
        for got, ref, yard, name in zip((out[0], out[2], out[3]), r64, y32, "ZLQ"):
            _check_bound(_np(got), ref, _bounds(ref, yard, lens), (form, D, name), worst)


def _direct(g, Xd, bd, D, ptrs, ldz):
    """hcspmm_forward_softmax through ctypes directly: ptrs = data pointers (or None) of Z, M, L, Q"""
    import hcspmm
    from hcspmm import capi
    c = hcspmm._planned_call(g["args"][:6], g["args"][6], D, Xd.size(0), Xd.device, ws_fn=hcspmm._ws_bytes_softmax)
    vp = [ctypes.c_void_p(p or 0) for p in ptrs]
    with c:
        rc = capi.lib().hcspmm_forward_softmax(ctypes.c_void_p(Xd.data_ptr()), Xd.size(0), Xd.stride(0), 0,
                                               ctypes.c_void_p(bd.data_ptr()), *vp, ldz, *c.graph, *c.ws)
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["default", "plan_free"])
def test_null_statistics_and_guard_columns(dev, form):
    """outputs inside wider buffers (row strides beyond D, bases off the 16-byte grid): the columns around them keep their
    sentinel, and a statistic left NULL changes nothing of the others.  Through ctypes only: the test hands raw pointers to
    the C entry point (both front-ends allocate their own contiguous outputs)"""
    fe = frontends.get("ctypes")
    g = _setup(fe, dev, "powerlaw", form)
    N = g["N"]
    for D in (3, 22, 64):
        Xd = torch.randn(N, D, device=dev, generator=torch.Generator(device=dev).manual_seed(D))
        bd = torch.from_numpy(_beta("vector", D)).to(dev)
        full = fe.forward_softmax(Xd, bd, *g["args"])
        for subset in ((0, 1, 2, 3), (0,), (0, 2), (0, 1, 3)):
            ldz = D + 9
            buf = [torch.full((N, ldz), -777.0, device=dev) for _ in range(4)]
            _direct(g, Xd, bd, D, [buf[k][:, 5:].data_ptr() if k in subset else None for k in range(4)], ldz)
            for k in range(4):
                if k in subset:
                    inner = buf[k][:, 5:5 + D].contiguous()
                    assert torch.equal(inner.view(torch.int32), full[k].view(torch.int32)), (form, D, subset, k)
                    assert (buf[k][:, :5] == -777.0).all() and (buf[k][:, 5 + D:] == -777.0).all(), (form, D, subset, k)
                else:
                    assert (buf[k] == -777.0).all(), (form, D, subset, k)
        # the front-ends' return_stats: what is not asked for is None, the rest has the same bits
        for stats, have in ((False, (0,)), (0, (0,)), (np.bool_(True), (0, 1, 2, 3)), (("M", "L"), (0, 1, 2)), (("Q",), (0, 3)),
                            ("L", (0, 2))):
            out = fe.forward_softmax(Xd, bd, *g["args"], return_stats=stats)
            assert len(out) == 4
            for k in range(4):
                if k in have:
                    assert torch.equal(out[k].view(torch.int32), full[k].view(torch.int32)), (form, D, stats, k)
                else:
                    assert out[k] is None, (form, D, stats, k)


def test_return_stats_through_the_extension(dev):
    fe = frontends.get("extension")
    g = _setup(fe, dev, "uniform", "default")
    Xd = torch.randn(g["N"], 8, device=dev)
    full = fe.forward_softmax(Xd, 0.5, *g["args"])
    assert [o is None for o in fe.forward_softmax(Xd, 0.5, *g["args"], return_stats=False)] == [False, True, True, True]
    assert [o is None for o in fe.forward_softmax(Xd, 0.5, *g["args"], return_stats=np.bool_(False))] == [False, True, True, True]
    assert [o is None for o in fe.forward_softmax(Xd, 0.5, *g["args"], return_stats=1)] == [False] * 4
    assert [o is None for o in fe.forward_softmax(Xd, 0.5, *g["args"], return_stats="Q")] == [False, True, True, False]
    part = fe.forward_softmax(Xd, 0.5, *g["args"], return_stats=("M", "L"))
    assert part[3] is None and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(part[:3], full[:3]))
    with pytest.raises(ValueError):
        fe.forward_softmax(Xd, 0.5, *g["args"], return_stats=("S",))


def _transpose(rp, col, n_cols):
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return _csr(col.astype(np.int64), rows, n_cols)


@pytest.mark.parametrize("form", list(PLANS))
def test_backward_is_exact_where_every_row_has_one_entry(fe, dev, form):
    """A with exactly one entry per row: every softmax weight is 1 and Z[i] is its entry's x, so with integer G the backward on
    A^T -- whose rows have every length, one of them a hub -- equals the binary product forward(G) on A^T bit for bit"""
    rng = np.random.default_rng(41)
    N = 2000
    cols = rng.integers(0, N, N)
    cols[rng.random(N) < 0.3] = 7  # a hub column: row 7 of A^T is some 600 entries long
    rp, col = _csr(np.arange(N), cols, N)
    rp_t, col_t = _transpose(rp, col, N)
    lens_t = np.diff(rp_t)
    assert lens_t.max() > 400 and (lens_t == 0).any() and (lens_t == 1).any() and (lens_t == 2).any()
    g = _prepare(fe, dev, rp, col, "default")
    gt = _prepare(fe, dev, rp_t, col_t, form)
    for D in WIDTHS:
        X = rng.standard_normal((N, D)).astype(np.float32)
        G = _integers(rng, N, D)
        Xd, Gd = torch.from_numpy(X).to(dev), torch.from_numpy(G).to(dev)
        for bname in ("2", "vector"):
            b = _beta(bname, D)
            beta = _beta_arg(bname, b, dev)
            Z, M, L, Q = fe.forward_softmax(Xd, beta, *g["args"])
            assert _bits_equal(_np(Z), X[col]) and (_np(L) == 1).all(), (form, D, bname)
            dX = fe.softmax_backward(Gd, Z, M, L, Xd, beta, *gt["args"])
            want = fe.forward(Gd, *gt["args"])[0]
            assert torch.equal(dX.view(torch.int32), want.view(torch.int32)), (form, D, bname)


def _torch_gen(X, W, t, rp, col, eps=1e-7):
    """GENConv with the softmax aggregator from index_add / scatter_reduce, in X's dtype -> (out, Z, Q)"""
    N, D = rp.numel() - 1, X.size(1)
    lens = (rp[1:] - rp[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(N, device=X.device), lens)
    src = (torch.relu(X) + eps).index_select(0, col.long())
    s = t * src
    idx = rows[:, None].expand_as(s)
    m = torch.zeros(N, D, dtype=X.dtype, device=X.device).scatter_reduce(0, idx, s.detach(), "amax", include_self=False)
    w = torch.exp(s - m[rows])
    zero = torch.zeros(N, D, dtype=X.dtype, device=X.device)
    L = zero.index_add(0, rows, w).clamp(min=1e-30)
    Z = zero.index_add(0, rows, w * src) / L
    Q = zero.index_add(0, rows, w * src * src) / L
    return (X + Z) @ W, Z, Q


def _asymmetric(n=1500, per_row=6, seed=37):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row)
    pairs = np.unique(np.stack([rows, (rows + rng.integers(1, n // 2, rows.size)) % n], 1), axis=0)
    return _csr(pairs[:, 0], pairs[:, 1], n)


@pytest.mark.parametrize("kind", ["powerlaw", "planted", "molecule", "asymmetric"])
def test_genconv_matches_a_torch_layer(dev, kind):
    """forward, X.grad, weights.grad and t.grad against the same layer in torch.  The reference is that layer in fp64; the
    yardstick is the fp32 torch layer's own maximum error against it: the library layer may err by at most 4 x that plus
    1e-6 * max|ref| -- for t.grad, whose terms Q - Z^2 cancel, plus 1e-6 * sum |G| (Q + Z^2) instead."""
    _pkg_imports()
    import GNN_model
    ext = frontends.get("extension")
    directed = kind == "asymmetric"
    g = _prepare(ext, dev, *_asymmetric(), "default") if directed else _setup(ext, dev, kind, "default", sym=True)
    torch.manual_seed(35)
    conv = GNN_model.GENConv(24, 16, learn_t=True, directed=directed).to(dev)
    X = torch.randn(g["N"], 24, device=dev, requires_grad=True)
    out = conv(X, *g["args"], None)
    dY = torch.randn_like(out)
    out.backward(dY)
    rp, col = g["args"][0], g["args"][1]
    results, floor_t = {}, None
    for dtype in (torch.float64, torch.float32):
        Xr, Wr, tr = (v.detach().to(dtype).requires_grad_(True) for v in (X, conv.weights, conv.t))
        o, Z, Q = _torch_gen(Xr, Wr, tr, rp, col)
        Z.retain_grad()
        o.backward(dY.to(dtype))
        results[dtype] = (o.detach(), Xr.grad, Wr.grad, tr.grad)
        if dtype == torch.float64:
            floor_t = 1e-6 * float((Z.grad.abs() * (Q.detach() + Z.detach() ** 2)).sum())
    mine = (out.detach(), X.grad, conv.weights.grad, conv.t.grad)
    for name, m, t32, t64 in zip(("out", "X.grad", "weights.grad", "t.grad"), mine, results[torch.float32], results[torch.float64]):
        yard = float((t32.double() - t64).abs().max())
        err = float((m.double() - t64).abs().max())
        bound = 4.0 * yard + (floor_t if name == "t.grad" else 1e-6 * float(t64.abs().max()))
        print("%s %s: library error %.3e, fp32 torch error %.3e, bound %.3e" % (kind, name, err, yard, bound))
        assert err <= bound, (kind, name, err, yard, bound)


def test_refusals(fe, dev):
    _pkg_imports()
    import GNN_model
    g = _prepare(frontends.get("extension"), dev, *_asymmetric(200, 3, 36), "default")
    X = torch.randn(200, 8, device=dev)
    with pytest.raises(RuntimeError, match="symmetric"):
        GNN_model.GENConv(8, 8).to(dev)(X, *g["args"], None)
    with pytest.raises(RuntimeError, match="symmetric"):
        GNN_model.softmax_aggregate(X, g["args"])
    with pytest.raises(ValueError):
        GNN_model.GENConv(8, 8, directed=True).to(dev)(X, *g["args"], None, edge_weight=torch.ones(len(g["col"]), device=dev))
    h = _setup(fe, dev, "uniform", "default")
    Xu = torch.randn(h["N"], 8, device=dev)
    with pytest.raises(RuntimeError):
        fe.forward_softmax(Xu.cpu(), 1.0, *h["args"])
    with pytest.raises(RuntimeError):
        fe.forward_softmax(Xu.half(), 1.0, *h["args"])
    for bad in (torch.ones(3, device=dev), torch.ones(8, device=dev, dtype=torch.float64), torch.ones(8)):
        with pytest.raises(RuntimeError):
            fe.forward_softmax(Xu, bad, *h["args"])
    Z, M, L, _ = fe.forward_softmax(Xu, 1.0, *h["args"])
    with pytest.raises(RuntimeError):
        fe.softmax_backward(Z, Z, M, L, Xu, torch.ones(3, device=dev), *h["args"])
    with pytest.raises(RuntimeError):
        fe.softmax_backward(Z, Z, M, L, Xu.half(), 1.0, *h["args"])
    with pytest.raises(RuntimeError):
        fe.softmax_backward(Z.cpu(), Z, M, L, Xu, 1.0, *h["args"])


def test_hip_graph_capture(fe, dev):
    """one forward_softmax + softmax_backward pair, with a float and with a tensor beta, captured and replayed once: the eager bits"""
    g = _setup(fe, dev, "powerlaw", "default", sym=True)
    D = 32
    Xd = torch.randn(g["N"], D, device=dev)
    Gd = torch.randn(g["N"], D, device=dev)
    for beta in (1.5, torch.full((1,), 1.5, device=dev), torch.from_numpy(_beta("vector", D)).to(dev)):
        eager = fe.forward_softmax(Xd, beta, *g["args"])
        eager_dx = fe.softmax_backward(Gd, *eager[:3], Xd, beta, *g["args"])
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                out = fe.forward_softmax(Xd, beta, *g["args"])
                dx = fe.softmax_backward(Gd, *out[:3], Xd, beta, *g["args"])
        torch.cuda.current_stream().wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(tuple(out) + (dx,), tuple(eager) + (eager_dx,)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
