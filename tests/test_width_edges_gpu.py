"""The CSR-served aggregation families -- extremum, multi-aggregate, softmax, softmax gradient, edge messages -- with the
edge-message gradient and the fp32 weighted product, at the widths their own modules never run: ragged widths whose last lane
is moved back (lane_col) at every lane count L, more than one column chunk per wave (D > 256), column panels whose last panel
holds 1, 2, 4 or 6 columns, 64-column panels, and one-pass plans (panel_cols = -1) on a graph with wide tasks, split rows and
column slices, on an MI355X.

One square graph of 1203 rows (the last window has 3), every row length from 0 to 257 that changes a path, and three hubs of
513, 770 and 1100 entries whose last segments hold 1, 2 and 76 entries.  The plan forms differ in the plan only, so every
reference is computed once per (launch, D, data) and shared by all forms and both front-ends.  References and criteria are
the sibling modules' own; no tolerance is new here.  test_the_module_reaches_what_it_claims pins the table below.

  D    L   last lane moved back   column chunks     last panel: 32-column   64-column
  2    4   no  (8-byte lanes)     1
  5    4   yes                    1
  7    4   yes                    1
  33   16  yes                    1                 1
  65                                                1
  70   32  yes                    1                 6                       6
  130  64  yes                    1                 2                       2
  200                                                                       8
  260  64  no                     2                 4
  301  64  yes                    2
  520  64  no                     3
"""
import ctypes

import numpy as np
import pytest
import torch

import frontends
from test_edge_messages_gpu import _grad_f, _ints, _messages, _row_sums
from test_extremum_gpu import _prepare, _tie_features, reference
from test_multi_aggr_gpu import _check_extrema, reference_sums
from test_multi_aggr_gpu import _direct as _multi_direct
from test_softmax_aggr_gpu import _beta, _bounds, _check_bound, backward_reference, forward_reference, row_max
from test_softmax_aggr_gpu import _direct as _softmax_direct
from test_weighted_gpu import _short

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["ctypes"])
def fe(request):
    """the ctypes front-end runs everything; the extension runs test_the_extension_gives_the_ctypes_bits and the gradient"""
    return frontends.get(request.param)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


N = 1203
LENGTHS = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 64, 65, 100, 257]
HUBS = [513, 770, 1100]

# plan forms, set by build_plan parameters (never the environment)
FORMS = {
    "one_pass": dict(panel_cols=-1),
    "one_pass_slices": dict(panel_cols=-1, slice_threshold=16, n_slices=8),
    "one_pass_segments": dict(panel_cols=-1, split_threshold=9, segment_len=7),
    "one_pass_dense": dict(force=1, panel_cols=-1),
    "panel32": dict(panel_cols=32),
    "panel32_dense": dict(force=1, panel_cols=32),
    "panel64": dict(panel_cols=64),
    "plan_free": dict(plan=False),
}
ONE_PASS = [2, 5, 7, 33, 70, 130, 260, 301, 520]
PANELLED = [33, 65, 70, 130, 260]
PANEL64 = [70, 130, 200]
WIDTHS_OF = {f: PANELLED if f.startswith("panel32") else PANEL64 if f == "panel64" else ONE_PASS for f in FORMS}
# the issue's list has no width with sddmm_L = 1 or 8 at 16-byte lanes (D = 4 and 17 ... 32): 4 and 32 are added for them
GRAD_WIDTHS = [1, 2, 3, 4, 5, 8, 13, 16, 32, 33, 64, 70, 130, 256, 260, 301, 520]
EXT_FORMS = ["one_pass", "plan_free"]  # what the extension front-end runs as well, at EXT_WIDTHS
EXT_WIDTHS = [7, 130, 301]
SAFETY_FORMS = ["one_pass", "panel32", "plan_free"]
SAFETY_WIDTHS = {"one_pass": [7, 33, 130, 301], "plan_free": [7, 33, 130, 301], "panel32": [7, 33, 65, 130, 301]}
OPS = ("mul", "add_relu", "copy")
BETAS = ("2", "-3", "vector")

_GRAPH = []
_CACHE = {}
_REFS = {}  # (launch, D, data) -> operands and references, shared by every plan form and front-end


def _graph():
    if not _GRAPH:
        rng = np.random.default_rng(2101)
        lens = np.array([LENGTHS[i % len(LENGTHS)] for i in range(N - len(HUBS))] + HUBS)
        rng.shuffle(lens)
        rp = np.zeros(N + 1, np.int32)
        rp[1:] = np.cumsum(lens)
        col = np.concatenate([np.sort(rng.choice(N, n, replace=False)) for n in lens]).astype(np.int32)
        _GRAPH.append((rp, col))
    return _GRAPH[0]


def _setup(fe, dev, form):
    key = (fe.name, form)
    if key not in _CACHE:
        g = dict(_prepare(fe, dev, *_graph(), "plan_free"))  # the window products, and no plan
        p = dict(FORMS[form])
        force = p.pop("force", None)
        if p.pop("plan", True):
            rp_d, col_d, bp, e2c, e2r, ht, _, col_nzr = g["args"]
            if force is not None:
                ht = torch.full_like(ht, force)
            g["args"] = (rp_d, col_d, bp, e2c, e2r, ht, fe.build_plan(rp_d, col_d, bp, e2c, ht, **p), col_nzr)
        g["lens"] = np.diff(g["rp"])
        g["rows"] = np.repeat(np.arange(N), g["lens"])
        _CACHE[key] = g
    return _CACHE[key]


def _cached(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _np(t):
    return t.cpu().numpy()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _bits_equal(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32))


# ------------------------------------------------------------------------------------------- 0. what the module reaches
def _vec(D):
    """capi.hip pick_vec, fp32"""
    return 4 if D >= 4 else 2 if D >= 2 else 1


def _pick_L(width, vec):
    """spmm_impl.h pick_L: lanes per task"""
    slots, L = (width + vec - 1) // vec, 4
    while L < slots and L < 64:
        L <<= 1
    return L


def _sddmm_L(D, vec):
    """sddmm_impl.h sddmm_L: lanes per entry"""
    need, L = (D + vec - 1) // vec, 1
    while L < need and L < 64:
        L <<= 1
    return L


def _cell(D):
    """(L, the last lane is moved back by lane_col, column chunks per wave) of a one-pass launch"""
    vec = _vec(D)
    L = _pick_L(D, vec)
    return L, D % vec != 0, (D + L * vec - 1) // (L * vec)


def _last_panel(D, panel):
    return D - (D - 1) // panel * panel


def test_the_module_reaches_what_it_claims(fe, dev):
    """the width table of the module docstring, the plan regions each form must have, the wide thresholds and the last panels:
    dropping a width or a form from a table fails here"""
    import hcspmm
    cells = {D: _cell(D) for D in ONE_PASS}
    assert cells == {2: (4, False, 1), 5: (4, True, 1), 7: (4, True, 1), 33: (16, True, 1), 70: (32, True, 1), 130: (64, True, 1),
                     260: (64, False, 2), 301: (64, True, 2), 520: (64, False, 3)}
    assert {(4, True, 1), (16, True, 1), (32, True, 1), (64, True, 1), (64, False, 2), (64, True, 2)} <= set(cells.values())
    assert any(c[0] == 64 and c[2] == 3 for c in cells.values())
    builds = {(_vec(D), _sddmm_L(D, _vec(D))) for D in GRAD_WIDTHS}
    assert builds == {(4, L) for L in (1, 2, 4, 8, 16, 32, 64)} | {(2, 1), (2, 2), (1, 1)}  # x 3 ops: 30 of 30 kernels
    assert max(GRAD_WIDTHS) > 64 * 4  # the n_chunks > 1 loop
    assert [_last_panel(D, 32) for D in PANELLED] == [1, 1, 6, 2, 4]
    assert [_last_panel(D, 64) for D in PANEL64] == [6, 2, 8]
    assert _pick_L(32, 4) == 8 and _pick_L(64, 4) == 16  # lanes per task of the two panelled forms
    assert {33, 65, 130} <= set(SAFETY_WIDTHS["panel32"])  # the 1- and 2-column last panels are among the memory-safety cases

    rp, col = _graph()
    lens = np.diff(rp)
    assert len(col) == 49483 and (np.sort(lens)[-3:] == HUBS).all() and set(lens[lens < 513]) == set(LENGTHS)
    rows = np.repeat(np.arange(N), lens)
    assert ((np.diff(col) > 0) | (np.diff(rows) > 0)).all() and col.min() >= 0 and col.max() < N
    for form, p in FORMS.items():
        g = _setup(fe, dev, form)
        h = hcspmm.plan_header(g["args"][6])
        if not p.get("plan", True):
            assert h is None
            continue
        assert h.panel_cols == p["panel_cols"], form
        if "force" in p:  # every window a dense-tile window: no task at all, the 76 windows' rows are served from CSR
            assert h.n_dense == (N + 15) // 16 and h.n_tasks == 0 and h.n_tiny == 0, form
            continue
        assert h.n_dense == 0 and h.n_tiny > 0 and h.n_tasks - h.n_tiny > 0, form
        assert h.n_split_rows >= 3 and (h.n_split_rows == int((lens > 9).sum()) or form != "one_pass_segments"), form
        assert (h.n_slices == 8 and h.n_slice_tasks > 0) if form == "one_pass_slices" else h.n_slices == 0, form
        if form in ("one_pass", "panel32", "panel64"):  # the hubs' last segments: 1 and 2 entries are tiny tasks with a slot
            assert h.split_threshold == 512 and h.segment_len == 256 and h.n_split_rows == 3
            assert h.n_tiny == int((lens <= 2).sum()) + 2
    one_pass = _setup(fe, dev, "one_pass")["args"][6]
    for D in ONE_PASS:  # rows of 17, 31, 33 ... entries are wide tasks wherever a wave holds more than one lane group
        assert fe.wide_threshold(one_pass, D) == (16 if _cell(D)[0] < 64 else 2 ** 31 - 1), D
    assert all(fe.wide_threshold(one_pass, D) == 2 ** 31 - 1 for D in ONE_PASS if D > 128)
    assert {_cell(D)[0] for D in ONE_PASS if fe.wide_threshold(one_pass, D) == 16} == {4, 16, 32}
    for form, widths in (("panel32", PANELLED), ("panel64", PANEL64)):
        assert all(fe.wide_threshold(_setup(fe, dev, form)["args"][6], D) == 16 for D in widths), form


# ------------------------------------------------------------------------------------------- 1. max / min
def _fn(fe, reduce):
    return fe.forward_max if reduce == "max" else fe.forward_min


def _extremum_refs(D, data="special"):
    def make():
        rp, col = _graph()
        rng = np.random.default_rng(5000 + D + {"special": 0, "int": 1000, "randn": 2000}[data])
        X = rng.standard_normal((N, D)).astype(np.float32) if data == "randn" else _tie_features(rng, N, D, data == "special")
        r = dict(max=reference(rp, col, X, "max"), min=reference(rp, col, X, "min"))
        if data != "special":
            r["sum"], r["sumsq"], r["abs"], r["sq"] = reference_sums(rp, col, X)
        return X, r
    return _cached(("extremum", D, data), make)


@pytest.mark.parametrize("form", list(FORMS))
def test_forward_max_min_bits_and_arg(fe, dev, form):
    """ties, signed zeros, NaN and +-inf: values and arg are the bits of a sequential scan; return_arg=False gives the values"""
    g = _setup(fe, dev, form)
    for D in WIDTHS_OF[form]:
        X, r = _extremum_refs(D)
        Xd = torch.from_numpy(X).to(dev)
        for reduce in ("max", "min"):
            Z, arg = _fn(fe, reduce)(Xd, *g["args"])
            wz, wa = r[reduce]
            assert Z.shape == (N, D) and torch.equal(arg.cpu(), torch.from_numpy(wa)), (form, D, reduce)
            assert _bits_equal(_np(Z), wz), (form, D, reduce)
            Z1 = _fn(fe, reduce)(Xd, *g["args"], return_arg=False)
            assert len(Z1) == 1 and _bits_equal(_np(Z1[0]), wz), (form, D, reduce)


def _extremum_backward_refs(D):
    def make():
        rp, col = _graph()
        E = len(col)
        rng = np.random.default_rng(6000 + D)
        perm = rng.permutation(E).astype(np.int32)
        arg = rng.integers(0, E, (N, D)).astype(np.int32)
        half = np.sort(rng.choice(E, E // 2, replace=False))
        for e in half:  # (in entry order: a later entry of the same column overwrites an earlier one)
            arg[col[e], :] = perm[e]
        G = rng.integers(-8, 9, (N, D)).astype(np.float32)
        rows = np.repeat(np.arange(N), np.diff(rp))
        match = arg[col] == perm[:, None]
        assert match.any() and not match.all()
        want = np.zeros((N, D), np.float64)
        np.add.at(want, rows, np.where(match, G[col], 0.0))
        return perm, arg, G, (want + 0.0).astype(np.float32)
    return _cached(("extremum_backward", D), make)


@pytest.mark.parametrize("form", list(FORMS))
def test_extremum_backward_is_the_stated_function_of_its_operands(fe, dev, form):
    """grad_X[j][d] = the sum of grad_Z[i][d] over the entries e = (j, i) of row j with arg[i][d] == perm[e], for ANY perm and
    arg: this pins the launch as the function of its operands that hcspmm.h states, on a graph that need not be symmetric (a
    random permutation, random positions with planted matches), as test_softmax_aggr_gpu.test_backward_on_continuous_data
    does for its kernel.  Integer grad_Z: exact, so bit-equal to np.add.at; two calls give the same bits"""
    g = _setup(fe, dev, form)
    for D in WIDTHS_OF[form]:
        perm, arg, G, want = _extremum_backward_refs(D)
        Gd, arg_d, perm_d = (torch.from_numpy(v).to(dev) for v in (G, arg, perm))
        got = fe.forward_extremum_backward(Gd, arg_d, perm_d, *g["args"])
        assert got.shape == (N, D) and _bits_equal(_np(got), want), (form, D)
        assert _same_bits(got, fe.forward_extremum_backward(Gd, arg_d, perm_d, *g["args"])), (form, D)


# ------------------------------------------------------------------------------------------- 2. sum, sumsq, max, min
@pytest.mark.parametrize("form", list(FORMS))
def test_forward_multi_all_six_outputs_on_integer_data(fe, dev, form):
    g = _setup(fe, dev, form)
    for D in WIDTHS_OF[form]:
        X, r = _extremum_refs(D, "int")
        out = fe.forward_multi(torch.from_numpy(X).to(dev), *g["args"])
        assert len(out) == 6 and all(o.shape == (N, D) and o.is_contiguous() for o in out)
        _check_extrema(out, r, (form, D))
        assert _bits_equal(_np(out[0]), r["sum"].astype(np.float32)), (form, D, "sum")
        assert _bits_equal(_np(out[1]), r["sumsq"].astype(np.float32)), (form, D, "sumsq")


@pytest.mark.parametrize("form", list(FORMS))
def test_forward_multi_on_continuous_data(fe, dev, form):
    """randn: sum within 1e-5 * sum|x| and sumsq within 1e-5 * sum x^2 of fp64, per element; max, min and both args bit-exact
    and equal to forward_max / forward_min; two calls give the same bits"""
    g = _setup(fe, dev, form)
    for D in WIDTHS_OF[form]:
        X, r = _extremum_refs(D, "randn")
        Xd = torch.from_numpy(X).to(dev)
        out = fe.forward_multi(Xd, *g["args"])
        _check_extrema(out, r, (form, D))
        for k, name, bar in ((0, "sum", "abs"), (1, "sumsq", "sq")):
            err = np.abs(_np(out[k]).astype(np.float64) - r[name])
            assert (err <= 1e-5 * r[bar]).all(), (form, D, name, float((err / np.maximum(r[bar], 1e-300)).max()))
        for a, b in zip(out, fe.forward_multi(Xd, *g["args"])):
            assert _same_bits(a, b), (form, D)
        zx, ax = fe.forward_max(Xd, *g["args"])
        zn, an = fe.forward_min(Xd, *g["args"])
        for a, b in ((out[2], zx), (out[3], zn), (out[4], ax), (out[5], an)):
            assert _same_bits(a, b), (form, D)


# ------------------------------------------------------------------------------------------- 3. softmax aggregation
def _beta_arg(bname, b, dev):
    return torch.from_numpy(b).to(dev) if bname == "vector" else float(bname)


def _softmax_refs(D, bname):
    def make():
        rp, col = _graph()
        X = np.random.default_rng(7000 + D).standard_normal((N, D)).astype(np.float32)
        b = _beta(bname, D)
        Ms = row_max(rp, col, X, b)
        r64 = forward_reference(rp, col, X, b, np.float64, Ms)
        y32 = forward_reference(rp, col, X, b, np.float32, Ms)
        return X, b, Ms[0], r64, [_bounds(r, y, np.diff(rp)) for r, y in zip(r64, y32)]
    return _cached(("softmax", D, bname), make)


@pytest.mark.parametrize("form", list(FORMS))
def test_forward_softmax_on_continuous_data(fe, dev, form):
    """randn, beta in {2, -3, a per-column vector}: M equal to max fl32(beta x); Z, L, Q within 4 x the fp32 yardstick's error +
    1e-6 max|ref| of fp64, per row group (test_softmax_aggr_gpu._bounds)"""
    g = _setup(fe, dev, form)
    worst = {}
    for D in WIDTHS_OF[form]:
        for bname in BETAS:
            X, b, M, (Z64, L64, Q64), bounds = _softmax_refs(D, bname)
            out = fe.forward_softmax(torch.from_numpy(X).to(dev), _beta_arg(bname, b, dev), *g["args"])
            assert len(out) == 4 and all(o.shape == (N, D) and o.dtype == torch.float32 for o in out)
            tag = (form, D, bname)
            assert np.array_equal(_np(out[1]), M), tag
            for o, ref, bd, name in ((out[0], Z64, bounds[0], "Z"), (out[2], L64, bounds[1], "L"), (out[3], Q64, bounds[2], "Q")):
                _check_bound(_np(o), ref, bd, tag + (name,), worst)
    print("largest error / bound: %s" % {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("form", list(FORMS))
def test_forward_softmax_exact_cases(fe, dev, form):
    """integers in [-3, 3]: beta = +-1000 gives forward_max's / forward_min's values, everything finite; beta = 0 gives L = the
    row length and M = 0 exactly; rows of one entry give Z = x, Q = fl(x x) and L = 1 bit for bit"""
    g = _setup(fe, dev, form)
    lens = g["lens"]
    nonempty, one = lens > 0, lens == 1
    assert one.sum() == 75 and (~nonempty).sum() == 75
    x1_at = g["col"][g["rp"][:-1][one]]
    for D in WIDTHS_OF[form]:
        rng = np.random.default_rng(8000 + D)
        Xd = torch.from_numpy(rng.integers(-3, 4, (N, D)).astype(np.float32)).to(dev)
        for beta, ext in ((1000.0, fe.forward_max), (-1000.0, fe.forward_min)):
            Z, M, L, Q = (_np(o) for o in fe.forward_softmax(Xd, beta, *g["args"]))
            tag = (form, D, beta)
            assert np.array_equal(Z, _np(ext(Xd, *g["args"], return_arg=False)[0])), tag
            assert np.isfinite(Z).all() and np.isfinite(L).all() and np.isfinite(Q).all() and np.isfinite(M[nonempty]).all(), tag
            assert np.array_equal(M[nonempty], beta * Z[nonempty]) and np.array_equal(Q, Z * Z), tag
        Z, M, L, Q = (_np(o) for o in fe.forward_softmax(Xd, 0.0, *g["args"]))
        assert np.array_equal(L, np.broadcast_to(lens[:, None].astype(np.float32), L.shape)), (form, D, 0.0)
        assert (M[nonempty] == 0).all() and np.isneginf(M[~nonempty]).all(), (form, D, 0.0)
        Xr = rng.standard_normal((N, D)).astype(np.float32)  # rows of one entry, on data without zeros (a sum never holds -0)
        b = _beta("vector", D)
        Z, M, L, Q = (_np(o) for o in fe.forward_softmax(torch.from_numpy(Xr).to(dev), torch.from_numpy(b).to(dev), *g["args"]))
        x1 = Xr[x1_at]
        assert _bits_equal(Z[one], x1) and _bits_equal(Q[one], x1 * x1) and (L[one] == 1).all(), (form, D, "one entry")
        assert _bits_equal(M[one], x1 * b[None, :]), (form, D, "one entry")


def _softmax_backward_refs(D, bname):
    """test_softmax_aggr_gpu._backward_refs' synthetic operands on this graph as the walked graph: any G and Z, L >= 1, and M
    at or above every beta x of its column, so the exponent is never positive"""
    def make():
        rp, col = _graph()
        rng = np.random.default_rng(9000 + D)
        X = rng.standard_normal((N, D)).astype(np.float32)
        b = _beta(bname, D)
        G = rng.standard_normal((N, D)).astype(np.float32)
        Z = rng.standard_normal((N, D)).astype(np.float32)
        L = rng.uniform(1.0, 20.0, (N, D)).astype(np.float32)
        M = ((X * b[None, :]).max(0, keepdims=True) + rng.uniform(0.0, 0.5, (N, D))).astype(np.float32)
        r64 = backward_reference(rp, col, G, Z, M, L, X, b, np.float64)
        y32 = backward_reference(rp, col, G, Z, M, L, X, b, np.float32)
        return X, b, G, Z, M, L, r64, _bounds(r64, y32, np.diff(rp))
    return _cached(("softmax_backward", D, bname), make)


@pytest.mark.parametrize("form", list(FORMS))
def test_softmax_backward_on_continuous_data(fe, dev, form):
    """dX within the forward's bound of the fp64 formula; two calls give the same bits"""
    g = _setup(fe, dev, form)
    worst = {}
    for D in WIDTHS_OF[form]:
        for bname in BETAS:
            X, b, G, Z, M, L, r64, bounds = _softmax_backward_refs(D, bname)
            ops = [torch.from_numpy(v).to(dev) for v in (G, Z, M, L, X)]
            dX = fe.softmax_backward(*ops, _beta_arg(bname, b, dev), *g["args"])
            assert dX.shape == (N, D) and dX.dtype == torch.float32
            _check_bound(_np(dX), r64, bounds, (form, D, bname, "dX"), worst)
            assert _same_bits(dX, fe.softmax_backward(*ops, _beta_arg(bname, b, dev), *g["args"])), (form, D, bname)
    print("largest error / bound: %s" % {k: round(v, 3) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------- 4. edge-feature messages
def _edge_refs(D):
    def make():
        rp, col = _graph()
        E = len(col)
        rng = np.random.default_rng(10000 + D)
        V = E // 5
        index = dict(direct=None, perm=rng.permutation(E).astype(np.int32), many=rng.integers(0, V, E).astype(np.int32))
        X, F = _ints(rng, (N, D)), _ints(rng, (E, D))
        want = {}
        for op in OPS:
            for name, idx in index.items():
                FE = F if idx is None else F[:V][idx] if name == "many" else F[idx]
                want[op, name] = _row_sums(rp, _messages(op, X[col], FE)).astype(np.float32)
        return X, F, V, index, want
    return _cached(("edge", D), make)


@pytest.mark.parametrize("form", list(FORMS))
def test_edge_messages_integer_sums_are_exact_on_every_row(fe, dev, form):
    """integers in [-8, 8], F taken directly, through a permutation and through a many-to-one map with f_rows = E // 5: exact
    against int64 numpy on every row"""
    g = _setup(fe, dev, form)
    assert int(g["lens"].max()) * 64 < 2 ** 24  # |m| <= 64: every partial sum is an integer fp32 holds, in any order
    for D in WIDTHS_OF[form]:
        X, F, V, index, want = _edge_refs(D)
        Xd, Fd, Fs = _t(X, dev), _t(F, dev), _t(F[:V], dev)
        for op in OPS:
            xin = None if op == "copy" and D % 2 else Xd  # copy ignores X, which may be None
            for name, idx in index.items():
                idx_d = None if idx is None else torch.from_numpy(idx).to(dev)
                got = fe.forward_edge_messages(xin, Fs if name == "many" else Fd, *g["args"], op, idx_d)[0]
                assert got.shape == (N, D) and got.dtype == torch.float32
                assert torch.equal(got.cpu(), torch.from_numpy(want[op, name])), (form, D, op, name)


RECURRENCE_LEN = 256  # no longer row is compared with the recurrence (test_edge_messages_gpu's limit)


def _recurrence_refs(D):
    """the sequential fp32 recurrence of test_unsplit_rows_have_the_bits_of_the_csr_recurrence on dyadic data, one CSR position
    at a time; rows longer than RECURRENCE_LEN are left at their first RECURRENCE_LEN entries and never compared"""
    def make():
        rp, col = _graph()
        rng = np.random.default_rng(11000 + D)
        X, F = _short(rng, (N, D), 12), _short(rng, (len(col), D), 8)
        deg = np.diff(rp)
        want = {op: np.zeros((N, D), np.float32) for op in OPS}
        for k in range(RECURRENCE_LEN):
            r = np.nonzero(deg > k)[0]
            e = rp[r] + k
            t = (X[col[e]] + F[e]).astype(np.float32)
            want["mul"][r] = (want["mul"][r] + F[e] * X[col[e]]).astype(np.float32)  # products exact (8 x 12 bits): one rounding
            want["add_relu"][r] = (want["add_relu"][r] + np.where(t < 0, np.float32(0), t)).astype(np.float32)
            want["copy"][r] = (want["copy"][r] + F[e]).astype(np.float32)
        return X, F, want
    return _cached(("recurrence", D), make)


@pytest.mark.parametrize("form", [f for f in FORMS if f != "one_pass_slices"])  # the forms without column slices
def test_edge_messages_unsplit_rows_have_the_bits_of_the_csr_recurrence(fe, dev, form):
    """rows that one lane group sums -- not wide (whole-wave tree) and not split (fix-up; one_pass_segments splits above 9
    entries) -- have the bits of the sequential fp32 sum in CSR order, moved-back lanes and second chunks included"""
    import hcspmm
    g = _setup(fe, dev, form)
    planned = FORMS[form].get("plan", True)
    unsplit = hcspmm.plan_header(g["args"][6]).split_threshold if planned else RECURRENCE_LEN
    for D in [D for D in (7, 70, 301) if D in WIDTHS_OF[form]]:
        X, F, want = _recurrence_refs(D)
        thr = fe.wide_threshold(g["args"][6], D) if planned else 64
        ordered = g["lens"] <= min(thr, RECURRENCE_LEN, unsplit)
        assert ordered.sum() > 500, (form, D)
        for op in OPS:
            got = _np(fe.forward_edge_messages(_t(X, dev), _t(F, dev), *g["args"], op)[0])
            assert _bits_equal(got[ordered], want[op][ordered]), (form, D, op)


@pytest.mark.parametrize("fe_name", ["ctypes", "extension"])
def test_edge_messages_grad_every_build(fe_name, dev):
    """all 30 builds of edge_messages_grad_kernel (three ops x the ten (VEC, L) of GRAD_WIDTHS) and its n_chunks > 1 loop,
    bit-equal to the header's formulas on integer data with the kink and the dead side of add_relu in it.  The kernel takes no
    plan: once per front-end, not once per form"""
    fe = frontends.get(fe_name)
    g = _setup(fe, dev, "plan_free")
    rows, col, rp_d, col_d = g["rows"], g["col"], g["args"][0], g["args"][1]
    for D in GRAD_WIDTHS:
        def make():
            rng = np.random.default_rng(12000 + D)
            G, X, F = _ints(rng, (N, D)), _ints(rng, (N, D)), _ints(rng, (g["E"], D))
            s = X[col] + F
            assert (s == 0).any() and (s < 0).any()  # the kink and the dead side are in the data
            return G, X, F, {op: _grad_f(op, G, X, F, rows, col) for op in OPS}
        G, X, F, want = _cached(("grad", D), make)
        for op in OPS:
            got = fe.edge_messages_grad(_t(G, dev), None if op == "copy" else _t(X, dev), _t(F, dev) if op == "add_relu" else None,
                                        rp_d, col_d, op)
            assert got.shape == (g["E"], D) and want[op].dtype == np.float32
            assert _bits_equal(_np(got), want[op]), (fe_name, D, op)  # bits: the dead side is +0


# ------------------------------------------------------------------------------------------- 5. fp32 weighted product
def _weighted_operands(g, dev):
    def make():
        rng = np.random.default_rng(13000)
        a, b = rng.integers(-3, 4, N), rng.integers(-3, 4, N)
        vals = np.ldexp(np.ones(g["E"], np.float32), a[g["rows"]] + b[g["col"]]).astype(np.float32)
        return vals, np.ldexp(np.ones(N), a).astype(np.float32), np.ldexp(np.ones(N), b).astype(np.float32)
    vals, sa, sb = _cached(("weighted",), make)
    return torch.from_numpy(vals).to(dev), torch.from_numpy(sa).to(dev)[:, None], torch.from_numpy(sb).to(dev)[:, None]


@pytest.mark.parametrize("form", list(FORMS))
def test_forward_weighted_ones_and_powers_of_two(fe, dev, form):
    """checks 1 and 2 of test_weighted_gpu, fp32: values == 1 gives forward's bits; values[e] = 2^(a_row + b_col) gives the
    bits of 2^a * forward(2^b * X), so a wrong entry -> value mapping on any sub-path changes them.  (The binary product at
    these widths is pinned against the oracle by test_spmm_gpu.)"""
    g = _setup(fe, dev, form)
    ones = torch.ones(g["E"], dtype=torch.float32, device=dev)
    vals_d, sa, sb = _weighted_operands(g, dev)
    for D in WIDTHS_OF[form]:
        X = torch.from_numpy(_extremum_refs(D, "randn")[0]).to(dev)
        assert _same_bits(fe.forward_weighted(X, ones, *g["args"])[0], fe.forward(X, *g["args"])[0]), (form, D)
        want = sa * fe.forward(sb * X, *g["args"])[0]
        got = fe.forward_weighted(X, vals_d, *g["args"])[0]
        assert torch.equal(got, want), (form, D, (got - want).abs().max().item())


# ------------------------------------------------------------------------------------------- 6. both front-ends
@pytest.mark.parametrize("form", EXT_FORMS)
def test_the_extension_gives_the_ctypes_bits(dev, form):
    """every launch of this module through the torch extension, on the one-pass plan and without a plan at a ragged L = 4, a
    ragged one-chunk L = 64 and a ragged two-chunk width: the ctypes front-end's bits, which the tests above pin"""
    fc, fx = frontends.get("ctypes"), frontends.get("extension")
    gc, gx = _setup(fc, dev, form), _setup(fx, dev, form)
    assert torch.equal(gc["args"][5], gx["args"][5])  # the same window classification

    def both(call):
        a, b = call(fc, gc["args"]), call(fx, gx["args"])
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.dtype == y.dtype and _same_bits(x, y), k

    for D in EXT_WIDTHS:
        X = torch.from_numpy(_extremum_refs(D)[0]).to(dev)
        Xr = torch.from_numpy(_extremum_refs(D, "randn")[0]).to(dev)
        both(lambda f, a: f.forward_max(X, *a))
        both(lambda f, a: f.forward_min(X, *a))
        both(lambda f, a: f.forward_multi(Xr, *a))
        perm, arg, G, _ = _extremum_backward_refs(D)
        Gd, arg_d, perm_d = (torch.from_numpy(v).to(dev) for v in (G, arg, perm))
        both(lambda f, a: [f.forward_extremum_backward(Gd, arg_d, perm_d, *a)])
        bd = torch.from_numpy(_beta("vector", D)).to(dev)
        both(lambda f, a: f.forward_softmax(Xr, bd, *a))
        Xs, _, G, Z, M, L = _softmax_backward_refs(D, "vector")[:6]
        ops = [torch.from_numpy(v).to(dev) for v in (G, Z, M, L, Xs)]
        both(lambda f, a: [f.softmax_backward(*ops, bd, *a)])
        Xe, F, V, index, _ = _edge_refs(D)
        Xd, Fd, many_d = _t(Xe, dev), _t(F, dev), torch.from_numpy(index["many"]).to(dev)
        for op in OPS:
            both(lambda f, a: f.forward_edge_messages(Xd, Fd, *a, op))
            both(lambda f, a: f.forward_edge_messages(Xd, Fd[:V].contiguous(), *a, op, many_d))
        vals_d = _weighted_operands(gc, dev)[0]
        both(lambda f, a: f.forward_weighted(Xr, vals_d, *a))


# ------------------------------------------------------------------------------------------- 7. memory safety
def _forward_launches(fe, dev, D):
    """name -> call(X, F, args) -> the outputs, for every forward launch that takes strided views (forward_weighted takes a
    contiguous X: its strides are checked through the C entry point below)"""
    bd = torch.from_numpy(_beta("vector", D)).to(dev)
    calls = {
        "max": lambda X, F, a: fe.forward_max(X, *a),
        "min": lambda X, F, a: fe.forward_min(X, *a),
        "multi": lambda X, F, a: fe.forward_multi(X, *a),
        "softmax": lambda X, F, a: fe.forward_softmax(X, bd, *a),
    }
    for op in OPS:
        calls["edge_" + op] = lambda X, F, a, op=op: fe.forward_edge_messages(X, F, *a, op)
    return calls


def _in_a_nan_frame(t, left, right):
    """a view with t's values inside a wider matrix that is NaN everywhere else"""
    wide = torch.full((t.size(0), left + t.size(1) + right), float("nan"), device=t.device)
    wide[:, left:left + t.size(1)] = t
    return wide[:, left:left + t.size(1)]


@pytest.mark.parametrize("form", SAFETY_FORMS)
def test_strided_input_is_never_read_outside_the_view(fe, dev, form):
    """X (and F) as column-slice views of matrices that are NaN outside the view: the bits of the contiguous call.  A lane
    moved back too far, or a chunk that starts past the row, would read a NaN"""
    g = _setup(fe, dev, form)
    for D in SAFETY_WIDTHS[form]:
        X, F = _t(_extremum_refs(D, "int")[0], dev), _t(_edge_refs(D)[1], dev)
        Xv, Fv = _in_a_nan_frame(X, 5, 8), _in_a_nan_frame(F, 3, 4)
        assert Xv.stride(0) == D + 13 and not Xv.is_contiguous()
        for name, call in _forward_launches(fe, dev, D).items():
            want, got = call(X, F, g["args"]), call(Xv, Fv, g["args"])
            for k, (a, b) in enumerate(zip(want, got)):
                assert not torch.isnan(b.float()).any() and _same_bits(a, b), (form, D, name, k)


SENTINEL = -777.0


def _guarded(dev, D, n=1, dtype=torch.float32):
    """n sentinel-filled [N, D + 9] buffers and the pointers of their inner blocks, 5 elements in (off the 16-byte grid)"""
    bufs = [torch.full((N, D + 9), SENTINEL, dtype=dtype, device=dev) for _ in range(n)]
    return bufs, [b[:, 5:].data_ptr() for b in bufs]


def _check_guarded(bufs, full, D, tag):
    for k, (b, want) in enumerate(zip(bufs, full)):
        assert (b[:, :5] == SENTINEL).all() and (b[:, 5 + D:] == SENTINEL).all(), tag + (k, "guard columns")
        assert _same_bits(b[:, 5:5 + D], want), tag + (k,)


def _raw(g, D, src_rows, dev, ws_fn, launch):
    """one C entry point with raw output pointers: launch(lib, c) with c the _planned_call of this graph and width"""
    import hcspmm
    from hcspmm import capi
    c = hcspmm._planned_call(g["args"][:6], g["args"][6], D, src_rows, dev, ws_fn=ws_fn)
    with c:
        rc = launch(capi.lib(), c)
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", SAFETY_FORMS)
def test_guard_columns_around_every_output(dev, form):
    """every output inside a sentinel-filled buffer with ldz = D + 9, its base 5 elements in: the columns on both sides keep
    the sentinel and the inner block has the contiguous call's bits -- where the last panel holds 1 or 2 columns (D = 33, 65,
    130 on panel32) the last lane reaches back across the panel boundary and must stop at its own row.  Through ctypes only:
    the test hands raw pointers to the C entry points"""
    import hcspmm
    fe = frontends.get("ctypes")
    g = _setup(fe, dev, form)
    vp = ctypes.c_void_p
    vals_d = _weighted_operands(g, dev)[0]
    for D in SAFETY_WIDTHS[form]:
        X = _t(_extremum_refs(D, "int")[0], dev)
        ld = D + 9
        for reduce, code in (("max", 0), ("min", 1)):
            zb, zp = _guarded(dev, D)
            ab, ap = _guarded(dev, D, dtype=torch.int32)
            _raw(g, D, N, dev, hcspmm._ws_bytes_extremum, lambda lib, c: lib.hcspmm_forward_extremum(
                vp(X.data_ptr()), N, D, vp(zp[0]), ld, 0, *c.graph, *c.ws, code, vp(ap[0]), ld))
            _check_guarded(zb + ab, _fn(fe, reduce)(X, *g["args"]), D, (form, D, reduce))
        zb, zp = _guarded(dev, D, 4)
        ab, ap = _guarded(dev, D, 2, torch.int32)
        _multi_direct(g, X, D, zp, ld, ap, ld)
        _check_guarded(zb + ab, fe.forward_multi(X, *g["args"]), D, (form, D, "multi"))
        bd = torch.from_numpy(_beta("vector", D)).to(dev)
        zb, zp = _guarded(dev, D, 4)
        _softmax_direct(g, X, bd, D, zp, ld)
        _check_guarded(zb, fe.forward_softmax(X, bd, *g["args"]), D, (form, D, "softmax"))
        F = _t(_edge_refs(D)[1], dev)
        for op in OPS:
            zb, zp = _guarded(dev, D)
            _raw(g, D, N, dev, hcspmm._ws_bytes, lambda lib, c: lib.hcspmm_forward_edge_messages(
                vp(X.data_ptr()), N, D, vp(F.data_ptr()), g["E"], D, None, hcspmm.EDGE_OPS[op], vp(zp[0]), ld, *c.graph, *c.ws))
            _check_guarded(zb, fe.forward_edge_messages(X, F, *g["args"], op), D, (form, D, op))
        Xv = _in_a_nan_frame(X, 5, 8)  # forward_weighted: strided X and Z in one call
        zb, zp = _guarded(dev, D)
        _raw(g, D, N, dev, hcspmm._ws_bytes, lambda lib, c: lib.hcspmm_forward_weighted(
            vp(Xv.data_ptr()), N, Xv.stride(0), vp(zp[0]), ld, 0, *c.graph, *c.ws, vp(vals_d.data_ptr())))
        _check_guarded(zb, fe.forward_weighted(X, vals_d, *g["args"]), D, (form, D, "weighted"))
