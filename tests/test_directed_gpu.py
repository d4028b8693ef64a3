"""Directed graphs on an MI355X: the indexed-values SpMM (hcspmm_forward_weighted_indexed), the backward entry points that
take the transposed graph, and the functions, layers and driver built on them (directed=True).

Contracts (include/hcspmm.h):
  * forward_weighted_indexed(X, V, idx) is bit for bit forward_weighted_heads(X, V[:, idx]) -- forward_weighted for one head --
    on every plan form of test_heads_gpu.py and across the size gates of test_scale_paths_gpu.py;
  * on a pattern-symmetric graph the _directed backwards called with (row_pointers, column_index, perm) as the transposed
    graph return the bits of the entry points they generalise;
  * on asymmetric graphs every directed operator and layer matches a float64 torch reference built from the edge list within
    |got - want| <= 1e-4 * max|want| (the _close of the sibling files), forward and every gradient, while the gradient taken
    through A instead of A^T misses that bar: the tests can tell the two apart.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import frontends
import hcspmm
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


def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


# ------------------------------------------------------------------------------------------- the indexed SpMM
def _graph(kind):  # test_heads_gpu._graph
    if kind == "powerlaw":  # hubs: wide tasks, split rows
        return graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    if kind == "planted":  # dense-tile windows of every record kind
        return graphs.planted_dense_graph(2400, seed=4)
    if kind == "community":
        return graphs.community_graph(2500, 20000, seed=5)[:2]
    if kind == "molecule":  # short rows: tiny tasks
        return graphs.molecule_graph(3000, seed=6)
    return graphs.uniform_graph(2000, 16000, seed=7)


PLANS = {  # test_heads_gpu.PLANS
    "default": {},
    "slices": dict(slice_threshold=16, n_slices=8),
    "sparse": dict(force=0),
    "dense": dict(force=1),
    "tiny_segments": dict(split_threshold=9, segment_len=7),
    "panel32": dict(panel_cols=32),
    "plan_free": dict(plan=False),
}
KINDS = ["powerlaw", "planted", "community", "molecule", "uniform"]
# of test_heads_gpu.SHAPES: every heads in {1, 2, 3, 4, 8} and every Dh in {4, 8, 16, 32, 64}, D from 4 to 256
SHAPES = [(1, 4), (1, 64), (2, 8), (3, 16), (4, 32), (8, 8), (2, 64), (4, 4), (8, 32), (3, 4)]
assert {h for h, _ in SHAPES} == {1, 2, 3, 4, 8} and {d for _, d in SHAPES} == {4, 8, 16, 32, 64}

_CACHE = {}


def _setup(fe, dev, kind, form):  # test_heads_gpu._setup
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


def _indices(E, gen, dev):
    """(name, int32 index [E], number of values): a random permutation, the identity, a many-to-one index"""
    few = max(E // 3, 1)
    return [("permutation", torch.randperm(E, generator=gen).to(torch.int32).to(dev), E),
            ("identity", torch.arange(E, dtype=torch.int32, device=dev), E),
            ("many_to_one", torch.randint(0, few, (E,), generator=gen).to(torch.int32).to(dev), few)]


@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_indexed_values_are_the_gathered_values(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    gen = torch.Generator(device="cpu").manual_seed(41)
    for name, idx, V in _indices(g["E"], gen, dev):
        for heads, dh in SHAPES:
            D = heads * dh
            X = torch.randn(g["N"], D, generator=gen).to(dev)
            vals = torch.randn(heads, V, generator=gen).to(dev)
            got = fe.forward_weighted_indexed(X, vals, idx, *g["args"])[0]
            gathered = vals[:, idx.long()].contiguous()
            want = fe.forward_weighted_heads(X, gathered, *g["args"])[0]
            assert got.shape == (g["N"], D)
            assert torch.equal(got, want), (kind, form, name, heads, dh)
            if heads == 1:
                assert torch.equal(got, fe.forward_weighted(X, gathered[0].contiguous(), *g["args"])[0]), (kind, form, name, dh)
                assert torch.equal(got, fe.forward_weighted_indexed(X, vals[0].contiguous(), idx, *g["args"])[0])  # 1-D values


@pytest.mark.parametrize("form", ["default", "tiny_segments", "dense", "plan_free"])
@pytest.mark.parametrize("kind", ["powerlaw", "planted", "molecule"])
def test_one_head_takes_every_width_of_the_weighted_product(fe, dev, kind, form):
    """heads = 1: the widths forward_weighted serves that the multi-head form does not (D % 4 != 0; 8- and 4-byte lanes)"""
    g = _setup(fe, dev, kind, form)
    gen = torch.Generator(device="cpu").manual_seed(42)
    for name, idx, V in _indices(g["E"], gen, dev):
        for D in (1, 2, 3, 6, 22, 33, 70, 130):
            X = torch.randn(g["N"], D, generator=gen).to(dev)
            vals = torch.randn(V, generator=gen).to(dev)
            got = fe.forward_weighted_indexed(X, vals, idx, *g["args"])[0]
            want = fe.forward_weighted(X, vals[idx.long()].contiguous(), *g["args"])[0]
            assert torch.equal(got, want), (kind, form, name, D)


def _short_rows(N, seed=9):  # test_scale_paths_gpu._short_rows
    rng = np.random.default_rng(seed)
    deg = rng.choice([0, 1, 2, 3, 7, 40], size=N, p=[0.35, 0.3, 0.2, 0.1, 0.04, 0.01])
    hubs = {5: 513, N // 2 + 1700: 514, N - 1: 770}
    for r, d in hubs.items():
        deg[r] = d
    rows = np.repeat(np.arange(N, dtype=np.int64), deg)
    cols = rng.integers(0, N, rows.shape[0])
    start = np.concatenate([[0], np.cumsum(deg)])
    for r, d in hubs.items():
        c = rng.choice(N - 1, d, replace=False)
        cols[start[r]:start[r] + d] = c + (c >= r)
    return rows, cols


def test_indexed_values_across_the_size_gates(fe, dev):
    """test_scale_paths_gpu.py's generators at their sizes, shipped defaults: the short-row graph takes the tiny tasks' own
    launch and has segmented rows, the power-law graph gets automatic column slices and segmented rows"""
    for k in ("HCSPMM_TINY_KERNEL_MIN_TASKS", "HCSPMM_PANEL_COLS", "HCSPMM_SLICE_THRESHOLD", "HCSPMM_SLICES"):
        assert k not in os.environ, "unset %s: the shipped launch decisions are the subject" % k
    gen = torch.Generator(device="cpu").manual_seed(43)
    crossed = set()
    for kind in ("short_rows", "power_law"):
        if kind == "short_rows":
            rows, cols = _short_rows(700000)
            rp, col = graphs._to_csr(rows, cols, 700000)
        else:
            rp, col = graphs.powerlaw_graph(300000, 6000000, seed=3, max_degree_frac=0.02)
        N, E = len(rp) - 1, len(col)
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        args = (rp_d, col_d) + tuple(fe.preprocess(col_d, rp_d, N, E, (N + 15) // 16, rule=3))
        h = hcspmm.plan_header(args[6])
        if hcspmm.own_tiny_launch(args[6]):
            crossed.add("tiny_launch")
        if h.n_slices > 0 and h.n_slice_tasks > 0:
            crossed.add("column_slices")
        if h.n_split_rows > 0:
            crossed.add("segments")
        if kind == "short_rows":
            assert hcspmm.own_tiny_launch(args[6]) is True and h.n_split_rows == 3
        else:
            assert h.n_slices > 0 and h.n_slice_tasks > 0 and h.n_split_rows > 0
        idx = torch.randperm(E, generator=gen).to(torch.int32).to(dev)
        for heads, dh in ((4, 8), (1, 64), (8, 16)):
            X = torch.randn(N, heads * dh, generator=gen).to(dev)
            vals = torch.randn(heads, E, generator=gen).to(dev)
            got = fe.forward_weighted_indexed(X, vals, idx, *args)[0]
            want = fe.forward_weighted_heads(X, vals[:, idx.long()].contiguous(), *args)[0]
            assert torch.equal(got, want), (kind, heads, dh)
            del X, vals, got, want
        del args, rp_d, col_d, idx
        torch.cuda.empty_cache()
    assert crossed == {"tiny_launch", "column_slices", "segments"}


def test_indexed_operands_are_checked(fe, dev):
    g = _setup(fe, dev, "uniform", "default")
    N, E = g["N"], g["E"]
    X = torch.randn(N, 24, device=dev)
    idx = torch.arange(E, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        fe.forward_weighted_indexed(X, torch.rand(4, E, device=dev), idx, *g["args"])  # Dh = 6
    with pytest.raises(RuntimeError, match="float32"):
        fe.forward_weighted_indexed(X.half(), torch.rand(2, E, device=dev), idx, *g["args"])
    with pytest.raises(RuntimeError, match="value_index"):
        fe.forward_weighted_indexed(X, torch.rand(2, E, device=dev), idx.long(), *g["args"])
    with pytest.raises(RuntimeError, match="value_index"):
        fe.forward_weighted_indexed(X, torch.rand(2, E, device=dev), idx[:-1].contiguous(), *g["args"])


# ------------------------------------------------------------------------------------------- symmetric identity
def _symmetric_setup(fe, dev):
    """a pattern-symmetric graph with rows beyond 2048 entries (every row class of the attention kernels)"""
    key = (fe.name, "symmetric_hubs")
    if key not in _CACHE:
        rp, col = graphs.powerlaw_graph(6000, 120000, seed=11, max_degree_frac=0.9)
        assert np.diff(rp).max() > 2048
        N, E = len(rp) - 1, len(col)
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        args = (rp_d, col_d) + tuple(fe.preprocess(col_d, rp_d, N, E, (N + 15) // 16, rule=3))
        perm = fe.transpose_permutation(rp_d, col_d)
        rp_t, col_t, eid_t = fe.transpose_graph(rp_d, col_d)
        assert all(t.dtype == torch.int32 and t.device == rp_d.device for t in (rp_t, col_t, eid_t))
        assert torch.equal(rp_t, rp_d) and torch.equal(col_t, col_d) and torch.equal(eid_t.long(), perm)
        _CACHE[key] = dict(N=N, E=E, args=args, perm=perm, perm32=perm.to(torch.int32))
    return _CACHE[key]


@pytest.mark.parametrize("heads", [1, 2, 3, 4, 8])
def test_gat_backward_directed_is_the_symmetric_backward(fe, dev, heads):
    g = _symmetric_setup(fe, dev)
    rp_d, col_d = g["args"][:2]
    gen = torch.Generator(device="cpu").manual_seed(44 + heads)
    s_dst, s_src = (torch.randn(g["N"], heads, generator=gen).to(dev) for _ in range(2))
    alpha = fe.gat_attention(s_dst, s_src, rp_d, col_d, 0.2)
    ga = torch.randn(heads, g["E"], generator=gen).to(dev)
    want = fe.gat_attention_backward(alpha, ga, s_dst, s_src, rp_d, col_d, g["perm"], 0.2)
    got = fe.gat_attention_backward_directed(alpha, ga, s_dst, s_src, rp_d, col_d, rp_d, g["perm32"], 0.2)
    again = fe.gat_attention_backward_directed(alpha, ga, s_dst, s_src, rp_d, col_d, rp_d, g["perm32"], 0.2)
    for a, b, c in zip(got, want, again):
        assert torch.equal(a, b) and torch.equal(a, c), heads


@pytest.mark.parametrize("heads,dh", [(1, 16), (4, 8), (2, 64), (8, 4), (3, 32)])
def test_gatv2_backward_directed_is_the_symmetric_backward(fe, dev, heads, dh):
    g = _symmetric_setup(fe, dev)
    rp_d, col_d = g["args"][:2]
    D = heads * dh
    gen = torch.Generator(device="cpu").manual_seed(45 + D)
    H = torch.randn(g["N"], 2 * D, generator=gen).to(dev)
    H_src, H_dst = H[:, :D], H[:, D:]  # views: the halves of one projection
    att = torch.randn(heads, dh, generator=gen).to(dev)
    gl = torch.randn(heads, g["E"], generator=gen).to(dev)
    want = fe.gatv2_scores_backward(gl, H_dst, H_src, att, rp_d, col_d, g["perm"], 0.2)
    got = fe.gatv2_scores_backward_directed(gl, H_dst, H_src, att, rp_d, col_d, rp_d, col_d, g["perm32"], 0.2)
    again = fe.gatv2_scores_backward_directed(gl, H_dst, H_src, att, rp_d, col_d, rp_d, col_d, g["perm32"], 0.2)
    for a, b, c in zip(got, want, again):
        assert torch.equal(a, b) and torch.equal(a, c), (heads, dh)


@pytest.mark.parametrize("reduce", ["max", "min"])
def test_extremum_backward_on_the_graph_itself_is_todays_call(fe, dev, reduce):
    """A^T = A on a symmetric pattern: the backward on transposed_graph's tensors (A's own plan, entry_index_t = perm) is
    the backward the symmetric path has always made"""
    g = _symmetric_setup(fe, dev)
    rp_d, col_d = g["args"][:2]
    gen = torch.Generator(device="cpu").manual_seed(46)
    X = torch.randn(g["N"], 32, generator=gen).to(dev)
    dY = torch.randn(g["N"], 32, generator=gen).to(dev)
    Z, arg = (fe.forward_max if reduce == "max" else fe.forward_min)(X, *g["args"], True)
    want = fe.forward_extremum_backward(dY, arg, g["perm32"], *g["args"])
    rp_t, col_t, eid_t = fe.transpose_graph(rp_d, col_d)
    args_t = (rp_t, col_t) + tuple(fe.preprocess(col_t, rp_t, g["N"], g["E"], (g["N"] + 15) // 16, rule=3))
    got = fe.forward_extremum_backward(dY, arg, eid_t, *args_t)
    assert torch.equal(got, want)
    assert torch.equal(got, fe.forward_extremum_backward(dY, arg, eid_t, *args_t))


# ------------------------------------------------------------------------------------------- directed, against fp64
def _asymmetric(kind):
    if kind == "uniform":
        return graphs.uniform_graph(500, 3000, seed=6)
    if kind == "powerlaw":
        return graphs.powerlaw_graph(3000, 40000, seed=3, symmetric=False)
    if kind == "powerlaw_hubs":
        return graphs.powerlaw_graph(3000, 60000, seed=4, symmetric=False, max_degree_frac=0.9)
    if kind == "planted":
        return graphs.planted_dense_graph(1200, seed=8)
    rp, col = graphs.powerlaw_graph(20000, 400000, seed=5, symmetric=False, max_degree_frac=0.9)
    assert np.bincount(col).max() > 2048  # a row of A^T beyond 2048 entries: the workgroup-per-row class
    return rp, col


DIRECTED = ["uniform", "powerlaw", "powerlaw_hubs", "planted", "in_degree_hubs"]


def _directed_setup(dev, kind):
    key = ("directed", kind)
    if key not in _CACHE:
        _pkg_imports()
        import HCSPMM
        rp, col = _asymmetric(kind)
        N, E = len(rp) - 1, len(col)
        rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(rp))
        assert not np.array_equal(np.sort(rows * N + col), np.sort(col.astype(np.int64) * N + rows)), "symmetric pattern"
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        args = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16))
        _CACHE[key] = dict(N=N, E=E, args=args, rows=torch.from_numpy(rows), cols=torch.from_numpy(col).long())
    return _CACHE[key]


def _close(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return bool(((got - want).abs() <= 1e-4 * want.abs().max()).all())


def _segment_softmax64(x, rows, N):
    idx = rows.expand_as(x)
    m = torch.full((x.size(0), N), -float("inf"), dtype=x.dtype).scatter_reduce(1, idx, x, "amax")
    ex = torch.exp(x - m.gather(1, idx))
    s = torch.zeros((x.size(0), N), dtype=x.dtype).scatter_add(1, idx, ex)
    return ex / s.gather(1, idx)


class _Gathers:
    """X[cols] of the float64 references, kept with their gradients: scattering a gathered tensor's gradient back by column
    is the gradient through A^T (what autograd does), scattering it by row is the gradient through A -- what the
    directed=False machinery would compute on these graphs"""

    def __init__(self, g):
        self.g, self.kept = g, []

    def __call__(self, leaf):
        t = leaf.index_select(0, self.g["cols"])
        t.retain_grad()
        self.kept.append((leaf, t))
        return t

    def through_a(self, leaf):
        """the gradient of `leaf` with its gathered part sent along A instead of A^T"""
        t = next(t for lf, t in self.kept if lf is leaf)
        right = torch.zeros_like(leaf).index_add(0, self.g["cols"], t.grad)
        wrong = torch.zeros_like(leaf).index_add(0, self.g["rows"], t.grad)
        return leaf.grad - right + wrong


def _leaf64(t):
    return t.detach().cpu().double().requires_grad_(True)


def _run_twice(fn, leaves):
    """fn() -> output; backward with a fixed cotangent, twice: (output, gradients), asserting the two runs give the same bits"""
    runs = []
    for _ in range(2):
        for t in leaves:
            t.grad = None
        out = fn()
        if not runs:
            cot = torch.randn(out.shape, generator=torch.Generator(device="cpu").manual_seed(7)).to(out.device)
        (out * cot).sum().backward()
        runs.append((out.detach().clone(), [t.grad.clone() for t in leaves]))
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b), "two directed backward passes differ"
    return runs[0][0], runs[0][1], cot


def _compare(kind, what, out, grads, out64, leaves64, wrong):
    """forward and every gradient at the bar; `wrong`: {leaf position: its gradient through A}, which must miss it"""
    assert _close(out, out64), (kind, what, "forward")
    for i, (got, leaf) in enumerate(zip(grads, leaves64)):
        assert _close(got, leaf.grad), (kind, what, "gradient %d" % i)
    assert wrong
    for i, w in wrong.items():
        assert not _close(grads[i], w), (kind, what, "gradient %d does not tell A^T from A" % i)


@pytest.mark.parametrize("kind", DIRECTED)
def test_directed_edge_weighted_aggregate(dev, kind):
    g = _directed_setup(dev, kind)
    import GNN_model
    gen = torch.Generator(device="cpu").manual_seed(51)
    for D in (32, 6):
        X = torch.randn(g["N"], D, generator=gen).to(dev).requires_grad_(True)
        w = torch.rand(g["E"], generator=gen).to(dev).requires_grad_(True)
        out, grads, cot = _run_twice(lambda: GNN_model.edge_weighted_aggregate(X, w, g["args"], directed=True), [X, w])
        X64, w64 = _leaf64(X), _leaf64(w)
        gather = _Gathers(g)
        out64 = torch.zeros(g["N"], D, dtype=torch.float64).index_add(0, g["rows"], w64[:, None] * gather(X64))
        (out64 * cot.cpu().double()).sum().backward()
        _compare(kind, "edge_weighted_aggregate D=%d" % D, out, grads, out64, [X64, w64], {0: gather.through_a(X64)})
    # the values-without-gradient form the normalised GCN / GIN layers use
    X = torch.randn(g["N"], 16, generator=gen).to(dev).requires_grad_(True)
    w = torch.rand(g["E"], generator=gen).to(dev)
    out, grads, cot = _run_twice(lambda: GNN_model.weighted_aggregate(X, w, g["args"], directed=True), [X])
    X64 = _leaf64(X)
    gather = _Gathers(g)
    out64 = torch.zeros(g["N"], 16, dtype=torch.float64).index_add(0, g["rows"], w.cpu().double()[:, None] * gather(X64))
    (out64 * cot.cpu().double()).sum().backward()
    _compare(kind, "weighted_aggregate", out, grads, out64, [X64], {0: gather.through_a(X64)})


@pytest.mark.parametrize("kind", DIRECTED)
def test_directed_edge_weighted_aggregate_heads(dev, kind):
    g = _directed_setup(dev, kind)
    import GNN_model
    gen = torch.Generator(device="cpu").manual_seed(52)
    for heads, dh in ((4, 8), (2, 32), (3, 4)):
        X = torch.randn(g["N"], heads * dh, generator=gen).to(dev).requires_grad_(True)
        w = torch.rand(heads, g["E"], generator=gen).to(dev).requires_grad_(True)
        out, grads, cot = _run_twice(lambda: GNN_model.edge_weighted_aggregate_heads(X, w, g["args"], directed=True), [X, w])
        X64, w64 = _leaf64(X), _leaf64(w)
        gather = _Gathers(g)
        msg = w64.t()[:, :, None] * gather(X64).reshape(-1, heads, dh)
        out64 = torch.zeros(g["N"], heads, dh, dtype=torch.float64).index_add(0, g["rows"], msg).reshape(g["N"], heads * dh)
        (out64 * cot.cpu().double()).sum().backward()
        _compare(kind, "heads %dx%d" % (heads, dh), out, grads, out64, [X64, w64], {0: gather.through_a(X64)})


@pytest.mark.parametrize("kind", DIRECTED)
def test_directed_gat_attention(dev, kind):
    g = _directed_setup(dev, kind)
    import GNN_model
    gen = torch.Generator(device="cpu").manual_seed(53)
    for heads in (1, 4, 3):
        s_dst, s_src = (torch.randn(g["N"], heads, generator=gen).to(dev).requires_grad_(True) for _ in range(2))
        out, grads, cot = _run_twice(lambda: GNN_model.gat_attention(s_dst, s_src, g["args"], 0.2, directed=True), [s_dst, s_src])
        d64, s64 = _leaf64(s_dst), _leaf64(s_src)
        gather = _Gathers(g)
        logits = torch.nn.functional.leaky_relu(d64.index_select(0, g["rows"]) + gather(s64), 0.2).t()  # [heads, E]
        out64 = _segment_softmax64(logits, g["rows"], g["N"])
        (out64 * cot.cpu().double()).sum().backward()
        _compare(kind, "gat_attention heads=%d" % heads, out, grads, out64, [d64, s64], {1: gather.through_a(s64)})


@pytest.mark.parametrize("kind", DIRECTED)
def test_directed_gatv2_attention(dev, kind):
    g = _directed_setup(dev, kind)
    import GNN_model
    gen = torch.Generator(device="cpu").manual_seed(54)
    for heads, dh in ((1, 16), (4, 8), (2, 32)):
        D = heads * dh
        H_dst, H_src = (torch.randn(g["N"], D, generator=gen).to(dev).requires_grad_(True) for _ in range(2))
        att = torch.randn(heads, dh, generator=gen).to(dev).requires_grad_(True)
        out, grads, cot = _run_twice(lambda: GNN_model.gatv2_attention(H_dst, H_src, att, g["args"], 0.2, directed=True),
                                     [H_dst, H_src, att])
        d64, s64, a64 = _leaf64(H_dst), _leaf64(H_src), _leaf64(att)
        gather = _Gathers(g)
        e = torch.nn.functional.leaky_relu(d64.index_select(0, g["rows"]) + gather(s64), 0.2)
        logits = (e.reshape(-1, heads, dh) * a64[None]).sum(2).t()
        out64 = _segment_softmax64(logits, g["rows"], g["N"])
        (out64 * cot.cpu().double()).sum().backward()
        _compare(kind, "gatv2_attention %dx%d" % (heads, dh), out, grads, out64, [d64, s64, a64], {1: gather.through_a(s64)})


@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("kind", DIRECTED)
def test_directed_extremum_aggregate(dev, kind, reduce):
    g = _directed_setup(dev, kind)
    import GNN_model
    gen = torch.Generator(device="cpu").manual_seed(55)
    for D in (32, 6):
        X = torch.randn(g["N"], D, generator=gen).to(dev).requires_grad_(True)  # continuous data: no ties
        out, grads, cot = _run_twice(lambda: GNN_model.extremum_aggregate(X, g["args"], reduce, directed=True), [X])
        X64 = _leaf64(X)
        gather = _Gathers(g)
        src = gather(X64)
        out64 = torch.zeros(g["N"], D, dtype=torch.float64).scatter_reduce(
            0, g["rows"][:, None].expand_as(src), src, "amax" if reduce == "max" else "amin", include_self=False)
        (out64 * cot.cpu().double()).sum().backward()
        _compare(kind, "extremum %s D=%d" % (reduce, D), out, grads, out64, [X64], {0: gather.through_a(X64)})


def test_directed_false_still_refuses_these_graphs(dev):
    g = _directed_setup(dev, "uniform")
    import GNN_model
    X = torch.randn(g["N"], 8, device=dev, requires_grad=True)
    w = torch.rand(g["E"], device=dev)
    for call in (lambda: GNN_model.weighted_aggregate(X, w, g["args"]),
                 lambda: GNN_model.edge_weighted_aggregate(X, w, g["args"]),
                 lambda: GNN_model.edge_weighted_aggregate_heads(X, w.expand(2, -1).contiguous(), g["args"]),
                 lambda: GNN_model.gat_attention(X[:, :2], X[:, 2:4], g["args"]),
                 lambda: GNN_model.gatv2_attention(X, X, torch.rand(2, 4, device=dev), g["args"]),
                 lambda: GNN_model.extremum_aggregate(X, g["args"]),
                 lambda: GNN_model.GATConv(8, 8)(X, *g["args"]),
                 lambda: GNN_model.GATv2Conv(8, 8).to(dev)(X, *g["args"]),
                 lambda: GNN_model.SAGEConv(8, 8).to(dev)(X, *g["args"])):
        with pytest.raises(RuntimeError, match="symmetric"):
            call()


def test_transposed_graph_is_cached_and_has_its_own_plan(dev):
    g = _directed_setup(dev, "powerlaw_hubs")
    import GNN_model
    gt = GNN_model.transposed_graph(g["args"])
    assert GNN_model.transposed_graph(g["args"]) is gt and len(gt) == 9
    h, h_t = hcspmm.plan_header(g["args"][6]), hcspmm.plan_header(gt[6])
    assert (h_t.num_nodes, h_t.num_edges) == (h.num_nodes, h.num_edges) == (g["N"], g["E"])
    A = torch.zeros(g["N"], g["N"])
    A[g["rows"], g["cols"]] = torch.arange(1, g["E"] + 1, dtype=torch.float32)
    rows_t = torch.repeat_interleave(torch.arange(g["N"]), (gt[0][1:] - gt[0][:-1]).cpu().long())
    assert torch.equal(A.t()[rows_t, gt[1].cpu().long()], (gt[8].cpu() + 1).float())  # entry_index_t names A's entries


# ------------------------------------------------------------------------------------------- layers
def _layer_check(dev, conv, ref64, params, din=24):
    g = _directed_setup(dev, "powerlaw")
    X = torch.randn(g["N"], din, device=dev, requires_grad=True)
    leaves = [X] + list(params)
    out, grads, cot = _run_twice(lambda: conv(X, *g["args"], None), leaves)
    leaves64 = [_leaf64(t) for t in leaves]
    out64 = ref64(*leaves64, g["rows"], g["cols"], g["N"])
    (out64 * cot.cpu().double()).sum().backward()
    assert _close(out, out64)
    for i, (got, leaf) in enumerate(zip(grads, leaves64)):
        assert _close(got, leaf.grad), i
    return out


def _torch_gat64(X, W, a_src, a_dst, rows, cols, N, slope, concat):
    outs = []
    for k in range(W.size(0)):
        h = X @ W[k]
        logit = torch.nn.functional.leaky_relu((h @ a_dst[k])[rows] + (h @ a_src[k])[cols], slope)
        alpha = _segment_softmax64(logit[None], rows, N)[0]
        outs.append(torch.zeros(N, h.size(1), dtype=h.dtype).index_add(0, rows, alpha[:, None] * h[cols]))
    return torch.cat(outs, 1) if concat else torch.stack(outs).mean(0)


@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("heads", [1, 4])
def test_directed_gat_layer(dev, heads, concat):
    _pkg_imports()
    import GNN_model
    torch.manual_seed(61 + heads + 10 * concat)
    conv = GNN_model.GATConv(24, 16, 0, heads=heads, concat=concat, directed=True).to(dev)
    out = _layer_check(dev, conv, lambda X, W, a_s, a_d, r, c, N: _torch_gat64(X, W, a_s, a_d, r, c, N, conv.negative_slope, concat),
                       (conv.weights, conv.a_src, conv.a_dst))
    assert out.shape[1] == (heads * 16 if concat else 16)


def _torch_gatv2_64(X, W, att, rows, cols, N, slope, concat, share):  # test_gatv2_gpu._torch_gatv2_64
    heads, dout = att.shape
    width = heads * dout
    h = X @ W
    h_src = h[:, :width]
    h_dst = h_src if share else h[:, width:]
    e = torch.nn.functional.leaky_relu(h_dst.index_select(0, rows) + h_src.index_select(0, cols), slope)
    logits = (e.reshape(-1, heads, dout) * att[None]).sum(2).t()
    alpha = _segment_softmax64(logits, rows, N)
    msg = alpha.t()[:, :, None] * h_src.index_select(0, cols).reshape(-1, heads, dout)
    out = torch.zeros(N, heads, dout, dtype=h.dtype).index_add(0, rows, msg)
    return out.reshape(N, width) if concat else out.mean(1)


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("heads", [1, 4])
def test_directed_gatv2_layer(dev, heads, concat, share):
    _pkg_imports()
    import GNN_model
    torch.manual_seed(62 + heads + 2 * concat + 4 * share)
    conv = GNN_model.GATv2Conv(24, 16, 0, heads=heads, concat=concat, share_weights=share, directed=True).to(dev)
    _layer_check(dev, conv, lambda X, W, att, r, c, N: _torch_gatv2_64(X, W, att, r, c, N, conv.negative_slope, concat, share),
                 (conv.weights, conv.att))


@pytest.mark.parametrize("aggr", ["max", "min", "mean"])
def test_directed_sage_layer(dev, aggr):
    _pkg_imports()
    import GNN_model
    torch.manual_seed(63)
    conv = GNN_model.SAGEConv(24, 16, aggr=aggr, directed=True).to(dev)

    def ref(X, W_root, W_neigh, rows, cols, N):
        src = X.index_select(0, cols)
        if aggr == "mean":
            deg = torch.bincount(rows, minlength=N).double()
            agg = torch.zeros(N, X.size(1), dtype=X.dtype).index_add(0, rows, src / deg[rows][:, None])
        else:
            agg = torch.zeros(N, X.size(1), dtype=X.dtype).scatter_reduce(
                0, rows[:, None].expand_as(src), src, "amax" if aggr == "max" else "amin", include_self=False)
        return X @ W_root + agg @ W_neigh

    _layer_check(dev, conv, ref, (conv.weights_root, conv.weights_neigh))


def test_directed_normalised_gcn_and_gin_layers(dev):
    """_Conv with edge_weight: the weighted path runs on the transposed graph; the binary layer functions are untouched"""
    _pkg_imports()
    import GNN_model
    import HCSPMM
    g = _directed_setup(dev, "powerlaw")
    w = HCSPMM.edge_norm(g["args"][0], g["args"][1], "mean")
    for cls, first in ((GNN_model.GCNConv, False), (GNN_model.GINConv, True)):
        torch.manual_seed(64)
        conv = cls(24, 16, 0, directed=True).to(dev)
        X = torch.randn(g["N"], 24, device=dev, requires_grad=True)
        out, grads, cot = _run_twice(lambda: conv(X, *g["args"], None, edge_weight=w), [X, conv.weights])
        X64, W64, w64 = _leaf64(X), _leaf64(conv.weights), w.cpu().double()

        def agg(T):
            return torch.zeros(g["N"], T.size(1), dtype=torch.float64).index_add(0, g["rows"], w64[:, None] * T[g["cols"]])

        out64 = agg(X64) @ W64 if first else agg(X64 @ W64)
        (out64 * cot.cpu().double()).sum().backward()
        assert _close(out, out64) and _close(grads[0], X64.grad) and _close(grads[1], W64.grad), cls.__name__
        with pytest.raises(RuntimeError, match="symmetric"):
            cls(24, 16, 0).to(dev)(X, *g["args"], None, edge_weight=w)


# ------------------------------------------------------------------------------------------- driver
def test_driver_trains_gatv2_on_a_directed_graph(capsys, monkeypatch, tmp_path):
    _pkg_imports()
    rp, col = graphs.powerlaw_graph(600, 6000, seed=9, symmetric=False)
    os.makedirs(tmp_path / "Dataset")
    graphs.write_coo_text(str(tmp_path / "Dataset" / "directed.txt"), rp, col)
    monkeypatch.chdir(tmp_path)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_directed", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = []
    nll = mod.nll_loss

    def recording(log_probs, target):
        loss = nll(log_probs, target)
        losses.append(float(loss.detach()))
        return loss

    monkeypatch.setattr(mod, "nll_loss", recording)
    common = ["--dataset", "directed", "--dim", "16", "--num_layers", "3", "--hidden", "32", "--classes", "22", "--epochs", "2",
              "--model", "gatv2", "--heads", "4"]
    with pytest.raises(RuntimeError, match="symmetric"):
        mod.main(common)
    del losses[:]
    torch.manual_seed(0)
    net = mod.main(common + ["--directed"])
    assert "Train (ms/epoch):" in capsys.readouterr().out
    print("losses", losses)
    assert len(losses) == 9 + 2 and all(np.isfinite(losses)), losses
    assert losses[-1] < losses[-2] < losses[0], losses  # the two timed epochs keep going down
    assert net.conv1.directed and net.conv2.conv.directed
    for name, prm in net.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    with pytest.raises(SystemExit):
        mod.parse_args(["--model", "gcn", "--directed"])  # the binary layer functions aggregate with A
    assert mod.parse_args(["--model", "gcn", "--directed", "--norm", "mean"]).directed
