"""GATv2 attention (include/hcspmm.h hcspmm_gatv2_scores, hcspmm_gatv2_scores_backward; GNN_model.gatv2_attention,
GATv2Conv; HC-SpMM_main.py --model gatv2) on an MI355X, through both Python front-ends.

Every bound follows from the operation order the header states, with u = 2^-24:
  * forward: per element z and l are rounded once each, then Dh terms are summed with one rounding per addition in some
    order (fmaf chains and a butterfly): at most Dh + 2 roundings touch a term, so
        |out - ref| <= (Dh + 3) u sum_k |att_k l_k| + 2^-126;
  * grad_H_*: the n_i terms g * d(z) of a row (one rounding each at most), n_i - 1 additions, one product with att:
        |got - ref| <= (n_i + 3) u |att_j| sum_e |g_e d_e| + 2^-126;
  * grad_att: E terms g * l (z, l and the product-sum rounded), at most E - 1 additions on any path:
        |got - ref| <= (E + 4) u sum_e |g l| + 2^-126.
The references are torch fp64 from the same fp32 inputs; the branch of every element is taken from the fp32 sum z, whose
sign is that of the exact sum (an fp32 sum of two fp32 numbers is zero only when it is exact: denormals are kept).
"""
import ctypes
import importlib.util
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
TINY = 2.0 ** -126
SLOPE = 0.2
SLOPE64 = float(np.float32(SLOPE))  # the kernels multiply by the fp32 slope

GRAPHS = ["thresholds", "powerlaw", "community", "planted", "molecule"]
# heads x Dh, and the multi-pass path (more columns than a wave's 64 lanes x 4 cover)
SHAPES = [(h, dh) for h in (1, 2, 4, 8) for dh in (4, 8, 12, 32, 64)] + [(1, 320)]


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
    """Symmetric: a star with 12 000 leaves, complete bipartite blocks K(4, 16), K(3, 17), K(3, 2048), K(2, 2049) and 300
    isolated nodes: rows of 0, 1, 16, 17, 2048, 2049 and 12 000 entries; node ids shuffled so that workgroups mix them."""
    rows, cols, nxt = [], [], 0
    for a, b in ((1, 12000), (4, 16), (3, 17), (3, 2048), (2, 2049)):
        left, right = np.arange(nxt, nxt + a), np.arange(nxt + a, nxt + a + b)
        nxt += a + b
        r, c = np.repeat(left, b), np.tile(right, a)
        rows.extend([r, c])
        cols.extend([c, r])
    N = nxt + 300
    relabel = np.random.default_rng(41).permutation(N)
    rp, col = _csr(N, relabel[np.concatenate(rows)], relabel[np.concatenate(cols)])
    assert {0, 1, 16, 17, 2048, 2049, 12000} <= set(np.diff(rp).tolist())
    return rp, col


def _symmetric(rp, col):
    """the pattern of A + A^T (the backward needs a symmetric pattern)"""
    N = len(rp) - 1
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(rp))
    key = np.unique(np.concatenate([rows * N + col, col.astype(np.int64) * N + rows]))
    out = np.zeros(N + 1, np.int32)
    np.cumsum(np.bincount(key // N, minlength=N), out=out[1:])
    return out, (key % N).astype(np.int32)


def _raw_graph(kind):
    if kind == "thresholds":
        return _threshold_graph()
    if kind == "powerlaw":
        return graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    if kind == "community":
        return graphs.community_graph(3000, 40000, seed=5)[:2]
    if kind == "planted":
        return graphs.planted_dense_graph(1200, seed=8)
    if kind == "molecule":
        return graphs.molecule_graph(2500, seed=9)
    raise KeyError(kind)


_CACHE = {}


def _setup(dev, kind, symmetric=False):
    """the generator's graph as it comes (forward), or its symmetrised pattern with the transpose permutation (backward)"""
    key = (kind, symmetric)
    if key not in _CACHE:
        rp, col = _raw_graph(kind)
        if symmetric:
            rp, col = _symmetric(rp, col)
        N = len(rp) - 1
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        g = dict(N=N, E=len(col), rp=rp_d, col=col_d, cols=col_d.long(),
                 rows=torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).to(dev), lens=torch.from_numpy(np.diff(rp)).to(dev))
        if symmetric:
            g["perm"] = frontends.get("ctypes").transpose_permutation(rp_d, col_d)
        _CACHE[key] = g
    return _CACHE[key]


def _features(dev, n, D, seed, sign=1.0):
    """[n, D] float32 with magnitudes spread over 1e-3 ... 30; every fifth column is +-0.5, so that H_dst(sign = 1) +
    H_src(sign = -1) is exactly zero there on every entry"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    mag = 10.0 ** (torch.rand((n, D), device=dev, generator=gen) * (np.log10(30.0) + 3.0) - 3.0)
    x = mag * torch.where(torch.rand((n, D), device=dev, generator=gen) < 0.5, -1.0, 1.0)
    x[:, ::5] = 0.5 * sign
    return x.float()


def _att(dev, heads, dh, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand((heads, dh), device=dev, generator=gen) * 2 - 1).float()


def _layouts(dev, hd, hs):
    """the operands as contiguous tensors, and as the two halves of one [n, 2 D] buffer (square graphs: equal row counts)"""
    yield "contiguous", hd, hs
    if hd.size(0) == hs.size(0):
        both = torch.cat([hs, hd], 1)
        D = hd.size(1)
        yield "views", both[:, D:], both[:, :D]


def _elements(hd, hs, att, rows, cols):
    """per entry and column, in fp64 from the fp32 inputs: l, d(z), and the fp32 z that decides the branch"""
    z32 = hd[rows] + hs[cols]  # one rounded fp32 add, as the kernel's
    z64 = hd.double()[rows] + hs.double()[cols]
    pos = z32 > 0
    assert bool((pos == (z64 > 0)).all())
    l64 = torch.where(pos, z64, z64 * SLOPE64)
    d64 = torch.where(pos, torch.ones_like(z64), torch.full_like(z64, SLOPE64))
    return z32, l64, d64


def _scores64(hd, hs, att, rows, cols):
    heads, dh = att.shape
    z32, l64, _ = _elements(hd, hs, att, rows, cols)
    prod = (l64 * att.double().reshape(1, -1)).reshape(-1, heads, dh)
    return prod.sum(2).t(), prod.abs().sum(2).t(), z32


def _check_scores(out, hd, hs, att, rows, cols, what):
    heads, dh = att.shape
    want, mag, z32 = _scores64(hd, hs, att, rows, cols)
    assert out.shape == (heads, rows.numel()) and out.dtype == torch.float32
    err = (out.double() - want).abs()
    bound = (dh + 3) * U * mag + TINY
    worst = float((err / bound).max()) if err.numel() else 0.0
    print("gatv2 forward %s heads=%d Dh=%d: worst error / bound = %.3f" % (what, heads, dh, worst))
    assert bool((err <= bound).all()), (what, heads, dh, worst)
    return z32


# ------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("heads,dh", SHAPES)
@pytest.mark.parametrize("kind", GRAPHS)
def test_scores_match_fp64(fe, dev, kind, heads, dh):
    g = _setup(dev, kind)
    D = heads * dh
    hd, hs = _features(dev, g["N"], D, 11 * heads + dh), _features(dev, g["N"], D, 13 * heads + dh + 1, sign=-1.0)
    att = _att(dev, heads, dh, 7 * heads + dh)
    first = None
    for name, a, b in _layouts(dev, hd, hs):
        out = fe.gatv2_scores(a, b, att, g["rp"], g["col"], SLOPE)
        z32 = _check_scores(out, hd, hs, att, g["rows"], g["cols"], "%s/%s" % (kind, name))
        zh = z32.reshape(-1, heads, dh)
        assert bool((z32 == 0).any()) and bool((zh < 0).any(2).any(0).all()) and bool((zh > 0).any(2).any(0).all())
        assert float(z32.abs().max()) > 10.0 and float(z32[z32 != 0].abs().min()) < 1e-2
        assert torch.equal(out, fe.gatv2_scores(a, b, att, g["rp"], g["col"], SLOPE))  # two calls, the same bits
        if first is None:
            first = out
        assert torch.equal(out, first)  # the leading dimension does not change a bit


def test_scores_of_a_row_block(fe, dev):
    """rectangular H_src: rows [lo, hi) of a larger graph keep their global column ids"""
    g = _setup(dev, "powerlaw")
    lo, hi = 1000, 2200
    rp = g["rp"].cpu().numpy()
    e0, e1 = int(rp[lo]), int(rp[hi])
    rp_b = torch.from_numpy((rp[lo:hi + 1] - rp[lo]).astype(np.int32)).to(dev)
    col_b = g["col"][e0:e1].contiguous()
    rows_b = g["rows"][e0:e1] - lo
    for heads, dh in ((1, 32), (4, 16), (8, 64)):
        D = heads * dh
        hd, hs = _features(dev, hi - lo, D, 3 + heads), _features(dev, g["N"], D, 4 + heads, sign=-1.0)
        att = _att(dev, heads, dh, 5)
        out = fe.gatv2_scores(hd, hs, att, rp_b, col_b, SLOPE)
        _check_scores(out, hd, hs, att, rows_b, col_b.long(), "row block")


@pytest.mark.parametrize("heads,dh", [(2, 4), (4, 12), (4, 16), (8, 8), (4, 32), (8, 64)])
def test_front_ends_and_single_head_calls_give_the_same_bits(dev, heads, dh):
    g = _setup(dev, "thresholds")
    D = heads * dh
    hd, hs = _features(dev, g["N"], D, 21), _features(dev, g["N"], D, 22, sign=-1.0)
    att = _att(dev, heads, dh, 23)
    a, b = (frontends.get(n).gatv2_scores(hd, hs, att, g["rp"], g["col"], SLOPE) for n in ("ctypes", "extension"))
    assert torch.equal(a, b)
    fe = frontends.get("ctypes")
    for h in range(heads):  # the contract of the other multi-head kernels
        sl = slice(h * dh, (h + 1) * dh)
        one = fe.gatv2_scores(hd[:, sl], hs[:, sl], att[h], g["rp"], g["col"], SLOPE)
        assert one.shape == (g["E"],) and torch.equal(one, a[h]), h


def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


@pytest.mark.parametrize("kind", ["thresholds", "powerlaw"])
def test_attention_is_the_edge_softmax_of_the_scores(fe, dev, kind):
    _pkg_imports()
    import GNN_model
    import HCSPMM
    g = _setup(dev, kind, symmetric=True)
    heads, dh = 4, 16
    hd, hs = _features(dev, g["N"], heads * dh, 31) * 0.1, _features(dev, g["N"], heads * dh, 32, sign=-1.0) * 0.1
    att = _att(dev, heads, dh, 33)
    graph = (g["rp"], g["col"]) + tuple(HCSPMM.preprocess(g["col"], g["rp"], g["N"], g["E"], (g["N"] + 15) // 16, -1))
    alpha = GNN_model.gatv2_attention(hd, hs, att, graph, SLOPE)
    assert torch.equal(alpha, fe.edge_softmax(fe.gatv2_scores(hd, hs, att, g["rp"], g["col"], SLOPE), g["rp"]))
    sums = torch.zeros((heads, g["N"]), dtype=torch.float64, device=dev).index_add_(1, g["rows"], alpha.double())
    full = g["lens"] > 0
    assert bool(((sums[:, full] - 1).abs() <= 1e-5).all())  # the edge softmax's own bar: 1e-5 of every alpha
    assert bool((sums[:, ~full] == 0).all())


# ------------------------------------------------------------------------------------------- backward
def _backward64(gl, hd, hs, att, g):
    """fp64 gradients and the magnitudes of their bounds; the per-entry terms are summed by row for H_dst and by COLUMN for
    H_src (index_add: no use of perm)"""
    heads, dh = att.shape
    N, rows, cols = g["N"], g["rows"], g["cols"]
    _, l64, d64 = _elements(hd, hs, att, rows, cols)
    ge = gl.double().t().repeat_interleave(dh, 1)  # [E, D]: g[h(j)][e]
    term = ge * d64
    a64 = att.double().reshape(1, -1)
    zeros = lambda: torch.zeros((N, heads * dh), dtype=torch.float64, device=hd.device)
    want_dst, mag_dst = a64 * zeros().index_add_(0, rows, term), a64.abs() * zeros().index_add_(0, rows, term.abs())
    want_src, mag_src = a64 * zeros().index_add_(0, cols, term), a64.abs() * zeros().index_add_(0, cols, term.abs())
    gl_l = ge * l64
    return want_dst, mag_dst, want_src, mag_src, gl_l.sum(0).reshape(heads, dh), gl_l.abs().sum(0).reshape(heads, dh)


@pytest.mark.parametrize("heads,dh", SHAPES)
@pytest.mark.parametrize("kind", GRAPHS)
def test_backward_matches_fp64(fe, dev, kind, heads, dh):
    g = _setup(dev, kind, symmetric=True)
    D, N, E = heads * dh, g["N"], g["E"]
    hd, hs = _features(dev, N, D, 41 * heads + dh), _features(dev, N, D, 43 * heads + dh, sign=-1.0)  # H_dst != H_src
    att = _att(dev, heads, dh, 47)
    gen = torch.Generator(device=dev).manual_seed(heads + dh)
    gl = torch.randn((heads, E), device=dev, generator=gen)
    assert not torch.equal(gl, gl[:, g["perm"]])  # not symmetric under the transpose: g[e] for g[perm[e]] would show
    want_dst, mag_dst, want_src, mag_src, want_att, mag_att = _backward64(gl, hd, hs, att, g)
    n = g["lens"].double().reshape(-1, 1)
    first = None
    for name, a, b in _layouts(dev, hd, hs):
        got = fe.gatv2_scores_backward(gl, a, b, att, g["rp"], g["col"], g["perm"], SLOPE)
        gd, gs, ga = got
        assert gd.shape == (N, D) and gs.shape == (N, D) and ga.shape == (heads, dh)
        worst = []
        for x, want, mag in ((gd, want_dst, mag_dst), (gs, want_src, mag_src)):
            err, bound = (x.double() - want).abs(), (n + 3) * U * mag + TINY
            worst.append(float((err / bound).max()))
            assert bool((err <= bound).all()), (kind, name, heads, dh, worst)
        err, bound = (ga.double() - want_att).abs(), (E + 4) * U * mag_att + TINY
        worst.append(float((err / bound).max()))
        print("gatv2 backward %s/%s heads=%d Dh=%d: worst error / bound dst %.3f src %.3f att %.4f" % ((kind, name, heads, dh) + tuple(worst)))
        assert bool((err <= bound).all()), (kind, name, heads, dh, worst)
        again = fe.gatv2_scores_backward(gl, a, b, att, g["rp"], g["col"], g["perm"].int(), SLOPE)
        for x, y in zip(got, again):
            assert torch.equal(x, y)  # two calls, the same bits
        if first is None:
            first = got
        for x, y in zip(got, first):
            assert torch.equal(x, y)
    other = frontends.get("extension" if fe.name == "ctypes" else "ctypes")
    for x, y in zip(first, other.gatv2_scores_backward(gl, hd, hs, att, g["rp"], g["col"], g["perm"], SLOPE)):
        assert torch.equal(x, y)


def test_derivative_at_zero_is_the_negative_slope(fe, dev):
    """every z is exactly 0: grad_H = att * slope * the row sums of g"""
    g = _setup(dev, "powerlaw", symmetric=True)
    heads, dh = 2, 8
    hd = torch.full((g["N"], heads * dh), 0.75, device=dev)
    att = _att(dev, heads, dh, 51)
    gl = torch.ones((heads, g["E"]), device=dev)
    gd, gs, ga = fe.gatv2_scores_backward(gl, hd, -hd, att, g["rp"], g["col"], g["perm"], 0.25)
    want = g["lens"].float().reshape(-1, 1) * 0.25 * att.reshape(1, -1)  # exact in fp32: small integers times 0.25
    assert torch.equal(gd, want) and torch.equal(gs, want)
    assert bool((ga == 0).all())


# ------------------------------------------------------------------------------------------- edge cases
def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _capi_backward(gl, hd, hs, att, rp, col, perm, N, E, D, heads, gd, gs, ga, ws, ws_bytes=None, slope=SLOPE, ld=None):
    ld = D if ld is None else ld
    return capi.lib().hcspmm_gatv2_scores_backward(
        _p(gl), _p(hd), ld, _p(hs), ld, _p(att), slope, _p(rp), _p(col), _p(perm), N, E, D, heads, _p(gd), ld, _p(gs), ld, _p(ga),
        _p(ws), ws.numel() * 4 if ws_bytes is None else ws_bytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _workspace(dev, N, E, D, heads):
    n = capi.lib().hcspmm_gatv2_backward_workspace_bytes(N, E, D, heads)
    return torch.empty(n // 4, dtype=torch.float32, device=dev)


def test_without_entries_the_gradients_are_zeros(fe, dev):
    N, heads, dh = 37, 3, 8
    D = heads * dh
    rp = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    col = torch.zeros(0, dtype=torch.int32, device=dev)
    h, att = torch.randn(N, D, device=dev), _att(dev, heads, dh, 1)
    out = fe.gatv2_scores(h, h, att, rp, col)
    assert out.shape == (heads, 0)
    for t in fe.gatv2_scores_backward(out, h, h, att, rp, col, col):
        assert bool((t == 0).all())
    gd, gs, ga = _nan((N, D), dev), _nan((N, D), dev), _nan((heads, dh), dev)
    assert _capi_backward(None, h, h, att, rp, None, None, N, 0, D, heads, gd, gs, ga, _workspace(dev, N, 0, D, heads)) == 0
    torch.cuda.synchronize()
    assert bool((gd == 0).all()) and bool((gs == 0).all()) and bool((ga == 0).all())


def test_rows_without_entries_get_zeros(dev):
    g = _setup(dev, "thresholds", symmetric=True)
    heads, dh = 4, 8
    D, N, E = heads * dh, g["N"], g["E"]
    hd, hs, att = _features(dev, N, D, 61), _features(dev, N, D, 62, sign=-1.0), _att(dev, heads, dh, 63)
    gl = torch.randn((heads, E), device=dev)
    gd, gs, ga = _nan((N, D), dev), _nan((N, D), dev), _nan((heads, dh), dev)
    assert _capi_backward(gl, hd, hs, att, g["rp"], g["col"], g["perm"].int(), N, E, D, heads, gd, gs, ga,
                          _workspace(dev, N, E, D, heads)) == 0
    torch.cuda.synchronize()
    empty = g["lens"] == 0
    assert int(empty.sum()) == 300
    assert bool((gd[empty] == 0).all()) and bool((gs[empty] == 0).all())
    assert not bool(torch.isnan(gd).any() or torch.isnan(gs).any() or torch.isnan(ga).any())


def test_forward_and_backward_replay_in_a_hip_graph(fe, dev):
    g = _setup(dev, "thresholds", symmetric=True)
    heads, dh = 4, 16
    D = heads * dh
    hd, hs, att = _features(dev, g["N"], D, 71), _features(dev, g["N"], D, 72, sign=-1.0), _att(dev, heads, dh, 73)
    gl = torch.randn((heads, g["E"]), device=dev)
    perm32 = g["perm"].int()
    ref_out = fe.gatv2_scores(hd, hs, att, g["rp"], g["col"], SLOPE)
    ref = fe.gatv2_scores_backward(gl, hd, hs, att, g["rp"], g["col"], perm32, SLOPE)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fe.gatv2_scores(hd, hs, att, g["rp"], g["col"], SLOPE)
        outs = fe.gatv2_scores_backward(gl, hd, hs, att, g["rp"], g["col"], perm32, SLOPE)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref_out)
    for a, b in zip(outs, ref):
        assert torch.equal(a, b)
    hs.copy_(_features(dev, g["N"], D, 74))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fe.gatv2_scores(hd, hs, att, g["rp"], g["col"], SLOPE))
    for a, b in zip(outs, fe.gatv2_scores_backward(gl, hd, hs, att, g["rp"], g["col"], perm32, SLOPE)):
        assert torch.equal(a, b)


def test_argument_errors_raise(fe, dev):
    g = _setup(dev, "powerlaw", symmetric=True)
    N, E, rp, col, perm = g["N"], g["E"], g["rp"], g["col"], g["perm"]
    h, att = torch.randn(N, 16, device=dev), torch.randn(2, 8, device=dev)
    # the library's own refusals arrive as its error code
    for args in ((h, h, att, rp, col, float("nan")), (h, h, att, rp, col, float("inf")),
                 (h[:, :12], h[:, :12], torch.randn(2, 6, device=dev), rp, col)):  # Dh % 4
        with pytest.raises(RuntimeError, match=r"invalid argument.*code -1"):
            fe.gatv2_scores(*args)
    for bad in (h.double(), h[:N - 1], h.cpu(), h.t(), h[:, ::2]):
        with pytest.raises(RuntimeError):
            fe.gatv2_scores(bad, h, att, rp, col)
    for bad_att in (torch.randn(3, 8, device=dev), att.double(), att.cpu(), torch.randn(16, 2, device=dev).t()):
        with pytest.raises(RuntimeError):
            fe.gatv2_scores(h, h, bad_att, rp, col)
    with pytest.raises(RuntimeError):
        fe.gatv2_scores(h, torch.randn(N, 24, device=dev), att, rp, col)
    gl = torch.randn(2, E, device=dev)
    fe.gatv2_scores_backward(gl, h, h, att, rp, col, perm)
    for args in ((gl, h, h, att, rp, col, perm[:-1]), (gl, h, h, att, rp, col, perm.float()), (gl, h, h, att, rp, col, perm.cpu()),
                 (gl[:1], h, h, att, rp, col, perm), (gl.double(), h, h, att, rp, col, perm), (gl.cpu(), h, h, att, rp, col, perm),
                 (gl, h, torch.randn(N + 5, 16, device=dev), att, rp, col, perm)):  # rectangular backward
        with pytest.raises(RuntimeError):
            fe.gatv2_scores_backward(*args)
    with pytest.raises(RuntimeError, match=r"invalid argument.*code -1"):
        fe.gatv2_scores_backward(gl, h, h, att, rp, col, perm, float("nan"))


def test_library_error_codes_with_device_pointers(dev):
    """what the front-ends cannot get wrong for the caller (they size the workspace themselves): a short workspace and a
    short leading dimension, refused before any launch -- the outputs keep their NaN"""
    g = _setup(dev, "powerlaw", symmetric=True)
    heads, dh = 2, 8
    D, N, E = heads * dh, g["N"], g["E"]
    h, att, gl = torch.randn(N, D, device=dev), _att(dev, heads, dh, 2), torch.randn((heads, E), device=dev)
    gd, gs, ga = _nan((N, D), dev), _nan((N, D), dev), _nan((heads, dh), dev)
    ws = _workspace(dev, N, E, D, heads)
    assert ws.numel() > 0
    common = (gl, h, h, att, g["rp"], g["col"], g["perm"].int(), N, E, D, heads, gd, gs, ga, ws)
    assert _capi_backward(*common, ws_bytes=ws.numel() * 4 - 4) == capi.EWORKSPACE
    assert _capi_backward(*common, ld=D - 1) == capi.EINVAL
    assert _capi_backward(*common, slope=float("inf")) == capi.EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(gd).all() and torch.isnan(gs).all() and torch.isnan(ga).all())
    assert _capi_backward(*common) == 0


# ------------------------------------------------------------------------------------------- the layer
def _segment_softmax64(x, rows, N):
    idx = rows.expand_as(x)
    m = torch.full((x.size(0), N), -float("inf"), dtype=x.dtype).scatter_reduce(1, idx, x, "amax")
    ex = torch.exp(x - m.gather(1, idx))
    s = torch.zeros((x.size(0), N), dtype=x.dtype).scatter_add(1, idx, ex)
    return ex / s.gather(1, idx)


def _torch_gatv2_64(X, W, att, rows, cols, N, slope, concat, share):
    """the layer in plain torch fp64: index_select, leaky_relu, segment softmax, index_add"""
    heads, dout = att.shape
    width = heads * dout
    h = X @ W
    h_src = h[:, :width]
    h_dst = h_src if share else h[:, width:]
    e = torch.nn.functional.leaky_relu(h_dst.index_select(0, rows) + h_src.index_select(0, cols), slope)  # [E, width]
    logits = (e.reshape(-1, heads, dout) * att[None]).sum(2).t()  # [heads, E]
    alpha = _segment_softmax64(logits, rows, N)
    msg = alpha.t()[:, :, None] * h_src.index_select(0, cols).reshape(-1, heads, dout)
    out = torch.zeros(N, heads, dout, dtype=h.dtype).index_add(0, rows, msg)
    return out.reshape(N, width) if concat else out.mean(1)


def _close(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return bool(((got - want).abs() <= 1e-4 * want.abs().max()).all())


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("heads", [1, 4])
def test_gatv2_layer_matches_plain_torch_fp64(dev, heads, concat, share, monkeypatch):
    _pkg_imports()
    import GNN_model
    import HCSPMM
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = HCSPMM.gatv2_scores, HCSPMM.gatv2_scores_backward

    def counting_fwd(*a, **k):
        calls["fwd"] += 1
        return fwd(*a, **k)

    def counting_bwd(*a, **k):
        calls["bwd"] += 1
        return bwd(*a, **k)

    monkeypatch.setattr(HCSPMM, "gatv2_scores", counting_fwd)
    monkeypatch.setattr(HCSPMM, "gatv2_scores_backward", counting_bwd)
    rp, col = graphs.powerlaw_graph(1500, 20000, seed=21, max_degree_frac=0.2)
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    args = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16, -1))
    torch.manual_seed(heads + 2 * concat + 4 * share)
    conv = GNN_model.GATv2Conv(24, 16, 0, heads=heads, concat=concat, share_weights=share).to(dev)
    assert conv.weights.shape == (24, heads * 16 * (1 if share else 2)) and conv.att.shape == (heads, 16)
    X = torch.randn(N, 24, device=dev, requires_grad=True)
    Y = conv(X, *args, None)
    assert Y.shape == (N, heads * 16 if concat else 16)
    assert calls == {"fwd": 1, "bwd": 0}
    G = torch.randn_like(Y)
    (Y * G).sum().backward()
    assert calls == {"fwd": 1, "bwd": 1}
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp))).long()
    cols = torch.from_numpy(col).long()
    leaves = [t.detach().cpu().double().requires_grad_(True) for t in (X, conv.weights, conv.att)]
    Y64 = _torch_gatv2_64(*leaves, rows, cols, N, conv.negative_slope, concat, share)
    (Y64 * G.cpu().double()).sum().backward()
    assert _close(Y, Y64)
    for name, got, want in zip(("X", "weights", "att"), (X.grad, conv.weights.grad, conv.att.grad), leaves):
        assert _close(got, want.grad), (name, heads, concat, share)


def test_gatv2_layer_refusals(dev):
    _pkg_imports()
    import GNN_model
    import HCSPMM
    for bad in (6, 0, 2):
        with pytest.raises(ValueError, match="multiple of 4"):
            GNN_model.GATv2Conv(8, bad)
    conv = GNN_model.GATv2Conv(24, 16, 0, heads=2).to(dev)
    rp2, col2 = graphs.uniform_graph(500, 3000, seed=6)
    rp2_d, col2_d = torch.from_numpy(rp2).to(dev), torch.from_numpy(col2).to(dev)
    args2 = (rp2_d, col2_d) + tuple(HCSPMM.preprocess(col2_d, rp2_d, 500, len(col2), (500 + 15) // 16, -1))
    with pytest.raises(RuntimeError, match="symmetric"):
        conv(torch.randn(500, 24, device=dev), *args2, None)
    with pytest.raises(ValueError, match="edge_weight"):
        conv(torch.randn(500, 24, device=dev), *args2, None, edge_weight=torch.ones(len(col2), device=dev))


@pytest.mark.parametrize("extra", [[], ["--gat-concat"]])
def test_driver_trains_gatv2(extra, capsys, monkeypatch):
    _pkg_imports()
    monkeypatch.chdir(PKG)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_gatv2", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = []
    nll = mod.nll_loss

    def recording(log_probs, target):
        loss = nll(log_probs, target)
        losses.append(float(loss.detach()))
        return loss

    monkeypatch.setattr(mod, "nll_loss", recording)
    torch.manual_seed(0)
    net = mod.main(["--dataset", "example", "--dim", "16", "--num_layers", "3", "--hidden", "32", "--classes", "22",
                    "--epochs", "3", "--model", "gatv2", "--heads", "4"] + extra)
    assert "Train (ms/epoch):" in capsys.readouterr().out
    assert len(losses) == 9 + 3 and all(np.isfinite(losses)), losses
    assert net.conv1.concat == bool(extra) and net.conv1.att.shape == (4, 8 if extra else 32)
    for name, prm in net.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    net.eval()
    with torch.no_grad():
        logp = net()
    assert logp.shape == (600, 22) and torch.isfinite(logp).all()
