"""Softmax aggregation on fp16 / bf16 features (hcspmm_forward_softmax_typed / hcspmm_softmax_backward_typed: spmm_softmax16.hip,
softmax_aggr_grad16.hip), SoftmaxAggregate16 and the 16-bit GENConv, on an MI355X.  The operands are widened exactly and the
arithmetic is fp32, so test_softmax_aggr_gpu.py's rule applies to the widened values: the reference is the formula in fp64 numpy,
the yardstick the same formula in fp32 numpy (two passes, CSR-order sums), and LSE, Var and dX may err by 4 x the yardstick's
maximum error + 1e-6 max|ref| per row group; Z gets one rounding of its type on top (2^-8 |ref| bf16, 2^-11 |ref| fp16).  Widths:
4 (one 8-byte lane), 6 / 22 (moved-back 4-element lanes at L = 4 / 8), 32 (the first 8-element width), 34 (a moved-back 16-byte
lane), 64 (one panel), 130 (panel boundary + ragged tail), 256.  The module's name sorts it behind every other GPU module."""
import numpy as np
import pytest
import torch

import frontends
from test_softmax_aggr_gpu import _bounds, _check_bound, _csr, _graph, _np, _pkg_imports, _sum_rows, _symmetric
from test_z_gated_gpu import _same_bits, _t, dev  # noqa: F401  (dev: the fixture)
from test_zz_gated_h16_gpu import FORMS, _args, _prep

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
WIDTHS = [4, 6, 22, 32, 34, 64, 130, 256]
ROUND = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
BOTH = ("lse", "var")
_REFS, _WORST = {}, {}


def _forward(rp, col, X, b, dt):
    """(Z, LSE, Var) of the formula in `dt` arithmetic on the widened X; s = fl32(beta x) and its row maximum are exact"""
    lens = np.diff(rp)
    rows = np.repeat(np.arange(len(rp) - 1), lens)
    s = X[col] * b[None, :]
    M = np.full((len(rp) - 1, X.shape[1]), -np.inf, np.float32)
    M[lens > 0] = np.maximum.reduceat(s, rp[:-1][lens > 0], axis=0)
    V = X[col].astype(dt)
    w = np.exp(s.astype(dt) - M[rows].astype(dt))
    L = _sum_rows(w, rp)
    safe = np.where(L > 0, L, 1).astype(dt)
    Z, Q = _sum_rows(w * V, rp) / safe, _sum_rows(w * (V * V), rp) / safe
    with np.errstate(divide="ignore"):
        return Z, M.astype(dt) + np.log(L), Q - Z * Z


def _backward(rp, col, G, Z, LSE, X, b, dt):
    """dX of the formula in `dt` arithmetic on the walked graph (rp, col): row j sums over its entries (j, i)"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    x, s = X.astype(dt)[rows], (X * b[None, :])[rows].astype(dt)
    term = np.exp(s - LSE[col].astype(dt)) * G[col].astype(dt) * (1 + b.astype(dt)[None, :] * (x - Z[col].astype(dt)))
    return _sum_rows(term, rp)


def _finite(a):
    return np.where(np.isinf(a), 0.0, a)


def _beta(D):
    """per column in +-[0.25, 4], one column 0"""
    rng = np.random.default_rng(8800 + D)
    b = (rng.uniform(0.25, 4.0, D) * rng.choice([-1.0, 1.0], D)).astype(np.float32)
    b[D // 2] = 0.0
    return b


def _refs(kind, D, dtype):
    """X rounded to dtype, beta, the fp64 forward reference with its bounds, and (sym only) the backward's operands, reference and
    bounds: once per graph, width and type"""
    if (kind, D, dtype) not in _REFS:
        rp, col = _symmetric(*_graph("powerlaw")) if kind == "sym" else _graph(kind)
        rng = np.random.default_rng(8700 + D)
        n, lens, b = len(rp) - 1, np.diff(rp), _beta(D)
        X16 = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dtype)
        X = X16.float().numpy()
        r64, y32 = _forward(rp, col, X, b, np.float64), _forward(rp, col, X, b, np.float32)
        # (LSE of a row without entries is -inf in both: out of the error statistics)
        out = dict(X=X16, b=b, fwd=r64, fwd_bounds=[_bounds(_finite(r), _finite(y), lens) for r, y in zip(r64, y32)])
        if kind == "sym":
            G16 = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dtype)
            Z16, LSE = torch.from_numpy(r64[0]).to(dtype), r64[1].astype(np.float32)
            ops = (G16.float().numpy(), Z16.float().numpy(), LSE, X, b)
            d64 = _backward(rp, col, *ops, np.float64)
            out.update(G=G16, Z=Z16, LSE=LSE, bwd=d64, bwd_bounds=_bounds(d64, _backward(rp, col, *ops, np.float32), lens))
        _REFS[(kind, D, dtype)] = out
    return _REFS[(kind, D, dtype)]


def _check(got, ref, bounds, tag, slack=0.0):
    """_check_bound on the error left after `slack` |ref| (the output's own rounding) is taken off"""
    err = np.maximum(np.abs(got.astype(np.float64) - ref) - slack * np.abs(ref), 0.0)
    _check_bound(ref + err, ref, bounds, tag, _WORST)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,form", [(k, f) for k in ("powerlaw", "molecule") for f in FORMS])
def test_forward_against_fp64(dev, kind, form, dtype):
    for fe, widths in ((frontends.get("extension"), WIDTHS), (frontends.get("ctypes"), [6, 34, 130])):
        args = _args(fe, dev, kind, form)
        for D in widths:
            r = _refs(kind, D, dtype)
            Z, LSE, Var = fe.forward_softmax16(r["X"].to(dev), _t(r["b"], dev), *args, stats=BOTH)
            assert Z.dtype == dtype and LSE.dtype == Var.dtype == torch.float32 and Z.shape == LSE.shape == Var.shape == r["X"].shape
            tag = (kind, form, fe.name, D, str(dtype))
            _check(_np(Z.float()), r["fwd"][0], r["fwd_bounds"][0], tag + ("Z",), ROUND[dtype])
            assert np.array_equal(np.isneginf(_np(LSE)), np.isinf(r["fwd"][1])), tag  # rows without entries: -inf exactly
            _check(_finite(_np(LSE)), _finite(r["fwd"][1]), r["fwd_bounds"][1], tag + ("LSE",))
            _check(_np(Var), r["fwd"][2], r["fwd_bounds"][2], tag + ("Var",))
    print("largest error / bound so far: %s" % {k: round(v, 3) for k, v in _WORST.items()})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", list(FORMS))
def test_backward_against_fp64_on_reference_inputs(dev, form, dtype):
    """Z = the fp64 forward reference rounded to the type, LSE = it rounded to fp32, G ~ N(0, 1) rounded: the backward on its own"""
    for fe, widths in ((frontends.get("extension"), WIDTHS), (frontends.get("ctypes"), [6, 34, 130])):
        args = _args(fe, dev, "sym", form)
        for D in widths:
            r = _refs("sym", D, dtype)
            dX = fe.softmax_backward16(r["G"].to(dev), r["Z"].to(dev), _t(r["LSE"], dev), r["X"].to(dev), _t(r["b"], dev), *args)
            assert dX.dtype == torch.float32 and dX.shape == r["X"].shape and dX.is_contiguous()
            _check(_np(dX), r["bwd"], r["bwd_bounds"], (form, fe.name, D, str(dtype), "dX"))
    print("largest error / bound so far: %s" % {k: round(v, 3) for k, v in _WORST.items()})


@pytest.mark.parametrize("dtype", DTYPES)
def test_fixed_order_bits(dev, dtype):
    """plan-free rows of 0 ... 64 entries are one lane group's CSR-order scan at any lane count, in both units: Z16 is the fp32
    call's Z on the widened X rounded once; Var on or off leaves Z and LSE alone; two calls agree"""
    fe = frontends.get("extension")
    rng = np.random.default_rng(82)
    N = 325
    rows = np.repeat(np.arange(N), np.arange(N) % 65)
    args = _prep(fe, dev, *_csr(rows, rng.integers(0, N, len(rows)), N), "plan_free")
    for D in (6, 34, 128):
        X = _t(rng.standard_normal((N, D)).astype(np.float32), dev).to(dtype)
        b = _t(_beta(D), dev)
        Z, LSE, Var = fe.forward_softmax16(X, b, *args, stats=BOTH)
        assert _same_bits(Z, fe.forward_softmax(X.float(), b, *args, return_stats=False)[0].to(dtype)), D
        Z1, LSE1, none = fe.forward_softmax16(X, b, *args)
        assert none is None and _same_bits(Z, Z1) and _same_bits(LSE, LSE1), D
        again = fe.forward_softmax16(X, b, *args, stats=BOTH)
        assert all(_same_bits(x, y) for x, y in zip((Z, LSE, Var), again)), D
        assert fe.forward_softmax16(X, b, *args, stats=())[1:] == (None, None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_saturated_softmax_selects_exactly(dev, form, dtype):
    """integers in [-3, 3] with beta = +-1000 on a graph with empty rows, repeated columns and a split hub: Z is
    the row max / min; where it is unique LSE = +-1000 Z and Var = 0; rows without entries give +0 / -inf / +0"""
    fe = frontends.get("extension")
    rng = np.random.default_rng(33)
    N = 700
    deg = rng.integers(0, 12, N)
    deg[::7] = 0
    deg[5] = 600
    rows = np.repeat(np.arange(N), deg)
    rp, col = _csr(rows, rng.integers(0, N, rows.size), N)
    args = _prep(fe, dev, rp, col, form)
    has = deg > 0
    for D in (6, 34, 128):
        X = rng.integers(-3, 4, (N, D)).astype(np.float32)
        for sign in (1.0, -1.0):
            best = np.zeros((N, D), np.float32)
            best[has] = sign * np.maximum.reduceat(sign * X[col], rp[:-1][has], axis=0)
            unique = np.zeros((N, D), bool)
            unique[has] = np.add.reduceat((X[col] == best[np.repeat(np.arange(N), deg)]).astype(np.int32), rp[:-1][has], axis=0) == 1
            Z, LSE, Var = (_np(o.float()) for o in fe.forward_softmax16(_t(X, dev).to(dtype), sign * 1000.0, *args, stats=BOTH))
            assert np.array_equal(Z, best) and not np.signbit(Z[~has]).any(), (form, D, sign)
            assert np.array_equal(LSE[unique], sign * 1000.0 * best[unique]) and np.isneginf(LSE[~has]).all(), (form, D, sign)
            assert not Var[unique].any() and not Var[~has].any() and not np.signbit(Var[~has]).any(), (form, D, sign)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "plan_free"])
def test_permutation_graph_pins_the_row_lookups(dev, form, dtype):
    """one entry (j, perm[j]) per row.  Forward, beta = 0: Z = X[perm], LSE = 0, Var = 0.  Backward, beta = 1 on integers with
    LSE[perm[j]] = x_j (the weight is exp2(0) = 1): dX[j] = G[perm[j]] (1 + x_j - Z[perm[j]]), the per-entry torch fp32 formula bit
    for bit -- the own row and all three gathered rows"""
    fe = frontends.get("extension")
    rng = np.random.default_rng(44)
    N = 1500
    perm = rng.permutation(N)
    args = _prep(fe, dev, *_csr(np.arange(N), perm, N), form)
    pl = torch.from_numpy(perm).to(dev)
    for D in (6, 64):
        X, G, Zi = (_t(rng.integers(-3, 4, (N, D)).astype(np.float32), dev) for _ in range(3))
        Z, LSE, Var = fe.forward_softmax16(X.to(dtype), 0.0, *args, stats=BOTH)
        assert torch.equal(Z.float(), X[pl]) and not bool(LSE.any()) and not bool(Var.any()), (form, D)
        lse = torch.empty_like(X)
        lse[pl] = X
        dX = fe.softmax_backward16(G.to(dtype), Zi.to(dtype), lse, X.to(dtype), 1.0, *args)
        assert _same_bits(dX, G[pl] * (1.0 + 1.0 * (X - Zi[pl])) + 0.0), (form, D)  # (+ 0: the kernel's fma sum starts from +0)


def test_layers_in_bf16(dev):
    """softmax_aggregate(activation_dtype=bf16) with a learnt t against the formula in torch fp64 on the same rounded X, within 4 x
    the fp32 torch formula's error + 1e-6 max|ref| + one bf16 rounding; GENConv(24, 16, learn_t, bf16): dtypes, shapes, finite
    gradients, and out against the layer in torch fp64 on the tensors the layer rounds (the aggregate it forms included)"""
    _pkg_imports()
    import GNN_model
    args = _args(frontends.get("extension"), dev, "sym", "default")
    N = args[0].numel() - 1
    rows, c = torch.repeat_interleave(torch.arange(N, device=dev), (args[0][1:] - args[0][:-1]).long()), args[1].long()
    bf16 = torch.bfloat16

    def bound_check(out, res, name):
        ref = res[torch.float64]
        yard, err = (res[torch.float32].double() - ref).abs().max(), ((out.detach().double() - ref).abs() - 2.0 ** -8 * ref.abs()).max()
        bound = 4.0 * float(yard) + 1e-6 * float(ref.abs().max())
        print("%s: library error beyond one rounding %.3e, fp32 torch error %.3e, bound %.3e" % (name, float(err), float(yard), bound))
        assert float(err) <= bound, (name, float(err), float(yard), bound)

    torch.manual_seed(36)
    X = torch.randn(N, 24, device=dev, requires_grad=True)
    t = torch.full((), 1.5, device=dev, requires_grad=True)
    agg = GNN_model.softmax_aggregate(X, args, t, activation_dtype=bf16)
    agg.backward(torch.randn_like(agg))
    assert agg.dtype == bf16 and X.grad.dtype == t.grad.dtype == torch.float32 and X.grad.shape == X.shape and t.grad.shape == ()
    assert bool(torch.isfinite(agg).all()) and bool(torch.isfinite(X.grad).all()) and bool(torch.isfinite(t.grad))
    res = {}
    for dt in (torch.float64, torch.float32):
        H = X.detach().to(bf16).to(dt)[c]
        w = torch.exp(1.5 * H)  # |1.5 x| stays small: no running maximum needed
        res[dt] = (torch.zeros(N, 24, dtype=dt, device=dev).index_add(0, rows, w * H)
                   / torch.zeros(N, 24, dtype=dt, device=dev).index_add(0, rows, w).clamp_min(1e-30))
    bound_check(agg, res, "softmax_aggregate")

    conv = GNN_model.GENConv(24, 16, learn_t=True, activation_dtype=bf16).to(dev)
    X = torch.randn(N, 24, device=dev, requires_grad=True)
    out = conv(X, *args, None)
    out.float().sum().backward()
    for v, shape, dtype in ((out, (N, 16), bf16), (X.grad, (N, 24), torch.float32), (conv.weights.grad, (24, 16), torch.float32),
                            (conv.t.grad, (), torch.float32)):
        assert v.dtype == dtype and v.shape == shape and bool(torch.isfinite(v).all())
    X16 = X.detach().to(bf16)
    S16 = X16 + GNN_model.HCSPMM.forward_softmax16(torch.relu(X16) + conv.eps, conv.t.detach(), *args)[0]
    bound_check(out, {dt: S16.to(dt) @ conv.weights.detach().to(bf16).to(dt) for dt in (torch.float64, torch.float32)}, "GENConv")
    with pytest.raises(ValueError, match="even widths"):
        GNN_model.GENConv(24, 15, activation_dtype=bf16)
    with pytest.raises(ValueError, match="activation_dtype"):
        GNN_model.softmax_aggregate(X, args, activation_dtype=torch.float64)


@pytest.mark.parametrize("fe_name", ["ctypes", "extension"])
def test_refusals_come_before_a_launch(dev, fe_name):
    fe = frontends.get(fe_name)
    args = _args(fe, dev, "molecule", "default")
    A = torch.randn(args[0].numel() - 1, 9, device=dev).half()
    even, odd_stride, lse = A[:, :8].contiguous(), A[:, :8], torch.zeros(A.size(0), 8, device=dev)
    for bad in (A[:, :5].contiguous(), odd_stride, even[:, :2].contiguous()):
        with pytest.raises(RuntimeError, match="even width"):
            fe.forward_softmax16(bad, 1.0, *args)
        with pytest.raises(RuntimeError, match="even width"):
            fe.softmax_backward16(even, even, lse, bad, 1.0, *args)
    for bad in ((even.float(), even, lse, even), (even, even.bfloat16(), lse, even), (even, even, lse.half(), even)):
        with pytest.raises(RuntimeError):
            fe.softmax_backward16(*bad, 1.0, *args)
    with pytest.raises(RuntimeError):
        fe.forward_softmax16(even.float(), 1.0, *args)
    with pytest.raises(ValueError):
        fe.forward_softmax16(even, 1.0, *args, stats=("M",))
