"""Gated neighbour aggregation on fp16 / bf16 operands (hcspmm_forward_gated_typed, spmm_gate16.hip) and the gather_dtype form of
gated_aggregate / ResGatedGraphConv, on an MI355X.  The operands are widened exactly and the arithmetic after that is the fp32
kernel's, so test_z_gated_gpu.py's rule applies as it stands to the widened values (fp64 reference, fp32 CSR-order numpy yardstick,
4 x its error + 1e-6 max|ref| per row group; the fp32 kernel's worst error / bound was 0.23).  Widths: 4 (one 8-byte lane), 6 / 22
(moved-back 4-element lanes at L = 4 / 8), 32 (the first 8-element width), 34 (a moved-back 16-byte lane), 64 (one panel), 130
(panel boundary + ragged tail), 256.  The module's name sorts it behind every other one, as test_z_gated_gpu.py's does."""
import numpy as np
import pytest
import torch

import frontends
from hcspmm import graphs
from test_softmax_aggr_gpu import PLANS, _bits_equal, _bounds, _check_bound, _csr, _graph, _np, _pkg_imports, _sum_rows, _symmetric
from test_width_edges_gpu import FORMS as ONE_PASS_FORMS
from test_z_gated_gpu import BOTH, _checker, _operands, _same_bits, _t, dev, gated_reference  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
WIDTHS = [4, 6, 22, 32, 34, 64, 130, 256]
FORMS = dict({k: PLANS[k] for k in ("default", "panel32", "tiny_segments", "plan_free")},
             **{k: ONE_PASS_FORMS[k] for k in ("one_pass_slices", "one_pass_segments", "one_pass_dense")})
_CACHE, _REFS, _WORST = {}, {}, {}


def _prep(fe, dev, rp, col, form, num_columns=None):
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = _t(rp, dev), _t(col, dev)
    bp, e2c, e2r, ht, row_nzr, col_nzr = fe.preprocess(col_d, rp_d, N, E, (N + 15) // 16, rule=3, num_columns=num_columns)
    p = dict(FORMS[form])
    force, plan = p.pop("force", None), p.pop("plan", True)
    if force is not None:
        ht = torch.full_like(ht, force)
    row_nzr = (fe.build_plan(rp_d, col_d, bp, e2c, ht, num_columns=num_columns, **p) if plan
               else torch.zeros(1, dtype=torch.int32, device=dev))
    return (rp_d, col_d, bp, e2c, e2r, ht, row_nzr, col_nzr)


def _args(fe, dev, kind, form):
    if (fe.name, kind, form) not in _CACHE:
        _CACHE[(fe.name, kind, form)] = _prep(fe, dev, *(_symmetric(*_graph("powerlaw")) if kind == "sym" else _graph(kind)), form)
    return _CACHE[(fe.name, kind, form)]


def _refs(key, rp, col, D, dtype, rows=None):
    """operands rounded to dtype, the fp64 reference on their widened values and the bounds: once per graph, width and type"""
    if key + (D, dtype) not in _REFS:
        n = len(rp) - 1
        ops = [torch.from_numpy(a).to(dtype) for a in _operands(np.random.default_rng(7900 + D), n, rows or n, D)]
        wide = [o.float().numpy() for o in ops]
        r64, y32 = gated_reference(rp, col, *wide, np.float64), gated_reference(rp, col, *wide, np.float32)
        _REFS[key + (D, dtype)] = (ops, r64, [_bounds(r, y, np.diff(rp)) for r, y in zip(r64, y32)])
    return _REFS[key + (D, dtype)]


def _rect():
    rp, col = graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    return rp[:1201].copy(), col[:rp[1200]].copy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,form", [(k, f) for k in ("powerlaw", "molecule") for f in FORMS] + [("rect", "default"), ("rect", "plan_free")])
def test_both_outputs_on_continuous_data(dev, kind, form, dtype):
    """both front-ends within the bound (rect: a row block whose column ids index taller Q and V); and P / Q / V as column blocks
    of one [N, 3 D + 10] buffer, 2 elements in, NaN everywhere else, give the contiguous call's bits"""
    rect = kind == "rect"
    rp, col = _rect() if rect else _graph(kind)
    for fe, widths in ((frontends.get("extension"), [22, 64] if rect else WIDTHS), (frontends.get("ctypes"), [] if rect else [6, 34, 130])):
        args = _prep(fe, dev, rp, col, form, num_columns=3000) if rect else _args(fe, dev, kind, form)
        for D in widths:
            ops, r64, bounds = _refs((kind,), rp, col, D, dtype, rows=3000 if rect else None)
            ops = [o.to(dev) for o in ops]
            out = fe.forward_gated(*ops, *args, outputs=BOTH)
            for o, ref, bd, name in zip(out, r64, bounds, BOTH):
                assert o.dtype == torch.float32 and o.shape == ref.shape
                _check_bound(_np(o), ref, bd, (kind, form, fe.name, D, str(dtype), name), _WORST)
            if fe.name == "extension" and form in ("default", "plan_free") and D in (6, 34, 130):
                buf = torch.full((len(rp) - 1, 3 * D + 10), float("nan"), device=dev, dtype=dtype)
                views = [buf[:, 2 + k * D:2 + (k + 1) * D] for k in range(3)]
                for v, src in zip(views, ops):
                    v.copy_(src)
                framed = fe.forward_gated(*views, *args, outputs=BOTH)
                assert _same_bits(out[0], framed[0]) and _same_bits(out[1], framed[1]), (kind, form, D)
    print("largest error / bound so far: %s" % {k: round(v, 3) for k, v in _WORST.items()})


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_fp32_kernels_bits_where_the_order_is_fixed(dev, dtype):
    """plan-free rows of 0 ... 64 entries are one lane group's CSR-order sum at any lane count, in both units: the 16-bit call has
    the bits of forward_gated on the widened operands, and each single-output call the bits of the two-output one"""
    fe = frontends.get("extension")
    rng = np.random.default_rng(81)
    N = 325
    rows = np.repeat(np.arange(N), np.arange(N) % 65)
    args = _prep(fe, dev, *_csr(rows, rng.integers(0, N, len(rows)), N), "plan_free")
    for D in (6, 34, 128):
        ops = [_t(a, dev).to(dtype) for a in _operands(rng, N, N, D)]
        both = fe.forward_gated(*ops, *args, outputs=BOTH)
        wide = fe.forward_gated(*(o.float() for o in ops), *args, outputs=BOTH)
        assert _same_bits(both[0], wide[0]) and _same_bits(both[1], wide[1]), D
        assert _same_bits(both[0], fe.forward_gated(*ops, *args)[0]), D
        assert _same_bits(both[1], fe.forward_gated(*ops, *args, outputs=("dgate",))[1]), D


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_saturated_gates_select_exactly(dev, form, dtype):
    """+-200 checkerboards in P, then in Q, on integer V (all exact in both types): the exact integer sums and Z_dgate = +0 -- the
    own-row lookup of every task kind (through the fix-up list on a split row's last segment) and the gathered-row lookup"""
    fe = frontends.get("extension")
    rp, col = _graph("powerlaw")
    N, args = len(rp) - 1, _args(fe, dev, "powerlaw", form)
    for D in (6, 34, 128):
        V = np.random.default_rng(7100 + D).integers(-3, 4, (N, D)).astype(np.float32)
        zero, own, sel = np.zeros((N, D), np.float32), _checker(N, D), _checker(N, D, 1)
        want_p = np.where(own > 0, _sum_rows(V[col].astype(np.float64), rp), 0.0).astype(np.float32) + 0.0
        want_q = _sum_rows(np.where(sel[col] > 0, V[col], 0.0).astype(np.float64), rp).astype(np.float32) + 0.0
        for (P, Q), want in (((own, zero), want_p), ((zero, sel), want_q)):
            Zg, Zd = fe.forward_gated(*(_t(a, dev).to(dtype) for a in (P, Q, V)), *args, outputs=BOTH)
            assert _bits_equal(_np(Zg), want) and _bits_equal(_np(Zd), zero), (form, D)


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_recipe_has_the_forwards_gates_on_a_permutation(dev, dtype):
    """one entry (i, perm[i]) per row and operands / G representable in dtype: out, dP, dQ, dV of gated_aggregate(gather_dtype=)
    equal the per-entry torch fp32 formula on the gates, bit for bit"""
    _pkg_imports()
    import GNN_model
    fe = frontends.get("extension")
    rng = np.random.default_rng(43)
    N = 1500
    perm = rng.permutation(N)
    args = _prep(fe, dev, *_csr(np.arange(N), perm, N), "default")
    pl = torch.from_numpy(perm).to(dev)
    for D in (6, 64):
        P, Q, V = (_t(a, dev).to(dtype) for a in _operands(rng, N, N, D))
        G = torch.randn(N, D, device=dev).to(dtype).float()
        S, dS = fe.forward_gated(P, Q, torch.ones_like(V), *args, outputs=BOTH)  # sigma and sigma' of every entry
        ops = [x.float().requires_grad_(True) for x in (P, Q, V)]
        out = GNN_model.gated_aggregate(*ops, args, directed=True, gather_dtype=dtype)
        out.backward(G)
        want_dV, want_dQ, Vg = torch.empty_like(G), torch.empty_like(G), V.float()[pl]
        want_dV[pl] = S * G
        want_dQ[pl] = Vg * (dS * G)
        assert _same_bits(out, S * Vg) and _same_bits(ops[0].grad, G * (dS * Vg)), D
        assert _same_bits(ops[1].grad, want_dQ) and _same_bits(ops[2].grad, want_dV), D


def test_resgatedgraphconv_gathers_in_bf16(dev):
    """forward and backward run and give finite fp32 results; out against the layer in torch fp64 on the SAME rounded block (the
    layer's own fp32 product, rounded to bf16 as the layer rounds it), within 4 x the fp32 torch layer's error against that
    reference + 1e-6 max|ref|"""
    _pkg_imports()
    import GNN_model
    args = _args(frontends.get("extension"), dev, "sym", "default")
    N, H = args[0].numel() - 1, 16
    torch.manual_seed(35)
    conv = GNN_model.ResGatedGraphConv(24, H, gather_dtype=torch.bfloat16).to(dev)
    X = torch.randn(N, 24, device=dev, requires_grad=True)
    out = conv(X, *args, None)
    out.backward(torch.randn_like(out))
    for t, shape in ((out, (N, H)), (X.grad, (N, 24)), (conv.weights.grad, (24, 4 * H))):
        assert t.dtype == torch.float32 and t.shape == shape and bool(torch.isfinite(t).all())
    proj = GNN_model._Update.apply(X.detach(), conv.weights.detach())
    rows, c = torch.repeat_interleave(torch.arange(N, device=dev), (args[0][1:] - args[0][:-1]).long()), args[1].long()
    res = {}
    for dt in (torch.float64, torch.float32):
        P, Q, V = (proj[:, k * H:(k + 1) * H].to(torch.bfloat16).to(dt) for k in range(3))
        res[dt] = proj[:, 3 * H:].to(dt) + torch.zeros(N, H, dtype=dt, device=dev).index_add(0, rows, torch.sigmoid(P[rows] + Q[c]) * V[c])
    ref = res[torch.float64]
    yard, err = float((res[torch.float32].double() - ref).abs().max()), float((out.detach().double() - ref).abs().max())
    bound = 4.0 * yard + 1e-6 * float(ref.abs().max())
    print("out: library error %.3e, fp32 torch error %.3e, bound %.3e, error / bound %.3f" % (err, yard, bound, err / bound))
    assert err <= bound, (err, yard, bound)


@pytest.mark.parametrize("fe_name", ["ctypes", "extension"])
def test_refusals(dev, fe_name):
    _pkg_imports()
    import GNN_model
    fe = frontends.get(fe_name)
    args = _args(fe, dev, "molecule", "default")
    A = torch.randn(args[0].numel() - 1, 9, device=dev).half()
    even, odd_stride = A[:, :8].contiguous(), A[:, :8]
    for bad in ((A[:, :5].contiguous(),) * 3, (odd_stride,) * 3, (even, odd_stride, even), (even[:, :2].contiguous(),) * 3):
        with pytest.raises(RuntimeError, match="even width"):
            fe.forward_gated(*bad, *args)
    for bad in ((even, even.float(), even.float()), (even.float(), even, even), (even, even.bfloat16(), even.bfloat16())):
        with pytest.raises(RuntimeError):
            fe.forward_gated(*bad, *args)
    with pytest.raises(ValueError, match="gather_dtype"):
        GNN_model.gated_aggregate(even.float(), even.float(), even.float(), args, directed=True, gather_dtype=torch.float64)
    with pytest.raises(ValueError, match="even"):
        GNN_model.ResGatedGraphConv(8, 7, gather_dtype=torch.float16)
