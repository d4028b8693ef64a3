"""Edge-feature messages on fp16 / bf16 operands (hcspmm_forward_edge_messages_typed / hcspmm_edge_messages_grad_typed:
spmm_edgevec16.hip, edgevec16_grad.hip), EdgeMessageAggregate16 and the 16-bit GINEConv, on an MI355X.  The operands are widened
exactly and the arithmetic is the fp32 unit's, so test_edge_messages_gpu.py's references and bound apply to the widened values.
Widths: 4 (one 8-byte lane), 6 / 22 (moved-back 4-element lanes), 32 (the first 8-element width), 34 (a moved-back 16-byte lane),
64 (one panel), 130 (panel boundary + ragged tail).  The module's name sorts it behind every other one."""
import ctypes

import numpy as np
import pytest
import torch

import frontends
from test_edge_messages_gpu import OPS, _close, _ints, _messages, _row_sums, _rows_of, _torch_aggregate
from test_softmax_aggr_gpu import _csr, _graph, _pkg_imports, dev  # noqa: F401  (dev: the fixture)
from test_zz_gated_h16_gpu import FORMS, _args, _prep, _rect

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
WIDTHS = {"extension": [4, 6, 22, 32, 34, 64, 130], "ctypes": [6, 34, 130]}
_INT_REFS = {}


def _t16(a, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).to(dtype)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _int_case(kind, D):
    """small-integer operands (exact in both types), a permutation and a many-to-one index, and the int64 sums of every op and
    index form: once per graph and width"""
    if (kind, D) not in _INT_REFS:
        rp, col = _graph(kind)
        N, E = len(rp) - 1, len(col)
        rng = np.random.default_rng(2800 + D)
        X, F, perm, V = _ints(rng, (N, D)), _ints(rng, (E, D)), rng.permutation(E).astype(np.int32), max(E // 5, 1)
        many = rng.integers(0, V, E).astype(np.int32)
        want = {(op, name): _row_sums(rp, _messages(op, X[col], FE)).astype(np.float32)
                for op in OPS for name, FE in (("direct", F), ("perm", F[perm]), ("many", F[:V][many]))}
        _INT_REFS[(kind, D)] = (X, F, perm, many, V, want)
    return _INT_REFS[(kind, D)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,form", [(k, f) for k in ("powerlaw", "molecule") for f in FORMS])
def test_integer_sums_are_exact_on_every_row(dev, kind, form, dtype):
    """every task kind of every plan form, all ops, direct / permuted / many-to-one F rows, both front-ends: int64 numpy, all rows"""
    for fe in (frontends.get("extension"), frontends.get("ctypes")):
        args = _args(fe, dev, kind, form)
        for D in WIDTHS[fe.name]:
            X, F, perm, many, V, want = _int_case(kind, D)
            Xd, Fd, Fs = _t16(X, dev, dtype), _t16(F, dev, dtype), _t16(F[:V], dev, dtype)
            idx = {"direct": None, "perm": torch.from_numpy(perm).to(dev), "many": torch.from_numpy(many).to(dev)}
            for op in OPS:
                for name, Fin in (("direct", Fd), ("perm", Fd), ("many", Fs)):
                    got = fe.forward_edge_messages(None if op == "copy" and D == 34 else Xd, Fin, *args, op, idx[name])[0]
                    assert got.dtype == torch.float32 and torch.equal(got.cpu(), torch.from_numpy(want[(op, name)])), \
                        (kind, form, fe.name, D, op, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_fp32_kernels_bits_where_the_order_is_fixed(dev, dtype):
    """plan-free rows of 0 ... 64 entries are one lane group's CSR-order sum at any lane count, in both units"""
    fe = frontends.get("extension")
    rng = np.random.default_rng(281)
    N = 325
    rows = np.repeat(np.arange(N), np.arange(N) % 65)
    args = _prep(fe, dev, *_csr(rows, rng.integers(0, N, len(rows)), N), "plan_free")
    for D in (6, 34, 128):
        X, F = _t16(rng.standard_normal((N, D)), dev, dtype), _t16(rng.standard_normal((len(rows), D)), dev, dtype)
        for op in OPS:
            got, wide = (fe.forward_edge_messages(x, f, *args, op)[0] for x, f in ((X, F), (X.float(), F.float())))
            assert torch.equal(got.view(torch.int32), wide.view(torch.int32)), (D, op)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,form", [(k, f) for k in ("powerlaw", "molecule") for f in FORMS])
def test_normal_data_within_the_rounding_bound(dev, kind, form, dtype):
    """test_edge_messages_gpu.py's bound, k u / (1 - k u) * scale with u = 2^-24, on the widened operands against fp64"""
    fe = frontends.get("extension")
    rp, col = _graph(kind)
    N, E, args = len(rp) - 1, len(col), _args(fe, dev, kind, form)
    deg, u = np.diff(rp).astype(np.float64)[:, None], 2.0 ** -24
    rng = np.random.default_rng(283)
    for D in (22, 64, 130):
        Xd, Fd = _t16(rng.standard_normal((N, D)), dev, dtype), _t16(rng.standard_normal((E, D)), dev, dtype)
        XC, F64 = Xd.double().cpu().numpy()[col], Fd.double().cpu().numpy()
        for op in OPS:
            got = fe.forward_edge_messages(Xd, Fd, *args, op)[0].double().cpu().numpy()
            k = deg + 2 if op == "add_relu" else deg
            scale = _row_sums(rp, np.abs(XC * F64 if op == "mul" else XC + F64 if op == "add_relu" else F64))
            err, bound = np.abs(got - _row_sums(rp, _messages(op, XC, F64))), k * u / (1 - k * u) * scale
            print(kind, form, D, op, "max err / bound", float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (kind, form, D, op)


def _grad_reference(op, G, X, F, rows, col):
    """the torch expression on the widened operands, rounded once"""
    g = G.float()[rows]
    want = g * X.float()[col] if op == "mul" else torch.where(X.float()[col] + F.float() > 0, g, torch.zeros_like(g)) if op == "add_relu" else g
    return want.to(G.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["powerlaw", "molecule"])  # powerlaw: a hub row cut by the chunk boundaries
def test_gradient_with_respect_to_f_has_the_reference_bits(dev, kind, dtype):
    rp, col = _graph(kind)
    N, E = len(rp) - 1, len(col)
    rows, cl = (torch.from_numpy(a.astype(np.int64)).to(dev) for a in (_rows_of(rp), col))
    rng = np.random.default_rng(284)
    for D, fe in ((4, "extension"), (22, "ctypes"), (34, "extension"), (130, "ctypes")):
        fe = frontends.get(fe)
        rp_d, col_d = _args(fe, dev, kind, "default")[:2]
        G, X, F = (_t16(rng.standard_normal(s), dev, dtype) for s in ((N, D), (N, D), (E, D)))
        for op in OPS:
            got = fe.edge_messages_grad(G, None if op == "copy" else X, F if op == "add_relu" else None, rp_d, col_d, op)
            assert _same_bits(got, _grad_reference(op, G, X, F, rows, cl)), (kind, D, op)
    # every row of gF written, through a strided ldgf: column block [2, 2 + D) of a NaN-filled buffer, the rest untouched
    from hcspmm import capi
    D, ld = 22, 40
    out = torch.full((E, ld), float("nan"), device=dev, dtype=dtype)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    Gc = G[:, :D].contiguous()
    rc = capi.lib().hcspmm_edge_messages_grad_typed(p(Gc), D, p(X), N, X.stride(0), p(F), F.stride(0), 1 + DTYPES.index(dtype), p(out, 4), ld,
                                                    1, p(rp_d), p(col_d), N, E, D, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and _same_bits(out[:, 2:2 + D], _grad_reference("add_relu", G[:, :D], X[:, :D], F[:, :D], rows, cl))
    assert bool(torch.isnan(out[:, :2]).all()) and bool(torch.isnan(out[:, 2 + D:]).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_views_blocks_nans_and_empty_rows(dev, form, dtype):
    fe = frontends.get("extension")
    rp, col = _graph("powerlaw")
    N, E, args = len(rp) - 1, len(col), _args(fe, dev, "powerlaw", form)
    rng = np.random.default_rng(285)
    empty, rows = np.diff(rp) == 0, _rows_of(rp)
    for D in (6, 34):
        X, F = _t16(rng.standard_normal((N, D)), dev, dtype), _t16(rng.standard_normal((E, D)), dev, dtype)
        bx, bf = (torch.full((n, D + 10), float("nan"), device=dev, dtype=dtype) for n in (N, E))
        bx[:, 2:2 + D], bf[:, 2:2 + D] = X, F
        e = int(rp[int(np.argmax(np.diff(rp)))]) + 300  # the middle of the hub
        Fn = F.clone()
        Fn[e] = float("nan")
        for op in OPS:
            Z = fe.forward_edge_messages(X, F, *args, op)[0]
            assert (Z.cpu().numpy()[empty].view(np.int32) == 0).all(), (form, D, op)  # +0
            for again in (fe.forward_edge_messages(X, F, *args, op)[0], fe.forward_edge_messages(bx[:, 2:2 + D], bf[:, 2:2 + D], *args, op)[0]):
                assert torch.equal(Z.view(torch.int32), again.view(torch.int32)), (form, D, op)  # two calls; framed strided views
            nan_rows = torch.isnan(fe.forward_edge_messages(X, Fn, *args, op)[0]).cpu().numpy()
            want = np.zeros((N, D), bool)
            want[rows[e]] = True
            assert np.array_equal(nan_rows, want), (form, D, op)
        assert torch.equal(Z, fe.forward_edge_messages(None, F, *args, "copy")[0])  # copy never reads X
    if form != "tiny_segments":  # a row block whose column ids index a taller X
        rp, col = _rect()
        rargs = _prep(fe, dev, rp, col, form, num_columns=3000)
        X, F = _ints(rng, (3000, 22)), _ints(rng, (len(col), 22))
        Z = fe.forward_edge_messages(_t16(X, dev, dtype), _t16(F, dev, dtype), *rargs, "mul")[0]
        assert torch.equal(Z.cpu(), torch.from_numpy(_row_sums(rp, X[col] * F).astype(np.float32)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("op", ["mul", "add_relu"])
def test_edge_message_aggregate16_matches_torch_at_the_rounded_operands(dev, op, directed, dtype):
    """fp64 autograd of the composition that rounds operands and dZ once: out and dX within _close, dF equal after its rounding"""
    _pkg_imports()
    import GNN_model
    args = _args(frontends.get("extension"), dev, "powerlaw" if directed else "sym", "default")
    N, E = args[0].numel() - 1, args[1].numel()
    torch.manual_seed(286)
    X, F = torch.randn(N, 24, device=dev, requires_grad=True), torch.randn(E, 24, device=dev, requires_grad=True)
    out = GNN_model.edge_message_aggregate(X, F, args, op, directed, gather_dtype=dtype)
    X64, F64 = (t.detach().to(dtype).double().requires_grad_(True) for t in (X, F))
    ref = _torch_aggregate(X64, F64, args[0], args[1], op)
    dY = torch.randn_like(out)
    out.backward(dY)
    ref.backward(dY.to(dtype).double())
    assert out.dtype == X.grad.dtype == F.grad.dtype == torch.float32 and _close(out, ref) and _close(X.grad, X64.grad)
    assert _same_bits(F.grad.to(dtype), F64.grad.to(dtype)) and torch.equal(F.grad, F.grad.to(dtype).float())


def test_gineconv_in_bf16(dev):
    """against the same layer composed in torch with the same roundings (X, edge_attr, W_e, W, F and the combined input once each).
    The rule of the 16-bit GENConv / PNAConv tests as it stands: beyond one bf16 rounding of the output, 4 x the fp32 torch
    composition's error against fp64 + 1e-6 max|ref|"""
    _pkg_imports()
    import GNN_model
    bf16 = torch.bfloat16
    args = _args(frontends.get("extension"), dev, "sym", "default")
    N, E = args[0].numel() - 1, args[1].numel()
    torch.manual_seed(287)
    conv = GNN_model.GINEConv(24, 16, 5, eps=0.25, train_eps=True, activation_dtype=bf16).to(dev)
    X, A = torch.randn(N, 24, device=dev, requires_grad=True), torch.randn(E, 5, device=dev, requires_grad=True)
    out = conv(X, *args, None, A)
    out.float().sum().backward()
    for v, dtype, shape in ((out, bf16, (N, 16)), (X.grad, torch.float32, (N, 24)), (A.grad, torch.float32, (E, 5)),
                            (conv.weights.grad, torch.float32, (24, 16)), (conv.weights_edge.grad, torch.float32, (5, 24)),
                            (conv.eps.grad, torch.float32, ())):
        assert v.dtype == dtype and v.shape == shape and bool(torch.isfinite(v).all())
    res = {}
    for dt in (torch.float64, torch.float32):
        X16, F16 = X.detach().to(bf16).to(dt), (A.detach().to(bf16).to(dt) @ conv.weights_edge.detach().to(bf16).to(dt)).to(bf16).to(dt)
        S = (1 + conv.eps.detach().to(dt)) * X16 + _torch_aggregate(X16, F16, args[0], args[1], "add_relu")
        res[dt] = S.to(bf16).to(dt) @ conv.weights.detach().to(bf16).to(dt)
    ref = res[torch.float64]
    yard, err = (res[torch.float32].double() - ref).abs().max(), ((out.detach().double() - ref).abs() - 2.0 ** -8 * ref.abs()).max()
    bound = 4.0 * float(yard) + 1e-6 * float(ref.abs().max())
    print("GINEConv: library error beyond one rounding %.3e, fp32 torch error %.3e, bound %.3e" % (float(err), float(yard), bound))
    assert float(err) <= bound, (float(err), float(yard), bound)


@pytest.mark.parametrize("fe_name", ["ctypes", "extension"])
def test_refusals(dev, fe_name):
    fe = frontends.get(fe_name)
    args = _args(fe, dev, "molecule", "default")
    N, E = args[0].numel() - 1, args[1].numel()
    X, F = torch.randn(N, 9, device=dev).half(), torch.randn(E, 9, device=dev).half()
    for cols in (5, 2):  # an odd width, D = 2
        x, f = X[:, :cols].contiguous(), F[:, :cols].contiguous()
        for call in (lambda: fe.forward_edge_messages(x, f, *args, "mul"), lambda: fe.edge_messages_grad(x, x, None, args[0], args[1], "mul")):
            with pytest.raises(RuntimeError, match="even width"):
                call()
    x8, f8 = X[:, :8].contiguous(), F[:, :8].contiguous()
    for bad in ((x8.float(), f8), (x8, f8.bfloat16()), (X[:, :8], f8)):  # mixed dtypes; an odd row stride
        with pytest.raises(RuntimeError):
            fe.forward_edge_messages(*bad, *args, "add_relu")
    with pytest.raises(RuntimeError, match="dtype"):
        fe.edge_messages_grad(x8, x8.float(), None, args[0], args[1], "mul")
