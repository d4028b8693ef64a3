"""Edge-feature messages (hcspmm_forward_edge_messages), their gradients (hcspmm_edge_messages_grad; dX through A^T) and the
layers built on them (edge_message_aggregate, GINEConv, --model gine), on an MI355X through both Python front-ends.

The contract (include/hcspmm.h): Z[r][d] = sum over the entries e of row r of m(X[col(e)][d], F[fi(e)][d]) for the ops mul /
add_relu / copy, summed in hcspmm_forward_weighted's order on every plan form, without atomics.  Integer data makes every sum
exact in any order (checked against int64 numpy on ALL rows); dyadic data pins the CSR order of the unsplit rows; normal data
stays within the rounding bound of the number of additions.  References are numpy, computed here.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import frontends
from hcspmm import graphs
from test_extremum_gpu import KINDS, PLANS, WIDTHS, _csr, _pkg_imports, _prepare, _setup, _symmetric

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hc-spmm_amd")
OPS = ("mul", "add_relu", "copy")


@pytest.fixture(scope="module", params=["ctypes", "extension"])
def fe(request):
    return frontends.get(request.param)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def _row_sums(rp, M):
    """sum of the rows of M [E, D] over each CSR row, in M's dtype (int64: exact)"""
    out = np.zeros((len(rp) - 1, M.shape[1]), M.dtype)
    nonempty = np.diff(rp) > 0
    if nonempty.any():
        out[nonempty] = np.add.reduceat(M, rp[:-1][nonempty], axis=0)
    return out


def _messages(op, XC, FE):
    """the per-entry messages, XC = X[col], FE = F[fi], in their dtype"""
    if op == "mul":
        return XC * FE
    if op == "add_relu":
        return np.maximum(XC + FE, 0)
    return FE


def _ints(rng, shape):
    return rng.integers(-8, 9, shape)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _short(rng, shape, bits):
    """test_weighted_gpu._short: at most `bits` significant bits, exponents in a narrow range"""
    m = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), shape)
    return np.ldexp(m.astype(np.float64), rng.integers(-bits - 2, -bits + 3, shape)).astype(np.float32)


# ------------------------------------------------------------------------------------------- 1. exact on every path
@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_integer_sums_are_exact_on_every_row(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    rp, col, N, E = g["rp"], g["col"], g["N"], g["E"]
    assert int(np.diff(rp).max()) * 64 < 2 ** 24  # |m| <= 64: every partial sum is an integer fp32 holds, in any order
    rng = np.random.default_rng(141)
    perm = rng.permutation(E).astype(np.int32)
    V = max(E // 5, 1)
    many = rng.integers(0, V, E).astype(np.int32)  # many-to-one, f_rows != E
    perm_d, many_d = torch.from_numpy(perm).to(dev), torch.from_numpy(many).to(dev)
    for D in WIDTHS:
        X, F = _ints(rng, (N, D)), _ints(rng, (E, D))
        Xd, Fd, Fs = _t(X, dev), _t(F, dev), _t(F[:V], dev)
        XC = X[col]
        for op in OPS:
            xin = None if op == "copy" and D % 2 else Xd  # copy ignores X, which may be None
            for name, idx_d, FE, Fin in (("direct", None, F, Fd), ("perm", perm_d, F[perm], Fd), ("many", many_d, F[:V][many], Fs)):
                got = fe.forward_edge_messages(xin, Fin, *g["args"], op, idx_d)[0]
                want = _row_sums(rp, _messages(op, XC, FE))
                assert got.shape == (N, D) and got.dtype == torch.float32
                assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32))), (kind, form, D, op, name)


# ------------------------------------------------------------------------------------------- 2. CSR-order bits
@pytest.mark.parametrize("form", ["sparse", "dense", "panel32", "plan_free"])  # the forms without column slices
@pytest.mark.parametrize("kind", KINDS)
def test_unsplit_rows_have_the_bits_of_the_csr_recurrence(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    rng = np.random.default_rng(142)
    rp, col, N, E = g["rp"], g["col"], g["N"], g["E"]
    deg = np.diff(rp)
    for D in (4, 32, 128):
        X, F = _short(rng, (N, D), 12), _short(rng, (E, D), 8)
        thr = fe.wide_threshold(g["args"][6], D) if PLANS[form].get("plan", True) else 64
        ordered = deg <= min(thr, 256)  # not wide (whole-wave tree) and not split (fix-up)
        for op in OPS:
            got = fe.forward_edge_messages(_t(X, dev), _t(F, dev), *g["args"], op)[0].cpu().numpy()
            want = np.zeros((N, D), np.float32)
            for k in range(int(deg.max())):  # the sequential fp32 recurrence, one CSR position at a time
                r = np.nonzero(deg > k)[0]
                e = rp[r] + k
                if op == "mul":  # products exact (8 x 12 bits): fmaf rounds once, as this sum does
                    want[r] = (want[r] + F[e] * X[col[e]]).astype(np.float32)
                elif op == "add_relu":
                    t = (X[col[e]] + F[e]).astype(np.float32)
                    want[r] = (want[r] + np.where(t < 0, np.float32(0), t)).astype(np.float32)
                else:
                    want[r] = (want[r] + F[e]).astype(np.float32)
            assert np.array_equal(got[ordered].view(np.int32), want[ordered].view(np.int32)), (kind, form, D, op)


# ------------------------------------------------------------------------------------------- 3. rounding bound
@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_normal_data_within_the_rounding_bound(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    rng = np.random.default_rng(143)
    rp, col, N, E = g["rp"], g["col"], g["N"], g["E"]
    deg = np.diff(rp).astype(np.float64)[:, None]
    u = 2.0 ** -24
    for D in (3, 32, 64):
        X = rng.standard_normal((N, D)).astype(np.float32)
        F = rng.standard_normal((E, D)).astype(np.float32)
        XC, F64 = X[col].astype(np.float64), F.astype(np.float64)
        for op in OPS:
            got = fe.forward_edge_messages(_t(X, dev), _t(F, dev), *g["args"], op)[0].cpu().numpy().astype(np.float64)
            exact = _row_sums(rp, _messages(op, XC, F64))
            k = deg + 2 if op == "add_relu" else deg  # add_relu: the entry's own add, then the sum
            scale = _row_sums(rp, np.abs(XC * F64 if op == "mul" else XC + F64 if op == "add_relu" else F64))
            err = np.abs(got - exact)
            bound = k * u / (1 - k * u) * scale
            print(kind, form, D, op, "max err / bound", float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (kind, form, D, op)


# ------------------------------------------------------------------------------------------- 4. edge cases
def test_rows_without_entries_give_plus_zero(fe, dev):
    for form in ("default", "plan_free"):
        g = _setup(fe, dev, "powerlaw", form)
        empty = np.diff(g["rp"]) == 0
        assert empty.sum() == 7
        for op in OPS:
            Z = fe.forward_edge_messages(torch.full((g["N"], 22), -1.0, device=dev), torch.full((g["E"], 22), -1.0, device=dev),
                                         *g["args"], op)[0]
            assert (Z.cpu().numpy()[empty].view(np.int32) == 0).all(), (form, op)


@pytest.mark.parametrize("form", ["default", "plan_free"])
def test_graph_without_entries(fe, dev, form):
    rp, col = np.zeros(41, np.int32), np.zeros(0, np.int32)
    g = _prepare(fe, dev, rp, col, form)
    for op in OPS:
        Z = fe.forward_edge_messages(torch.ones(40, 8, device=dev), torch.zeros(0, 8, device=dev), *g["args"], op)[0]
        assert Z.shape == (40, 8) and (Z.cpu().numpy().view(np.int32) == 0).all(), (form, op)
        gF = fe.edge_messages_grad(torch.ones(40, 8, device=dev), torch.ones(40, 8, device=dev), torch.zeros(0, 8, device=dev),
                                   g["args"][0], g["args"][1], op)
        assert gF.shape == (0, 8)


@pytest.mark.parametrize("form", ["default", "slices", "plan_free"])
def test_rectangular_block_and_strided_views(fe, dev, form):
    """a row block whose column ids index a taller X; X and F read through column-slice views of wider matrices"""
    rp_full, col_full = graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    n = 1200
    rp, col = rp_full[:n + 1].copy(), col_full[:rp_full[n]].copy()
    g = _prepare(fe, dev, rp, col, form, num_columns=3000)
    rng = np.random.default_rng(144)
    for D in (3, 22, 64):
        X, F = _ints(rng, (3000, D)), _ints(rng, (len(col), D))
        wx = torch.zeros(3000, D + 13, device=dev)
        wf = torch.zeros(len(col), D + 7, device=dev)
        wx[:, 5:5 + D], wf[:, 3:3 + D] = _t(X, dev), _t(F, dev)
        for op in OPS:
            Z = fe.forward_edge_messages(wx[:, 5:5 + D], wf[:, 3:3 + D], *g["args"], op)[0]
            want = _row_sums(rp, _messages(op, X[col], F))
            assert Z.shape == (n, D) and torch.equal(Z.cpu(), torch.from_numpy(want.astype(np.float32))), (form, D, op)


def test_strided_output_through_the_c_abi(dev):
    """Z with a row stride wider than D: the rows land in the view, the columns beside it stay untouched"""
    import hcspmm
    from hcspmm import capi
    fe = frontends.get("ctypes")
    g = _setup(fe, dev, "powerlaw", "default")
    rp_d, col_d, bp, e2c, e2r, ht, plan, _ = g["args"]
    rng = np.random.default_rng(145)
    D, ldz = 22, 40
    X, F = _ints(rng, (g["N"], D)), _ints(rng, (g["E"], D))
    Xd, Fd = _t(X, dev), _t(F, dev)
    out = torch.full((g["N"], ldz), 7.0, device=dev)
    h = hcspmm.plan_header(plan)
    ws_bytes = int(capi.lib().hcspmm_workspace_bytes(ctypes.byref(h), D))
    ws = torch.empty(max(ws_bytes // 4, 1), device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = capi.lib().hcspmm_forward_edge_messages(p(Xd), g["N"], D, p(Fd), g["E"], D, None, 1, ctypes.c_void_p(out.data_ptr() + 4 * 9),
                                                 ldz, p(rp_d), p(col_d), p(bp), p(e2c), p(e2r), p(ht), p(plan), ctypes.byref(h), g["N"],
                                                 g["E"], D, p(ws), ws_bytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    want = _row_sums(g["rp"], _messages("add_relu", X[g["col"]], F)).astype(np.float32)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, 9:9 + D], want)
    assert (got[:, :9] == 7).all() and (got[:, 9 + D:] == 7).all()


@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_a_nan_in_one_f_row_reaches_exactly_its_row(fe, dev, form):
    g = _setup(fe, dev, "powerlaw", form)
    rng = np.random.default_rng(146)
    rows = _rows_of(g["rp"])
    hub = int(np.argmax(np.diff(g["rp"])))
    for e in (0, int(g["rp"][hub]) + 300, g["E"] - 1):  # a short row, the middle of the hub, the last entry
        for D in (3, 64):
            X, F = _ints(rng, (g["N"], D)).astype(np.float32), _ints(rng, (g["E"], D)).astype(np.float32)
            F[e] = np.nan
            for op in ("add_relu", "mul"):
                Z = fe.forward_edge_messages(_t(X, dev), _t(F, dev), *g["args"], op)[0].cpu().numpy()
                want = np.zeros((g["N"], D), bool)
                want[rows[e]] = True
                assert np.array_equal(np.isnan(Z), want), (form, e, D, op)


def test_two_calls_give_the_same_bits_and_f_is_read_on_every_call(fe, dev):
    for form in ("default", "slices", "tiny_segments"):
        g = _setup(fe, dev, "powerlaw", form)
        X, F = torch.randn(g["N"], 64, device=dev), torch.randn(g["E"], 64, device=dev)
        for op in OPS:
            a = fe.forward_edge_messages(X, F, *g["args"], op)[0]
            b = fe.forward_edge_messages(X, F, *g["args"], op)[0]
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (form, op)
            F2 = F.clone()
            c = fe.forward_edge_messages(X, F2, *g["args"], op)[0]
            F2.mul_(2.0)  # in place, no preprocessing again: the same tensor, new values
            d = fe.forward_edge_messages(X, F2, *g["args"], op)[0]
            assert torch.equal(a, c) and not torch.equal(c, d), (form, op)
            if op != "add_relu":  # linear in F: exactly twice
                assert torch.equal(d, 2.0 * c), (form, op)


# ------------------------------------------------------------------------------------------- 5. gradient with respect to F
def _grad_f(op, G, X, F, rows, col):
    """the header's formulas in fp32 (the product of a zero and a negative number is -0, as on the device)"""
    G, X, F = G.astype(np.float32), X.astype(np.float32), F.astype(np.float32)
    if op == "mul":
        return G[rows] * X[col]
    if op == "add_relu":
        return np.where(X[col] + F > 0, G[rows], np.float32(0))
    return G[rows]


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_with_respect_to_f(fe, dev, kind):
    g = _setup(fe, dev, kind, "default")
    rng = np.random.default_rng(147)
    rows, col, rp_d, col_d = _rows_of(g["rp"]), g["col"], g["args"][0], g["args"][1]
    for D in (3, 4, 32, 128):
        G, X, F = _ints(rng, (g["N"], D)), _ints(rng, (g["N"], D)), _ints(rng, (g["E"], D))
        s = X[col] + F
        assert (s == 0).any() and (s < 0).any()  # the kink and the dead side are in the data
        for op in OPS:
            got = fe.edge_messages_grad(_t(G, dev), None if op == "copy" else _t(X, dev), _t(F, dev) if op == "add_relu" else None,
                                        rp_d, col_d, op)
            want = _grad_f(op, G, X, F, rows, col)
            assert got.shape == (g["E"], D) and want.dtype == np.float32
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (kind, D, op)  # bits: the dead side is +0


# ------------------------------------------------------------------------------------------- 6. gradient with respect to X
@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
@pytest.mark.parametrize("route", ["transpose_graph", "permutation"])
def test_gradient_with_respect_to_x_through_a_transposed(fe, dev, route, form):
    rp, col = graphs.uniform_graph(2000, 16000, seed=7)
    if route == "permutation":
        rp, col = _symmetric(rp, col)
    g = _prepare(fe, dev, rp, col, form)
    N, E, rows = g["N"], g["E"], _rows_of(rp)
    if route == "permutation":
        gb, index = g, fe.transpose_permutation(g["args"][0], g["args"][1]).to(torch.int32)
    else:
        assert not np.array_equal(_symmetric(rp, col)[1], col)  # directed
        rp_t, col_t, eid_t = fe.transpose_graph(g["args"][0], g["args"][1])
        gb, index = _prepare(fe, dev, rp_t.cpu().numpy(), col_t.cpu().numpy(), form), eid_t
    rng = np.random.default_rng(148)
    for D in (3, 32, 128):
        G, X, F = _ints(rng, (N, D)), _ints(rng, (N, D)), _ints(rng, (E, D))
        Gd, Xd, Fd = _t(G, dev), _t(X, dev), _t(F, dev)
        for op in ("mul", "add_relu"):
            want = np.zeros((N, D), np.int64)
            np.add.at(want, col, G[rows] * F if op == "mul" else np.where(X[col] + F > 0, G[rows], 0))
            if op == "mul":
                got = fe.forward_edge_messages(Gd, Fd, *gb["args"], "mul", index)[0]
            else:
                gF = fe.edge_messages_grad(Gd, Xd, Fd, g["args"][0], g["args"][1], "add_relu")
                got = fe.forward_edge_messages(None, gF, *gb["args"], "copy", index)[0]
            assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32))), (route, form, D, op)


# ------------------------------------------------------------------------------------------- 7. autograd and layer
def _close(got, want):
    want = want.detach().to(torch.float32)
    return torch.allclose(got, want, rtol=1e-4, atol=1e-4 * want.abs().max().item())  # test_weighted_gpu.py's layer tolerance


def _torch_aggregate(X, F, rp, col, op):
    """the same sum in torch autograd (float64): gather, elementwise op, index_add"""
    N = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(N, device=F.device), (rp[1:] - rp[:-1]).long())
    xc = X.index_select(0, col.long())
    m = xc * F if op == "mul" else torch.relu(xc + F)
    return torch.zeros(N, F.size(1), dtype=F.dtype, device=F.device).index_add(0, rows, m)


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("op", ["mul", "add_relu"])
@pytest.mark.parametrize("kind", ["powerlaw", "molecule", "uniform"])
def test_edge_message_aggregate_matches_torch_autograd(dev, kind, op, directed):
    _pkg_imports()
    import GNN_model
    g = _setup(frontends.get("extension"), dev, kind, "default", sym=not directed)
    rp_d, col_d = g["args"][0], g["args"][1]
    torch.manual_seed(149)
    X = torch.randn(g["N"], 24, device=dev, requires_grad=True)
    F = torch.randn(g["E"], 24, device=dev, requires_grad=True)
    out = GNN_model.edge_message_aggregate(X, F, g["args"], op, directed)
    X64, F64 = X.detach().double().requires_grad_(True), F.detach().double().requires_grad_(True)
    ref = _torch_aggregate(X64, F64, rp_d, col_d, op)
    assert _close(out, ref), (kind, op, directed)
    dY = torch.randn_like(out)
    out.backward(dY)
    ref.backward(dY.double())
    assert _close(X.grad, X64.grad) and _close(F.grad, F64.grad), (kind, op, directed)
    # needs_input_grad is honoured: a gradient nobody asked for is not computed
    Xn = X.detach().clone()
    Fr = F.detach().clone().requires_grad_(True)
    GNN_model.edge_message_aggregate(Xn, Fr, g["args"], op, directed).backward(dY)
    assert _close(Fr.grad, F64.grad) and Xn.grad is None


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("train_eps", [False, True])
def test_gineconv_matches_torch_autograd(dev, train_eps, directed):
    _pkg_imports()
    import GNN_model
    g = _setup(frontends.get("extension"), dev, "powerlaw", "default", sym=not directed)
    rp_d, col_d = g["args"][0], g["args"][1]
    torch.manual_seed(150)
    conv = GNN_model.GINEConv(24, 16, 5, eps=0.25, train_eps=train_eps, directed=directed).to(dev)
    X = torch.randn(g["N"], 24, device=dev, requires_grad=True)
    A = torch.randn(g["E"], 5, device=dev, requires_grad=True)
    out = conv(X, *g["args"], None, A)
    X64, A64 = X.detach().double().requires_grad_(True), A.detach().double().requires_grad_(True)
    We, W = conv.weights_edge.detach().double().requires_grad_(True), conv.weights.detach().double().requires_grad_(True)
    eps = conv.eps.detach().double().requires_grad_(True)
    ref = ((1 + eps) * X64 + _torch_aggregate(X64, A64 @ We, rp_d, col_d, "add_relu")) @ W
    assert _close(out, ref)
    dY = torch.randn_like(out)
    out.backward(dY)
    ref.backward(dY.double())
    pairs = [(X.grad, X64.grad), (A.grad, A64.grad), (conv.weights_edge.grad, We.grad), (conv.weights.grad, W.grad)]
    if train_eps:
        pairs.append((conv.eps.grad, eps.grad))
    else:
        assert not conv.eps.requires_grad
    for got, want in pairs:
        assert _close(got, want), (train_eps, directed)


def test_an_asymmetric_pattern_is_refused_before_any_launch(dev):
    _pkg_imports()
    import GNN_model
    g = _setup(frontends.get("extension"), dev, "uniform", "default")
    X, F = torch.randn(g["N"], 8, device=dev), torch.randn(g["E"], 8, device=dev)
    with pytest.raises(RuntimeError, match="symmetric"):
        GNN_model.edge_message_aggregate(X, F, g["args"], "add_relu")
    with pytest.raises(RuntimeError, match="symmetric"):
        GNN_model.GINEConv(8, 4, 8).to(dev)(X, *g["args"], None, F)
    with pytest.raises(ValueError):
        GNN_model.edge_message_aggregate(X, F, g["args"], "max")


# ------------------------------------------------------------------------------------------- 8. driver
@pytest.mark.parametrize("extra", [[], ["--directed"]])
def test_driver_trains_gine(extra, capsys, monkeypatch):
    _pkg_imports()
    monkeypatch.chdir(PKG)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_gine", os.path.join(PKG, "HC-SpMM_main.py"))
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
                    "--epochs", "3", "--model", "gine", "--edge-dim", "8"] + extra)
    assert "Train (ms/epoch):" in capsys.readouterr().out
    print("losses", losses)
    assert len(losses) == 9 + 3 and all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
    assert net.conv1.weights_edge.shape == (8, 16) and net.conv1.directed == bool(extra)
    for name, prm in net.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name


# ------------------------------------------------------------------------------------------- 9. 64-bit addressing
def test_addressing_past_two_to_the_31_elements(dev):
    """E * D > 2^31: F and grad_F rows are addressed in 64 bits.  F is made on the device from a hash of (e, d)."""
    fe = frontends.get("ctypes")
    N, D = 262144, 256
    rp, col = graphs.uniform_graph(N, 8_600_000, seed=151)
    E = len(col)
    assert E * D > 2 ** 31
    g = _prepare(fe, dev, rp, col, "default")
    d_idx = torch.arange(D, device=dev, dtype=torch.int32)[None, :]
    F = torch.empty(E, D, device=dev)
    for e0 in range(0, E, 1 << 20):  # (e * 7 + d * 3) mod 17 - 8, a million rows at a time
        e_idx = torch.arange(e0, min(e0 + (1 << 20), E), device=dev, dtype=torch.int32)[:, None]
        F[e0:e0 + (1 << 20)] = ((e_idx * 7 + d_idx * 3) % 17 - 8).float()

    def f_rows(e):
        return ((e[:, None] * 7 + np.arange(D)[None, :] * 3) % 17 - 8).astype(np.int64)

    rng = np.random.default_rng(152)
    X = _ints(rng, (N, D))
    Xd = _t(X, dev)
    Z = fe.forward_edge_messages(Xd, F, *g["args"], "add_relu")[0]
    sample = np.unique(np.concatenate([rng.integers(0, N, 63), [N - 1]]))
    Zs = Z[torch.from_numpy(sample).to(dev)].cpu().numpy()
    for r, z in zip(sample, Zs):
        e = np.arange(rp[r], rp[r + 1], dtype=np.int64)
        want = np.maximum(X[col[e]] + f_rows(e), 0).sum(0)
        assert np.array_equal(z, want.astype(np.float32)), r
    del Z
    G = _ints(rng, (N, D))
    gF = fe.edge_messages_grad(_t(G, dev), Xd, F, g["args"][0], g["args"][1], "add_relu")
    es = np.unique(np.concatenate([rng.integers(0, E, 63), [E - 1]])).astype(np.int64)
    got = gF[torch.from_numpy(es).to(dev)].cpu().numpy()
    rows = np.searchsorted(rp, es, side="right") - 1
    want = np.where(X[col[es]] + f_rows(es) > 0, G[rows], 0).astype(np.float32)
    assert np.array_equal(got, want)
