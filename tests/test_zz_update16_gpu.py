"""The update GEMM and its weight gradient on fp16 / bf16 operands (hcspmm_dense_update_typed, hcspmm_weight_grad_typed,
update_kernels_h16.hip) and the activation_dtype layers built on them, on an MI355X.  Integer operands make every fp32 sum exact in
any order, so the layout tests ask for equality; random operands are held to 4 x the error of torch's fp32 product of the widened
operands + 1e-6 max|ref| against fp64 (test_multi_aggr_gpu.py's criterion for combined sums)."""
import os
import sys

import pytest
import torch

import frontends

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float16, torch.bfloat16]
BOTH = ["ctypes", "extension"]
# masked dword rows (2, 22), one k-step and several, a padded last k-step (8, 40, 136), padded and full column tiles, T = 1 ... 8
SHAPES = [(2, 1), (8, 16), (22, 22), (32, 32), (40, 47), (96, 64), (136, 128), (256, 33)]


def _ints(shape, lim, seed):
    return torch.randint(-lim, lim + 1, shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("fe", BOTH)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,H", SHAPES)
@pytest.mark.parametrize("N", [1, 15, 17, 65, 4100])  # a partial tile, more than one tile per workgroup, more than one workgroup
def test_update_of_integers_is_exact(fe, dtype, N, D, H):
    fe = frontends.get(fe)
    for lim, out_dtype in ((4, torch.float32), (1 if dtype == torch.bfloat16 else 4, dtype)):  # bf16 holds integers up to 256
        X, W = _ints((N, D), lim, 31 * N + D), _ints((D, H), lim, 17 * D + H)
        ref = (X.double() @ W.double()).to(out_dtype)
        x16, w16 = X.to(dtype), W.to(dtype)
        for form, w in (("contiguous", w16), ("transposed view", w16.t().contiguous().t()), ("fp32", W.float())):
            out = fe.update(x16, w, out_dtype) if out_dtype != dtype else fe.update(x16, w)
            assert out.dtype == out_dtype and torch.equal(out, ref), (form, out_dtype)


# (70 000, 96, 32): 4375 row tiles on a grid capped at 512 workgroups x 8 waves = 4096 waves, so waves take a second tile in their
# stride loop; (300, 602, 64): masked dword rows over five chunks of k-steps, the staged weights above 64 KiB
@pytest.mark.parametrize("fe", BOTH)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,D,H", [(4100, 32, 32), (4100, 136, 47), (70000, 96, 32), (300, 602, 64)])
def test_update_of_random_operands(fe, dtype, N, D, H):
    fe = frontends.get(fe)
    g = torch.Generator().manual_seed(N + D + H)
    a16, w32 = torch.randn(N, D, generator=g).to(DEV).to(dtype), torch.randn(D, H, generator=g).to(DEV)
    a, w = a16.float(), w32.to(dtype).float()
    ref = a.double() @ w.double()
    yard = (a @ w - ref).abs().max().item()
    out32 = fe.update(a16, w32.to(dtype), torch.float32)
    err = (out32 - ref).abs().max().item()
    print("update", dtype, (N, D, H), "err %.3g yard %.3g" % (err, yard))
    assert err <= 4 * yard + 1e-6 * ref.abs().max().item()
    assert torch.equal(fe.update(a16, w32, torch.float32), out32)  # fp32 weights are rounded as they are staged
    assert torch.equal(fe.update(a16, w32).view(torch.int16), out32.to(dtype).view(torch.int16))


@pytest.mark.parametrize("fe", BOTH)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("out_dtype", [None, torch.float32])
@pytest.mark.parametrize("D,H,off", [(40, 47, 3), (22, 21, 1), (32, 32, 2)])  # (32, 32, 2): packed dwords into a framed block
def test_update_on_framed_views(fe, dtype, out_dtype, D, H, off):
    fe, N = frontends.get(fe), 65
    X, W = _ints((N, D), 4, 5).to(dtype), _ints((D, H), 4, 6).to(dtype)
    frame_in = torch.full((N, D + 10), float("nan"), dtype=dtype, device=DEV)
    frame_in[:, 4:4 + D] = X
    frame_out = torch.full((N, H + 2 * off + H % 2), 777.0, dtype=out_dtype or dtype, device=DEV)
    out = fe.update(frame_in[:, 4:4 + D], W, out_dtype, out=frame_out[:, off:off + H])
    assert out.data_ptr() == frame_out[:, off:].data_ptr() and torch.equal(out, fe.update(X, W, out_dtype))
    assert not torch.isnan(out).any() and (frame_out[:, :off] == 777).all() and (frame_out[:, off + H:] == 777).all()


def test_update_serves_what_it_says():
    fe, x = frontends.get("ctypes"), torch.zeros(64, 32, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(32, 16, dtype=torch.bfloat16, device=DEV)
    for X, W, od in ((x[:, :31], w[:31], None), (x, w.half(), None), (x, w, torch.float16), (x, w.double(), None),
                     (x[:, 1:31], w[:30], None), (x, torch.zeros(32, 129, dtype=torch.bfloat16, device=DEV), None)):
        assert fe.update(X, W, od) is None and frontends.get("extension").update(X, W, od) is None


@pytest.mark.parametrize("fe", BOTH)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,H", [(2, 2), (16, 16), (22, 40), (128, 32), (96, 64)])
@pytest.mark.parametrize("N", [1, 31, 33, 4100, 70000])  # 70 000 * 4 < 2^24: exact in fp32
def test_weight_grad_of_integers_is_exact(fe, dtype, N, D, H):
    A, B = _ints((N, D), 2, N + D), _ints((N, H), 2, N + H + 1)
    dW = frontends.get(fe).weight_grad(A.to(dtype), B.to(dtype))
    assert dW.dtype == torch.float32 and torch.equal(dW, (A.double().t() @ B.double()).float())


@pytest.mark.parametrize("fe", BOTH)
@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_grad_random_strided_and_refused(fe, dtype):
    fe, (N, D, H) = frontends.get(fe), (70000, 96, 32)
    g = torch.Generator().manual_seed(9)
    A, B = torch.randn(N, D, generator=g).to(DEV).to(dtype), torch.randn(N, H, generator=g).to(DEV).to(dtype)
    ref = A.double().t() @ B.double()
    yard = (A.float().t() @ B.float() - ref).abs().max().item()
    dW = fe.weight_grad(A, B)
    err = (dW - ref).abs().max().item()
    print("weight_grad", dtype, "err %.3g yard %.3g" % (err, yard))
    assert err <= 4 * yard + 1e-6 * ref.abs().max().item()
    assert torch.equal(dW, fe.weight_grad(A, B))  # deterministic
    frame_a, frame_b = (torch.full((N, w), float("nan"), dtype=dtype, device=DEV) for w in (D + 6, H + 10))
    frame_a[:, 2:2 + D], frame_b[:, 6:6 + H] = A, B
    assert torch.equal(fe.weight_grad(frame_a[:, 2:2 + D], frame_b[:, 6:6 + H]), dW)
    for a, b in ((A.repeat(1, 2)[:, :144], B), (A[:, :95], B), (A, B[:, 1:]), (A, B.float())):
        assert fe.weight_grad(a, b) is None


def _layer_setup(model, directed=False, n=300):
    for p in (os.path.join(frontends.ROOT, "hc-spmm_amd"), frontends.EXT_DIR):
        if p not in sys.path:
            sys.path.insert(0, p)
    import GNN_model
    import HCSPMM
    from hcspmm import graphs
    rp, col = graphs.uniform_graph(n, 10 * n, seed=3) if directed else graphs.powerlaw_graph(n, 10 * n, seed=21, max_degree_frac=0.2)
    rp_d, col_d = torch.from_numpy(rp).to(DEV), torch.from_numpy(col).to(DEV)
    args = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, n, len(col), (n + 15) // 16, -1))
    ew = HCSPMM.edge_norm(rp_d, col_d, "sym")
    A = torch.zeros(n, n, dtype=torch.float64, device=DEV)
    A[torch.repeat_interleave(torch.arange(n, device=DEV), (rp_d[1:] - rp_d[:-1]).long()), col_d.long()] = ew.double()
    return GNN_model, (GNN_model.GCNConv if model == "gcn" else GNN_model.GINConv), args, ew, A


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("model", ["gcn", "gin"])
def test_layer_on_bf16_activations(model, directed):
    """Forward, dX and dW against the same layer in fp64 on the widened operands.  The layer rounds to bf16 (u = 2^-8, nearest) after
    each of its two products per pass and nowhere else, so an output's error is at most u x (the first product's magnitude carried
    through the second product's absolute values + the output's own magnitude), plus fp32 accumulation (1e-6 of the largest
    entry); dW is rounded only in its operand.  Worst error / bound on an MI355X: see DESIGN.md section 3.4b."""
    GNN_model, cls, args, ew, A = _layer_setup(model, directed)
    n, D, H, u = A.size(0), 24, 16, 2.0 ** -8
    conv = cls(D, H, 0, directed=directed, activation_dtype=torch.bfloat16).to(DEV)
    g = torch.Generator().manual_seed(3)
    X = torch.randn(n, D, generator=g).to(DEV).bfloat16().requires_grad_(True)
    G = torch.randn(n, H, generator=g).to(DEV).bfloat16()
    Y = conv(X, *args, None, edge_weight=ew)
    Y.backward(G)
    x, w, gg = X.detach().double(), conv.weights.detach().bfloat16().double(), G.double()
    if model == "gcn":  # Y = A (X W)
        h = x @ w
        y, by = A @ h, A.abs() @ h.abs()
        dh = A.t() @ gg
        dx, bdx, dw, bdw = dh @ w.t(), dh.abs() @ w.abs().t(), x.t() @ dh, x.abs().t() @ dh.abs()
    else:  # Y = (A X) W
        z = A @ x
        y, by = z @ w, z.abs() @ w.abs()
        dz = gg @ w.t()
        dx, bdx, dw, bdw = A.t() @ dz, A.abs().t() @ dz.abs(), z.t() @ gg, z.abs().t() @ gg.abs()
    for name, got, ref, first in (("Y", Y, y, by), ("dX", X.grad, dx, bdx), ("dW", conv.weights.grad, dw, bdw)):
        bound = u * (first + (0 if name == "dW" else ref.abs())) + 1e-6 * ref.abs().max()
        worst = ((got.detach().double() - ref).abs() / bound).max().item()
        print("layer", model, "directed" if directed else "symmetric", name, "worst error / bound %.3f" % worst)
        assert worst <= 1.0, (name, worst)
    assert Y.dtype == torch.bfloat16 and conv.weights.grad.dtype == torch.float32


def test_layer_refusals_and_the_fp32_path():
    GNN_model, cls, args, ew, A = _layer_setup("gcn")
    X = torch.randn(A.size(0), 24, device=DEV)
    conv = cls(24, 16, 0, activation_dtype=torch.bfloat16).to(DEV)
    with pytest.raises(ValueError, match="edge_weight"):
        conv(X, *args, None)
    conv.feature_storage = "fp8"
    with pytest.raises(ValueError, match="fp8"):
        conv(X, *args, None, edge_weight=ew)
    with pytest.raises(ValueError, match="even widths"):
        cls(24, 15, 0, activation_dtype=torch.float16).to(DEV)(X, *args, None, edge_weight=ew)
    plain = cls(24, 16, 0).to(DEV)
    assert plain.activation_dtype is None
    want = GNN_model.weighted_aggregate(GNN_model._Update.apply(X, plain.weights), ew, args[:8])
    out = plain(X, *args, None, edge_weight=ew)
    assert out.dtype == torch.float32 and torch.equal(out, want)


@pytest.mark.parametrize("D,H", [(24, 16), (136, 16)])  # 136: d_x is wider than 128 and dW has 9 row tiles -- both declined
def test_update16_function_reaches_the_kernels(monkeypatch, D, H):
    """_Update16 at 4100 rows (its kernels' side of the 4096-row threshold) against fp64: Y and dX are rounded once from fp32 sums
    (u |ref| + 1e-6 max|ref|), dW is an fp32 sum of N exact products (N 2^-24 |X|^T |G|); what the kernels decline falls to torch.mm"""
    GNN_model, (N, served) = _layer_setup("gcn")[0], (4100, [])
    for name in ("update", "weight_grad"):
        def spy(*a, _real=getattr(GNN_model.HCSPMM, name), _name=name):
            out = _real(*a)
            served.append((_name, out is not None))
            return out
        monkeypatch.setattr(GNN_model.HCSPMM, name, spy)
    g = torch.Generator().manual_seed(4)
    X = torch.randn(N, D, generator=g).to(DEV).bfloat16().requires_grad_(True)
    W = torch.randn(D, H, generator=g).to(DEV).requires_grad_(True)
    G = torch.randn(N, H, generator=g).to(DEV).bfloat16()
    Y = GNN_model._Update16.apply(X, W)
    Y.backward(G)
    assert served == [("update", True), ("update", D <= 128), ("weight_grad", D <= 128)]
    x, w, gg, u = X.detach().double(), W.detach().bfloat16().double(), G.double(), 2.0 ** -8
    for got, ref, bound in ((Y, x @ w, None), (X.grad, gg @ w.t(), None), (W.grad, x.t() @ gg, N * 2.0 ** -24 * (x.abs().t() @ gg.abs()))):
        bound = u * ref.abs() + 1e-6 * ref.abs().max() if bound is None else bound
        assert ((got.detach().double() - ref).abs() <= bound).all()
    assert Y.dtype == X.grad.dtype == torch.bfloat16 and W.grad.dtype == torch.float32
