"""One-pass sum / sumsq / max / min aggregation on fp16 / bf16 features (hcspmm_forward_multi_typed, spmm_multi16.hip) on an MI355X
through both front-ends.  Integer features are exact in both formats and their sums in any order, so those checks are exact:
the sums against a numpy scan, the args against the sequential-scan oracle (test_extremum_gpu.reference), the extrema as the raw
16-bit patterns X16[col[arg], d] (+0 where arg is -1), compared as int16 so that no NaN is converted."""
import ctypes

import numpy as np
import pytest
import torch

import frontends
from hcspmm import capi, graphs
from test_extremum_gpu import (PLANS, _csr, _graph, _pkg_imports, _prepare, _setup, _symmetric, _tie_features, dev, fe,  # noqa: F401
                               reference)
from test_multi_aggr_gpu import reference_sums

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
_REF = {}  # (graph key, D) -> (X fp32, references): _tie_features' values are exact in both formats, so both share them


def _tied(key, g, rows, D, seed):
    if (key, D) not in _REF:
        X = _tie_features(np.random.default_rng(seed + D), rows, D)
        V = X[g["col"]].astype(np.float64)
        sums = [np.zeros((g["N"], D)), np.zeros((g["N"], D))]
        ne = np.diff(g["rp"]) > 0
        if len(g["col"]):
            with np.errstate(invalid="ignore"):
                sums[0][ne] = np.add.reduceat(V, g["rp"][:-1][ne], axis=0) + 0.0
                sums[1][ne] = np.add.reduceat(V * V, g["rp"][:-1][ne], axis=0) + 0.0
        _REF[(key, D)] = (torch.from_numpy(X), sums, reference(g["rp"], g["col"], X, "max")[1], reference(g["rp"], g["col"], X, "min")[1])
    return _REF[(key, D)]


def _bits(g, X16, arg):
    d = np.broadcast_to(np.arange(arg.shape[1]), arg.shape)
    return np.where(arg >= 0, X16.view(torch.int16).numpy()[g["col"][np.maximum(arg, 0)], d], 0).astype(np.int16)


def _check_extrema(g, X16, out, amax, amin, tag):
    assert out[2].dtype == out[3].dtype == X16.dtype and out[4].dtype == out[5].dtype == torch.int32, tag
    assert np.array_equal(out[4].cpu().numpy(), amax) and np.array_equal(out[5].cpu().numpy(), amin), tag
    assert np.array_equal(out[2].cpu().view(torch.int16).numpy(), _bits(g, X16, amax)), tag
    assert np.array_equal(out[3].cpu().view(torch.int16).numpy(), _bits(g, X16, amin)), tag


def _check(fe, dev, g, X16, ref, tag, view=None):
    _, sums, amax, amin = ref
    out = fe.forward_multi16(X16.to(dev) if view is None else view, *g["args"])
    assert out[0].dtype == out[1].dtype == torch.float32 and out[0].shape == amax.shape, tag
    for k in (0, 1):  # NaN-equal by value: inf - inf and NaN entries give NaN in both
        assert np.array_equal(out[k].cpu().numpy().astype(np.float64), sums[k], equal_nan=True), tag + (k,)
        assert not np.signbit(out[k].cpu().numpy()[np.diff(g["rp"]) == 0]).any(), tag
    _check_extrema(g, X16, out, amax, amin, tag)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", ["powerlaw", "planted", "molecule"])
def test_every_plan_form(fe, dev, kind, form, dtype):
    """widths: 4 = one 8-byte lane; 6, 22 = moved-back 4-column lanes; 32 = the first 8-column width; 34 = a moved-back 16-byte
    lane; 64; 130 = a panel boundary and a ragged tail; 256"""
    g = _setup(fe, dev, kind, form)
    for D in (4, 6, 22, 32, 34, 64, 130, 256):
        ref = _tied(kind, g, g["N"], D, 51)
        _check(fe, dev, g, ref[0].to(dtype), ref, (kind, form, D))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_continuous_data_bounds_determinism_and_the_extremum_launches(fe, dev, form, dtype):
    """section 3.17's bars on the widened values: 1e-5 * sum |x| and 1e-5 * sum x^2 against fp64"""
    g = _setup(fe, dev, "powerlaw", form)
    for D in (22, 64, 130):
        X16 = torch.from_numpy(np.random.default_rng(52 + D).standard_normal((g["N"], D)).astype(np.float32)).to(dtype)
        s, _, ab, sq = reference_sums(g["rp"], g["col"], X16.float().numpy())
        Xd = X16.to(dev)
        out = fe.forward_multi16(Xd, *g["args"])
        es = np.abs(out[0].cpu().numpy() - s) - 1e-5 * ab
        eq = np.abs(out[1].cpu().numpy() - sq) - 1e-5 * sq
        print(form, D, "sum excess", es.max(), "sumsq excess", eq.max())
        assert es.max() <= 0 and eq.max() <= 0, (form, D)
        again = fe.forward_multi16(Xd, *g["args"])
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(out, again)), (form, D)
        for k, f in ((2, fe.forward_max), (3, fe.forward_min)):
            Z, arg = f(Xd, *g["args"])
            assert torch.equal(out[k].view(torch.int16), Z.view(torch.int16)) and torch.equal(out[k + 2], arg), (form, D, k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "plan_free"])
def test_raw_patterns(fe, dev, form, dtype):
    """uniformly random 16-bit patterns, the NaN ones replaced: subnormals, +-inf, +-0 and last-bit neighbours"""
    g = _setup(fe, dev, "powerlaw", form)
    for D in (8, 64):
        bits = np.random.default_rng(53 + D).integers(0, 1 << 16, (g["N"], D), dtype=np.uint16)
        X16 = torch.from_numpy(bits.view(np.int16)).view(dtype)
        X16[X16.isnan()] = 1.5
        X = X16.float().numpy()
        out = fe.forward_multi16(X16.to(dev), *g["args"], aggregates=("max", "min"))
        assert out[0] is None and out[1] is None
        _check_extrema(g, X16, out, reference(g["rp"], g["col"], X, "max")[1], reference(g["rp"], g["col"], X, "min")[1], (form, D))


@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_subsets_and_a_direct_call_into_concatenated_buffers(fe, dev, form):
    g = _setup(fe, dev, "powerlaw", form)
    D = 34
    ref = _tied("powerlaw", g, g["N"], D, 51)
    X16 = ref[0].to(torch.bfloat16)
    Xd = X16.to(dev)
    full = _check(fe, dev, g, X16, ref, (form, "full"))
    for names, ra in ((("sum",), True), (("sumsq", "min"), True), (("max",), False), (("sum", "max", "min"), False)):
        out = fe.forward_multi16(Xd, *g["args"], aggregates=names, return_arg=ra)
        asked = [n in names for n in ("sum", "sumsq", "max", "min")] + [ra and n in names for n in ("max", "min")]
        for k in range(6):  # every dtype compared as bits
            assert (out[k] is not None) == asked[k], (names, k)
            assert out[k] is None or torch.equal(out[k].view(torch.int16), full[k].view(torch.int16)), (names, k)
    if fe.name != "ctypes":
        return
    # one C-ABI call: [sum | sumsq] in one fp32 buffer, [max | min] in one 16-bit buffer, guard columns behind each
    import hcspmm
    S = torch.full((g["N"], 2 * D + 2), float("nan"), device=dev)
    Zx = torch.full((g["N"], 2 * D + 2), float("nan"), dtype=torch.bfloat16, device=dev)
    c = hcspmm._planned_call(g["args"][:6], g["args"][6], D, g["N"], dev, ws_fn=hcspmm._ws_bytes_multi)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    with c:
        rc = capi.lib().hcspmm_forward_multi_typed(p(Xd), g["N"], D, 2, p(S), p(S, 4 * D), 2 * D + 2, p(Zx), p(Zx, 2 * D), 2 * D + 2,
                                                   ctypes.c_void_p(0), ctypes.c_void_p(0), 0, *c.graph, *c.ws)
    assert rc == 0
    torch.cuda.synchronize()
    for k in (0, 1):
        assert np.array_equal(S[:, k * D:(k + 1) * D].cpu().numpy(), full[k].cpu().numpy(), equal_nan=True)
        assert torch.equal(Zx[:, k * D:(k + 1) * D].contiguous().view(torch.int16), full[2 + k].view(torch.int16))
    assert S[:, 2 * D:].isnan().all() and Zx[:, 2 * D:].isnan().all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_empty_rows_duplicate_columns_and_a_split_hub(fe, dev, form, dtype):
    """the n = 700 graph of the existing modules: rows without entries give +0 / -1, the first copy of a duplicated column wins,
    row 5 (600 entries) is split into 7-entry segments"""
    rng = np.random.default_rng(33)
    N = 700
    deg = rng.integers(0, 12, N)
    deg[::7] = 0
    deg[5] = 600
    rows = np.repeat(np.arange(N), deg)
    cols = rng.integers(0, N, rows.size)
    cols[::5] = cols[np.maximum(np.arange(0, rows.size, 5) - 1, 0)]
    rp, col = _csr(rows, cols, N)
    g = _prepare(fe, dev, rp, col, form)
    for D in (4, 34):
        ref = _tied("n700", g, N, D, 54)
        assert (ref[2][np.diff(rp) == 0] == -1).all()
        _check(fe, dev, g, ref[0].to(dtype), ref, (form, D))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "plan_free"])
def test_rectangular_and_strided(fe, dev, form, dtype):
    """a row block whose column ids index a taller X, itself a column block (2 elements in) of a wider NaN-filled buffer"""
    rp_full, col_full = _graph("powerlaw")
    n = 1200
    rp, col = rp_full[:n + 1].copy(), col_full[:rp_full[n]].copy()
    g = _prepare(fe, dev, rp, col, form, num_columns=3000)
    for D in (22, 64):
        ref = _tied("rect", g, 3000, D, 55)
        wide = torch.full((3000, D + 6), float("nan"), dtype=dtype, device=dev)
        wide[:, 2:2 + D] = ref[0].to(dtype).to(dev)
        _check(fe, dev, g, ref[0].to(dtype), ref, (form, D), view=wide[:, 2:2 + D])


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_gradient_is_the_fp32_gradient_rounded_once(dev, dtype, directed):
    _pkg_imports()
    import GNN_model
    g = _setup(frontends.get("extension"), dev, "powerlaw", "default", sym=not directed)
    rng = np.random.default_rng(56)
    X16 = torch.from_numpy(_tie_features(rng, g["N"], 22, specials=False)).to(dtype).to(dev)
    G = [torch.from_numpy(rng.integers(-8, 9, (g["N"], 22)).astype(np.float32)).to(dev) for _ in range(4)]  # small integers
    grads = []
    for X in (X16.requires_grad_(True), X16.detach().float().requires_grad_(True)):  # MultiAggregate16, then the fp32 MultiAggregate
        Z = GNN_model.multi_aggregate(X, g["args"], directed=directed)
        assert [z.dtype for z in Z] == [torch.float32, torch.float32, X.dtype, X.dtype]
        torch.autograd.backward(Z, [gz.to(z.dtype) for gz, z in zip(G, Z)])
        grads.append(X.grad)
    assert grads[0].dtype == dtype and torch.equal(grads[0].view(torch.int16), grads[1].to(dtype).view(torch.int16))


def test_pnaconv_bf16_is_the_composition_of_the_public_pieces(dev):
    """4500 nodes: from 4096 rows on _Update16 runs HCSPMM.update, the composition's own product"""
    _pkg_imports()
    import GNN_model
    H, bf16 = GNN_model.HCSPMM, torch.bfloat16
    rp, col = graphs.powerlaw_graph(4500, 40000, seed=8, max_degree_frac=0.2)
    g = _prepare(frontends.get("extension"), dev, *_symmetric(rp, col), "default")
    torch.manual_seed(57)
    conv = GNN_model.PNAConv(24, 16, activation_dtype=bf16).to(dev)
    X = torch.randn(g["N"], 24, device=dev)
    out = conv(X, *g["args"], None)
    X16 = X.to(bf16)
    z = H.forward_multi16(X16, *g["args"], return_arg=False)
    S16 = conv.scaled_aggregates(z[0], z[1], z[2].float(), z[3].float(), g["args"][0]).to(bf16)  # the fp32 post-processing
    want = H.update(X16, conv.weights_root.detach().to(bf16)) + H.update(S16, conv.weights_neigh.detach().to(bf16))
    assert out.dtype == bf16 and torch.equal(out.view(torch.int16), want.view(torch.int16))
    out.float().sum().backward()
    assert conv.weights_root.grad.dtype == conv.weights_neigh.grad.dtype == torch.float32
    for dims in ((24, 15), (23, 16)):
        with pytest.raises(ValueError, match="even widths"):
            GNN_model.PNAConv(*dims, activation_dtype=bf16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_come_before_a_launch(fe, dev, dtype):
    g = _setup(fe, dev, "molecule", "default")
    buf = torch.zeros(g["N"], 40, dtype=dtype, device=dev)
    odd_stride = torch.zeros(g["N"], 41, dtype=dtype, device=dev)[:, :8]
    # odd D, D = 2, an odd row stride, a base 2 bytes off a dword, fp32 features
    for bad in (buf[:, :7], buf[:, :2], odd_stride, buf[:, 1:9], buf[:, :8].float()):
        with pytest.raises(RuntimeError, match="16-bit multi aggregation"):
            fe.forward_multi16(bad, *g["args"])
