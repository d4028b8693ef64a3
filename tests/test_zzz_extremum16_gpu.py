"""Max / min aggregation on fp16 / bf16 features (hcspmm_forward_extremum_typed, spmm_extremum16.hip), its autograd form and the
16-bit SAGEConv, on an MI355X through both front-ends.  A maximum selects, so every check is exact: arg is the sequential-scan
answer on the widened values (test_extremum_gpu.reference), and Z's raw 16-bit patterns are X16[col[arg], d] (+0 where arg is
-1), compared as int16 so that no NaN is converted."""
import numpy as np
import pytest
import torch

import frontends
from hcspmm import graphs
from test_extremum_gpu import (PLANS, _csr, _fn, _graph, _pkg_imports, _prepare, _setup, _symmetric, _tie_features,  # noqa: F401
                               dev, fe, reference, reference_backward)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
_REF = {}  # (graph key, D, reduce) -> (X fp32, arg): _tie_features' values are exact in both formats, so both share them


def _check(fe, dev, g, X16, reduce, want_arg, tag, view=None):
    """Z, arg of both call forms against the oracle; X16: the features on the CPU, view: a device view that holds them"""
    view = X16.to(dev) if view is None else view
    Z, arg = _fn(fe, reduce)(view, *g["args"])
    assert Z.dtype == X16.dtype and Z.shape == want_arg.shape and arg.dtype == torch.int32, tag
    assert np.array_equal(arg.cpu().numpy(), want_arg), tag
    d = np.broadcast_to(np.arange(want_arg.shape[1]), want_arg.shape)
    bits = X16.view(torch.int16).numpy()[g["col"][np.maximum(want_arg, 0)], d]
    want_bits = np.where(want_arg >= 0, bits, 0).astype(np.int16)
    assert np.array_equal(Z.cpu().view(torch.int16).numpy(), want_bits), tag
    Z1 = _fn(fe, reduce)(view, *g["args"], return_arg=False)
    assert len(Z1) == 1 and np.array_equal(Z1[0].cpu().view(torch.int16).numpy(), want_bits), tag


def _tied(key, g, rows, D, reduce, seed):
    if (key, D) not in _REF:
        _REF[(key, D)] = _tie_features(np.random.default_rng(seed + D), rows, D)
    if (key, D, reduce) not in _REF:
        _REF[(key, D, reduce)] = reference(g["rp"], g["col"], _REF[(key, D)], reduce)[1]
    return torch.from_numpy(_REF[(key, D)]), _REF[(key, D, reduce)]


@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", ["powerlaw", "planted", "molecule"])
def test_every_plan_form(fe, dev, kind, form, dtype, reduce):
    """widths: 4 = one 8-byte lane; 6, 22 = moved-back 4-element lanes; 32 = the first 8-element width; 34 = a moved-back 16-byte
    lane; 64; 130 = a panel boundary and a ragged tail; 256"""
    g = _setup(fe, dev, kind, form)
    for D in (4, 6, 22, 32, 34, 64, 130, 256):
        X, want = _tied(kind, g, g["N"], D, reduce, 41)
        _check(fe, dev, g, X.to(dtype), reduce, want, (kind, form, D))


@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "plan_free"])
def test_raw_patterns(fe, dev, form, dtype, reduce):
    """uniformly random 16-bit patterns, the NaN ones replaced: subnormals, +-inf, +-0 and last-bit neighbours"""
    g = _setup(fe, dev, "powerlaw", form)
    for D in (8, 64):
        bits = np.random.default_rng(42 + D).integers(0, 1 << 16, (g["N"], D), dtype=np.uint16)
        X16 = torch.from_numpy(bits.view(np.int16)).view(dtype)
        X16[X16.isnan()] = 1.5
        _check(fe, dev, g, X16, reduce, reference(g["rp"], g["col"], X16.float().numpy(), reduce)[1], (form, D))


@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "tiny_segments", "plan_free"])
def test_empty_rows_duplicate_columns_and_a_split_hub(fe, dev, form, dtype, reduce):
    """test_extremum_gpu.test_empty_rows_and_duplicate_columns' graph: rows without entries give +0 / -1, the first copy of a
    duplicated column wins, row 5 is split into segments"""
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
        X, want = _tied("n700", g, N, D, reduce, 43)
        assert (want[np.diff(rp) == 0] == -1).all()
        _check(fe, dev, g, X.to(dtype), reduce, want, (form, D))


@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["default", "plan_free"])
def test_rectangular_and_strided(fe, dev, form, dtype, reduce):
    """a row block whose column ids index a taller X, itself a column block (2 elements in) of a wider NaN-filled buffer"""
    rp_full, col_full = _graph("powerlaw")
    n = 1200
    rp, col = rp_full[:n + 1].copy(), col_full[:rp_full[n]].copy()
    g = _prepare(fe, dev, rp, col, form, num_columns=3000)
    for D in (22, 64):
        X, want = _tied("rect", g, 3000, D, reduce, 44)
        wide = torch.full((3000, D + 6), float("nan"), dtype=dtype, device=dev)
        wide[:, 2:2 + D] = X.to(dtype).to(dev)
        _check(fe, dev, g, X.to(dtype), reduce, want, (form, D), view=wide[:, 2:2 + D])


def test_arg_is_the_fp32_kernels_on_the_widened_input(fe, dev):
    g = _setup(fe, dev, "powerlaw", "default")
    X16 = _tied("powerlaw", g, g["N"], 64, "max", 41)[0].to(torch.bfloat16).to(dev)
    assert torch.equal(fe.forward_max(X16, *g["args"])[1], fe.forward_max(X16.float(), *g["args"])[1])


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_gradient_is_the_fp32_backward_on_the_saved_arg(dev, dtype, directed):
    _pkg_imports()
    import GNN_model
    g = _setup(frontends.get("extension"), dev, "powerlaw", "default", sym=not directed)
    rng = np.random.default_rng(45)
    X = torch.from_numpy(_tie_features(rng, g["N"], 22)).to(dtype).to(dev).requires_grad_(True)
    G = rng.integers(-8, 9, (g["N"], 22)).astype(np.float32)  # small integers: the fp32 sums are exact, then rounded once
    Z = GNN_model.extremum_aggregate(X, g["args"], "min", directed=directed)
    Z.backward(torch.from_numpy(G).to(dtype).to(dev))
    Z0, arg = GNN_model.HCSPMM.forward_min(X.detach(), *g["args"])
    assert Z.dtype == dtype and torch.equal(Z.detach().view(torch.int16), Z0.view(torch.int16))
    want = torch.from_numpy(reference_backward(g["rp"], g["col"], G, arg.cpu().numpy())).to(dtype)
    assert X.grad.dtype == dtype and torch.equal(X.grad.cpu().view(torch.int16), want.view(torch.int16))


def test_sageconv_bf16_is_the_composition_of_the_public_pieces(dev):
    """4500 nodes: from 4096 rows on _Update16 runs HCSPMM.update, the composition's own product"""
    _pkg_imports()
    import GNN_model
    rp, col = graphs.powerlaw_graph(4500, 40000, seed=8, max_degree_frac=0.2)
    g = _prepare(frontends.get("extension"), dev, *_symmetric(rp, col), "default")
    torch.manual_seed(46)
    conv = GNN_model.SAGEConv(24, 16, aggr="max", activation_dtype=torch.bfloat16).to(dev)
    X = torch.randn(g["N"], 24, device=dev)
    out = conv(X, *g["args"], None)
    X16 = X.to(torch.bfloat16)
    agg = GNN_model.HCSPMM.forward_max(X16, *g["args"])[0]
    want = (GNN_model.HCSPMM.update(X16, conv.weights_root.detach().to(torch.bfloat16))
            + GNN_model.HCSPMM.update(agg, conv.weights_neigh.detach().to(torch.bfloat16)))
    assert out.dtype == torch.bfloat16 and torch.equal(out.view(torch.int16), want.view(torch.int16))
    out.float().sum().backward()
    assert conv.weights_root.grad.dtype == conv.weights_neigh.grad.dtype == torch.float32
    for dims in ((24, 15), (23, 16)):
        with pytest.raises(ValueError, match="even widths"):
            GNN_model.SAGEConv(*dims, aggr="max", activation_dtype=torch.bfloat16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_come_before_a_launch(fe, dev, dtype):
    g = _setup(fe, dev, "molecule", "default")
    buf = torch.zeros(g["N"], 40, dtype=dtype, device=dev)
    odd_stride = torch.zeros(g["N"], 41, dtype=dtype, device=dev)[:, :8]
    for bad in (buf[:, :7], buf[:, :2], odd_stride, buf[:, 1:9]):  # odd D, D = 2, an odd row stride, a base 2 bytes off a dword
        with pytest.raises(RuntimeError, match="16-bit max / min"):
            fe.forward_max(bad, *g["args"])
