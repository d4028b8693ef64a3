"""Layers and driver on a sampled graph (GNN_model.sampled_graph; N = 300, D = 20, fanout 4) on an MI355X: a sample is just
another directed graph, so the directed=True layers are compared with dense float64 autograd on the adjacency rebuilt from
(row_pointers_s, column_index_s) at the bar of tests/test_directed_gpu.py for the same layers,
|got - want| <= 1e-4 * max|want|, forward and every gradient; the sample and its transpose are built while the host paths are
made to raise; and the driver trains with --sample-fanout."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import hcspmm
import sampling_reference as ref
from hcspmm import graphs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hc-spmm_amd")
N, D, FANOUT = 300, 20, 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


_CACHE = {}


def _setup(dev):
    """the full graph (with its plan), one sample of it and the sample's dense float64 adjacency"""
    if "g" not in _CACHE:
        _pkg_imports()
        import GNN_model
        import HCSPMM
        rp, col = graphs.powerlaw_graph(N, 4000, seed=21, symmetric=False, max_degree_frac=0.5)
        assert np.diff(rp).max() > 64 and (np.diff(rp) <= FANOUT).any()
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        graph = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, len(col), (N + 15) // 16))
        graph_s, eid_s = GNN_model.sampled_graph(graph, FANOUT, seed=5)
        rp_s, col_s, want_eid = ref.sample_neighbors(rp, col, FANOUT, 5)
        assert np.array_equal(graph_s[0].cpu().numpy(), rp_s) and np.array_equal(graph_s[1].cpu().numpy(), col_s)
        assert np.array_equal(eid_s.cpu().numpy(), want_eid) and len(graph_s) == 8
        rows = np.repeat(np.arange(N), np.diff(rp_s))
        A = torch.zeros(N, N, dtype=torch.float64)
        A[torch.from_numpy(rows), torch.from_numpy(col_s).long()] = 1.0
        assert not torch.equal(A, A.t())  # directed
        _CACHE["g"] = dict(graph=graph, graph_s=graph_s, eid_s=eid_s, A=A)
    return _CACHE["g"]


def _close(got, want):  # test_directed_gpu._close
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return bool(((got - want).abs() <= 1e-4 * want.abs().max()).all())


def _leaf64(t):
    return t.detach().cpu().double().requires_grad_(True)


def _compare(fn, leaves, ref64):
    for t in leaves:
        t.grad = None
    out = fn()
    cot = torch.randn(out.shape, generator=torch.Generator(device="cpu").manual_seed(7)).to(out.device)
    (out * cot).sum().backward()
    leaves64 = [_leaf64(t) for t in leaves]
    out64 = ref64(*leaves64)
    (out64 * cot.cpu().double()).sum().backward()
    assert _close(out, out64), "forward"
    for i, (t, t64) in enumerate(zip(leaves, leaves64)):
        assert _close(t.grad, t64.grad), "gradient %d" % i


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_sage_layer_on_a_sampled_graph(dev, aggr):
    g = _setup(dev)
    import GNN_model
    torch.manual_seed(31)
    conv = GNN_model.SAGEConv(D, 16, aggr=aggr, directed=True).to(dev)
    X = torch.randn(N, D, device=dev, requires_grad=True)
    A = g["A"]

    def ref64(X, W_root, W_neigh):
        if aggr == "mean":
            agg = (A / A.sum(1).clamp(min=1)[:, None]) @ X
        else:
            agg = torch.where(A[:, :, None] > 0, X[None], torch.full((), -float("inf"), dtype=X.dtype)).amax(1)
            agg = torch.where(A.sum(1)[:, None] > 0, agg, torch.zeros((), dtype=X.dtype))  # rows without entries give 0
        return X @ W_root + agg @ W_neigh

    _compare(lambda: conv(X, *g["graph_s"], None), [X, conv.weights_root, conv.weights_neigh], ref64)


def test_weighted_aggregate_on_a_sampled_graph(dev):
    """the values of A travel to the sample as values[entry_index_s]"""
    g = _setup(dev)
    import GNN_model
    gen = torch.Generator(device="cpu").manual_seed(32)
    values = torch.rand(g["graph"][1].numel(), generator=gen).to(dev)
    w_s = values[g["eid_s"].long()].contiguous()
    X = torch.randn(N, D, generator=gen).to(dev).requires_grad_(True)
    A_w = torch.zeros(N, N, dtype=torch.float64)
    rp_s = g["graph_s"][0].cpu().numpy()
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp_s)))
    A_w[rows, g["graph_s"][1].cpu().long()] = w_s.cpu().double()
    _compare(lambda: GNN_model.weighted_aggregate(X, w_s, g["graph_s"], directed=True), [X], lambda X64: A_w @ X64)


def test_sample_and_transpose_never_touch_the_host_paths(dev, monkeypatch):
    g = _setup(dev)
    import GNN_model
    import HCSPMM

    def refuse(*a, **k):
        raise AssertionError("a host path was taken")

    for mod in (HCSPMM, hcspmm):
        for name in ("transpose_graph", "preprocess", "transpose_permutation", "build_plan"):
            monkeypatch.setattr(mod, name, refuse)
    graph_s, eid_s = GNN_model.sampled_graph(g["graph"], FANOUT, seed=6)
    gt = GNN_model.transposed_graph(graph_s)  # entered by sampled_graph: found, not built
    assert len(gt) == 9 and GNN_model.transposed_graph(graph_s) is gt
    for t in tuple(graph_s) + tuple(gt) + (eid_s,):
        assert t.is_cuda and t.dtype == torch.int32
    # entry_index_t names the sample's entries: A_s^T[j, i] is entry e_t's source
    A = torch.zeros(N, N)
    rows = torch.repeat_interleave(torch.arange(N), (graph_s[0][1:] - graph_s[0][:-1]).cpu().long())
    A[rows, graph_s[1].cpu().long()] = torch.arange(1, graph_s[1].numel() + 1, dtype=torch.float32)
    rows_t = torch.repeat_interleave(torch.arange(N), (gt[0][1:] - gt[0][:-1]).cpu().long())
    assert torch.equal(A.t()[rows_t, gt[1].cpu().long()], (gt[8].cpu() + 1).float())
    torch.manual_seed(33)
    X = torch.randn(N, D, device=dev, requires_grad=True)
    for aggr in ("mean", "max"):
        conv = GNN_model.SAGEConv(D, 8, aggr=aggr, directed=True).to(dev)
        conv(X, *graph_s, None).sum().backward()
    w = torch.rand(graph_s[1].numel(), device=dev)
    GNN_model.weighted_aggregate(X, w, graph_s, directed=True).sum().backward()
    assert torch.isfinite(X.grad).all()
    # an ordinary graph still takes the host path
    with pytest.raises(AssertionError, match="host path"):
        GNN_model.transposed_graph((g["graph"][0].clone(), g["graph"][1].clone()))


def test_driver_trains_on_a_fresh_sample_every_epoch(capsys, monkeypatch):
    _pkg_imports()
    monkeypatch.chdir(PKG)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_sampled", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, drawn = [], []
    nll, sample = mod.nll_loss, mod.sampled_graph

    def recording_loss(log_probs, target):
        loss = nll(log_probs, target)
        losses.append(float(loss.detach()))
        return loss

    def recording_sample(graph, fanout, seed):
        graph_s, eid_s = sample(graph, fanout, seed)
        drawn.append((graph, fanout, seed, graph_s[1].clone()))
        return graph_s, eid_s

    monkeypatch.setattr(mod, "nll_loss", recording_loss)
    monkeypatch.setattr(mod, "sampled_graph", recording_sample)
    torch.manual_seed(0)
    net = mod.main(["--dataset", "example", "--model", "sage", "--aggr", "mean", "--sample-fanout", "3", "--epochs", "2"])
    out = capsys.readouterr().out
    assert "Train (ms/epoch):" in out and "Eval (full graph):" in out
    assert len(losses) == 9 + 2 + 1 and all(np.isfinite(losses)), losses  # warm-up, the timed epochs, the evaluation
    assert len(drawn) == 9 + 2 and [d[2] for d in drawn] == list(range(11)) and all(d[1] == 3 for d in drawn)
    assert net.conv1.directed
    assert drawn[-1][3].shape == drawn[-2][3].shape and not torch.equal(drawn[-1][3], drawn[-2][3])  # the two timed epochs
    graph, _, seed, col_s = drawn[-1]
    assert torch.equal(sample(graph, 3, seed)[0][1], col_s)  # equal seeds, equal samples
    assert net.graph[1].numel() > col_s.numel()  # evaluated on the full graph
    for name, prm in net.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    with pytest.raises(SystemExit):
        mod.parse_args(["--model", "gcn", "--sample-fanout", "3"])  # the fused binary layer functions have no directed form
    with pytest.raises(SystemExit):
        mod.parse_args(["--model", "sage", "--sample-fanout", "3", "--graph"])
    args = mod.parse_args(["--model", "gcn", "--norm", "mean", "--sample-fanout", "3"])
    assert args.directed and args.sample_fanout == 3
    assert mod.parse_args(["--model", "sage"]).sample_fanout == 0
