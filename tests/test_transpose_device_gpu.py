"""The device-side transpose on an MI355X (hcspmm_transpose_graph_device) through both front-ends: its three outputs equal the
host counting sort's (transpose_graph) element for element -- stability is the contract: within a row of A^T the entries ascend
in e.  The shapes walk the radix sort's passes (one per eight bits of num_cols - 1) and tiles (2048 entries, 64 per step)."""
import ctypes

import numpy as np
import pytest
import torch

import frontends
import hcspmm
from hcspmm import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["ctypes", "extension"])
def fe(request):
    return frontends.get(request.param)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _csr(rows, cols, N):
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))]).astype(np.int32)
    return rp, cols.astype(np.int32)


def _random_graph(N, M, E, seed, columns=None):
    """E distinct cells of an N x M matrix; columns: the column ids that may be used (default: all)"""
    rng = np.random.default_rng(seed)
    columns = np.arange(M) if columns is None else np.asarray(columns)
    cells = rng.choice(N * len(columns), E, replace=False)
    return _csr(cells // len(columns), columns[cells % len(columns)], N)


def _check(fe, dev, rp, col, M, what):
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    want = hcspmm.transpose_graph(rp_d.cpu(), col_d.cpu(), M)  # the host counting sort
    got = fe.transpose_graph_device(rp_d, col_d, M)
    square = fe.transpose_graph_device(rp_d, col_d) if M == len(rp) - 1 else got  # num_cols defaults to square
    for g, s, w, name in zip(got, square, want, ("row_pointers_t", "column_index_t", "entry_index_t")):
        assert g.dtype == torch.int32 and g.device == rp_d.device and g.shape == w.shape, (what, name)
        assert torch.equal(g.cpu(), w) and torch.equal(s.cpu(), w), (what, name)
    return got


@pytest.mark.parametrize("E", [0, 1, 255, 256, 257, 100003])
def test_entry_counts(fe, dev, E):
    for N, M in ((1500, 900), (700, 2100)):  # num_cols smaller and larger than num_rows
        rp, col = _random_graph(N, M, E, seed=E + N)
        _check(fe, dev, rp, col, M, (E, N, M))
    if E == 257:
        rp, col = _random_graph(300, 300, E, seed=3)
        _check(fe, dev, rp, col, 300, "square")


@pytest.mark.parametrize("M", [1, 2, 255, 256, 257, 65536, 65537, 70001])
def test_column_counts_across_the_sort_passes(fe, dev, M):
    N = 40
    E = min(5000, N * M)
    rp, col = _random_graph(N, M, E, seed=M)
    if M > 1:
        col[-1] = M - 1  # the last column is referenced: the top digit is exercised
    _check(fe, dev, rp, col, M, M)


def test_unreferenced_columns(fe, dev):
    """columns without entries at the start, in the middle and at the end"""
    used = np.concatenate([np.arange(100, 400), np.arange(600, 900)])
    rp, col = _random_graph(500, 1000, 20000, seed=5, columns=used)
    rp_t = _check(fe, dev, rp, col, 1000, "gaps")[0].cpu().numpy()
    assert rp_t[100] == 0 and rp_t[400] == rp_t[600] and rp_t[900] == rp_t[1000] == 20000


def test_one_column_with_70000_entries(fe, dev):
    N, M = 70001, 300
    rng = np.random.default_rng(8)
    rows = np.concatenate([np.arange(70000), rng.integers(0, N, 30000)])
    cols = np.concatenate([np.full(70000, 5), rng.integers(6, M, 30000)])
    cells = np.unique(rows * M + cols)
    rp, col = _csr(cells // M, cells % M, N)
    rp_t = _check(fe, dev, rp, col, M, "hub column")[0].cpu().numpy()
    assert rp_t[6] - rp_t[5] == 70000


def test_transposes_of_sampled_graphs(fe, dev):
    import test_sampling_gpu as sg
    for deg, fanout in ((sg._mixed_degrees(10, 512), 10), (sg.HUB_DEGREES, 65)):
        rp, col = sg._graph_of_degrees(deg)
        rp_s, col_s, _ = fe.sample_neighbors(torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev), fanout, 31)
        M = int(col.max()) + 1
        _check(fe, dev, rp_s.cpu().numpy(), col_s.cpu().numpy(), M, ("sampled", fanout))


def test_a_too_small_workspace_is_refused(dev):
    rp, col = _random_graph(50, 50, 300, seed=1)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    L = capi.lib()
    need = L.hcspmm_transpose_graph_device_workspace_bytes(50, 50, 300)
    assert need >= 2 * 300 * 4
    out = [torch.empty(n, dtype=torch.int32, device=dev) for n in (51, 300, 300)]
    ws = torch.empty(need // 4, dtype=torch.int32, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = lambda w, nbytes: L.hcspmm_transpose_graph_device(ptr(rp_d), ptr(col_d), 50, 50, 300, *map(ptr, out), w, nbytes, stream)  # noqa: E731
    assert call(ptr(ws), need - 1) == capi.EWORKSPACE
    assert call(ctypes.c_void_p(0), need) == capi.EWORKSPACE
    assert call(ptr(ws), need) == capi.OK
    torch.cuda.synchronize()
    want = hcspmm.transpose_graph(rp_d.cpu(), col_d.cpu(), 50)
    for g, w in zip(out, want):
        assert torch.equal(g.cpu(), w)
