"""The neighbour sampler on an MI355X (hcspmm_sample_row_pointers_device, hcspmm_sample_neighbors_device) through both
front-ends: every comparison is exact integer equality with the numpy restatement tests/sampling_reference.py, which is written
from the definition in include/hcspmm.h.  The graphs walk the three row classes of the kernel (copy rows: deg <= fanout; wave
rows: up to SAMPLE_WAVE_ROW_MAX entries; hub rows: the workgroup) across each class limit."""
import numpy as np
import pytest
import torch

import frontends
import sampling_reference as ref
from hcspmm import graphs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["ctypes", "extension"])
def fe(request):
    return frontends.get(request.param)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _graph_of_degrees(deg):
    """row r holds the columns 0 ... deg[r] - 1 shifted by r % 3 (ascending, distinct); the sampler never looks at N"""
    deg = np.asarray(deg, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    rows = np.repeat(np.arange(len(deg)), deg)
    col = (np.arange(rp[-1]) - rp[rows] + rows % 3).astype(np.int32)
    return rp, col


def _mixed_degrees(fanout, limit):
    """301 rows (no multiple of 16): empty rows, rows at and next to the fanout, around a wave's width, and at each class
    limit +- 1, between short random rows"""
    rng = np.random.default_rng(7)
    deg = rng.integers(0, 12, 301)
    special = [0, 0, 1, fanout - 1, fanout, fanout + 1, 63, 64, 65, limit - 1, limit, limit + 1, 2 * limit + 3, 0, fanout + 1]
    deg[1 + rng.choice(299, len(special), replace=False)] = [max(d, 0) for d in special]
    deg[0], deg[300] = fanout + 1, limit + 1  # a sampled row first, a hub row last
    return deg


_REF = {}


def _want(name, rp, col, fanout, seed):
    key = (name, fanout, seed)
    if key not in _REF:
        _REF[key] = ref.sample_neighbors(rp, col, fanout, seed)
    return _REF[key]


def _check(fe, dev, name, rp, col, fanout, seed, **kw):
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    got = fe.sample_neighbors(rp_d, col_d, fanout, seed, **kw)
    want = _want(name, rp, col, fanout, seed)
    for g, w, what in zip(got, want, ("row_pointers_s", "column_index_s", "entry_index_s")):
        assert g.dtype == torch.int32 and g.device == rp_d.device
        assert np.array_equal(g.cpu().numpy(), w), (name, fanout, seed, what)
    return got


def test_empty_graphs(fe, dev):
    for n in (0, 1, 37):
        rp = np.zeros(n + 1, dtype=np.int32)
        rp_s, col_s, eid_s = _check(fe, dev, "empty%d" % n, rp, np.zeros(0, dtype=np.int32), 5, 3)
        assert rp_s.numel() == n + 1 and col_s.numel() == 0 and eid_s.numel() == 0
        assert torch.equal(fe.sample_row_pointers(torch.from_numpy(rp).to(dev), 5).cpu(), torch.zeros(n + 1, dtype=torch.int32))


@pytest.mark.parametrize("fanout", [1, 4, 10, 64, 65])
def test_mixed_rows_across_the_class_limits(fe, dev, fanout):
    limit = fe.SAMPLE_WAVE_ROW_MAX
    assert limit == 512
    rp, col = _graph_of_degrees(_mixed_degrees(fanout, limit))
    rp_s, col_s, eid_s = _check(fe, dev, "mixed", rp, col, fanout, 11)
    assert torch.equal(fe.sample_row_pointers(torch.from_numpy(rp).to(dev), fanout), rp_s)
    # column ids stay strictly ascending inside every sampled row
    c, p = col_s.cpu().numpy().astype(np.int64), rp_s.cpu().numpy()
    inner = np.ones(len(c), dtype=bool)
    inner[p[:-1][p[:-1] < len(c)]] = False  # the first entry of a row has no predecessor in it
    assert np.all(np.diff(c)[inner[1:]] > 0)


@pytest.mark.parametrize("fanout", [511, 512, 513, 1100])
def test_fanouts_around_the_wave_row_limit(fe, dev, fanout):
    """deg <= fanout copies however long the row is; fanout = limit: the row of limit + 1 entries is a hub row at once"""
    rp, col = _graph_of_degrees(_mixed_degrees(fanout, fe.SAMPLE_WAVE_ROW_MAX))
    _check(fe, dev, "mixed_wide", rp, col, fanout, 5)


def test_fanout_at_least_the_maximum_degree_gives_the_graph_back(fe, dev):
    rp, col = _graph_of_degrees(_mixed_degrees(10, fe.SAMPLE_WAVE_ROW_MAX))
    for fanout in (int(np.diff(rp).max()), 10 ** 6):
        rp_s, col_s, eid_s = _check(fe, dev, "mixed", rp, col, fanout, 2)
        assert np.array_equal(rp_s.cpu().numpy(), rp) and np.array_equal(col_s.cpu().numpy(), col)
        assert torch.equal(eid_s.cpu(), torch.arange(len(col), dtype=torch.int32))


HUB_DEGREES = [3, 5000, 0, 70000, 17, 600, 1]


@pytest.mark.parametrize("fanout", [1, 10, 64, 65, 4999, 69999])
def test_hub_rows(fe, dev, fanout):
    """one row of 5 000 entries and one of 70 000 (past 65 535), fanouts up to deg - 1 of each"""
    rp, col = _graph_of_degrees(HUB_DEGREES)
    _check(fe, dev, "hubs", rp, col, fanout, 77)


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345])
def test_seeds(fe, dev, seed):
    rp, col = _graph_of_degrees(_mixed_degrees(10, fe.SAMPLE_WAVE_ROW_MAX))
    _check(fe, dev, "mixed", rp, col, 10, seed)
    if seed == 1:  # another seed, another sample
        assert not np.array_equal(_want("mixed", rp, col, 10, 0)[2], _want("mixed", rp, col, 10, 1)[2])


def test_repeatable_on_any_stream_and_with_kept_row_pointers(fe, dev):
    rp, col = _graph_of_degrees(_mixed_degrees(10, fe.SAMPLE_WAVE_ROW_MAX))
    first = _check(fe, dev, "mixed", rp, col, 10, 123)
    again = _check(fe, dev, "mixed", rp, col, 10, 123)
    kept = _check(fe, dev, "mixed", rp, col, 10, 123, row_pointers_s=first[0])
    assert kept[0] is first[0] or kept[0].data_ptr() == first[0].data_ptr()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = _check(fe, dev, "mixed", rp, col, 10, 123)
    side.synchronize()
    for a, b, c, d in zip(first, again, kept, other):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_arguments_are_checked(fe, dev):
    rp, col = _graph_of_degrees([2, 3, 0, 8])
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    with pytest.raises(RuntimeError, match="fanout"):
        fe.sample_neighbors(rp_d, col_d, 0, 1)
    with pytest.raises(RuntimeError, match="fanout"):
        fe.sample_row_pointers(rp_d, 0)
    with pytest.raises(RuntimeError, match="int32"):
        fe.sample_neighbors(rp_d.long(), col_d, 2, 1)
    with pytest.raises(RuntimeError, match="row_pointers_s"):
        fe.sample_neighbors(rp_d, col_d, 2, 1, row_pointers_s=rp_d[:-1].contiguous())
    with pytest.raises(RuntimeError, match="CUDA"):
        fe.sample_neighbors(rp_d.cpu(), col_d.cpu(), 2, 1)


def test_a_generated_graph_with_mixed_degrees(fe, dev):
    rp, col = graphs.powerlaw_graph(400, 9000, seed=12, symmetric=False, max_degree_frac=0.9)
    deg = np.diff(rp)
    assert deg.min() < 4 and deg.max() > 64
    for fanout in (4, 25):
        rp_s, col_s, eid_s = _check(fe, dev, "powerlaw", rp, col, fanout, 2024)
        assert int(rp_s[-1]) == int(np.minimum(deg, fanout).sum()) < len(col)
