"""GPU tests of the binary product on the first-index records of the plan's schedule copies (include/hcspmm.h
off_task_sched_idx / off_slice_sched_idx): the ordinary and the sliced waves take the first chunk of their tasks' column indices
from a record they ask for together with the descriptor, every later chunk from column_index as before.  What can go wrong is
which record a lane group reads (the last wave of a region, the padding of a slice list, lists that are empty or shorter than
one wave, the table of eight slices passed as kernel arguments), the hand-over from the record to column_index at entry 8
(one index per lane) or 32 (four), and lane groups of other widths than 8 (D = 128 in one pass for 16-bit and 8-bit rows).
The entries, the lanes and the order of the additions do not change, so every row keeps its bits.

One plan is built with the records and once more with HCSPMM_SCHED_INDEX=0 -- byte for byte the plan from before the records
existed (test_sched_index_cpu.py), so this is also the run of an old plan on the new kernels.  Both must pass
test_index_chunks_gpu.Case.check (oracle.spmm_f32 bit for bit on the rows one lane group sums, oracle.check_spmm -- fp64,
1e-5 * sum |x| -- on the others, exact integers everywhere), and their outputs must be equal bit for bit.

Graphs: 3 001 rows over as many columns; row lengths 0, 1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257 about equally
often and rows of 600-3 000 entries, shuffled.  On graphs of this size the launch hands rows above 16 entries to whole waves
when nothing is sliced, so the long first chunks are met in the column-sliced plans, whose pieces are never wide."""
import os

import numpy as np
import pytest
import torch

import frontends
import hcspmm
import test_index_chunks_gpu as chunks
from test_task_schedule_gpu import _graph, _integer_features

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257]
LONG = [600, 777, 1024, 1500, 2049, 3000]
N_ROWS = 3001
_t = chunks._t


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _degrees(seed, last=None):
    deg = np.concatenate([np.resize(np.array(LENGTHS, np.int64), N_ROWS - len(LONG) - (last is not None)), LONG])
    np.random.default_rng(seed).shuffle(deg)
    return deg if last is None else np.concatenate([deg, [last]])


def _without_records(build):
    keep = os.environ.get("HCSPMM_SCHED_INDEX")
    os.environ["HCSPMM_SCHED_INDEX"] = "0"  # read by every plan build
    try:
        return build()
    finally:
        if keep is None:
            del os.environ["HCSPMM_SCHED_INDEX"]
        else:
            os.environ["HCSPMM_SCHED_INDEX"] = keep


# kind -> (row lengths, column band count of test_task_schedule_gpu._graph, plan parameters)
#   slices_off   the plan the library builds at this size, no slices
#   sliced       rows above 32 entries in 8 column slices, every row of at most 256 entries inside one of 8 column ranges: pieces
#                of up to 256 entries, both index paths in one wave; the last row's 100 entries stay one piece, so column_index
#                ends inside a task's continuation chunks
_KINDS = {
    "slices_off": (lambda: _degrees(71), None, dict(slice_threshold=-1)),
    "sliced": (lambda: _degrees(75, last=100), 8, dict(slice_threshold=32, n_slices=8)),
}


def _make(kind):
    """(rp, col) of a kind: as many columns as rows, ascending unique ids; with bands, rows of at most 256 entries draw theirs
    from one of 8 equal column ranges.  sliced: the last row's 100 entries lie in the last 128 columns, one piece."""
    degrees, band, _ = _KINDS[kind]
    deg = degrees()
    rp, col = _graph(deg, seed=80 + len(kind), band=band or 0)
    if kind == "sliced":
        col[-100:] = len(deg) - 128 + np.sort(np.random.default_rng(5).choice(128, size=100, replace=False))
    return rp, col


def _lists(plan, h):
    """Real descriptors per slice list of a plan."""
    words = plan.cpu().numpy()
    table = words[h.off_slice_table:h.off_slice_table + h.n_slices + 1]
    d = words[h.off_slice_sched:h.off_slice_sched + 4 * h.n_slice_tasks].reshape(-1, 4)
    return [int((d[table[s]:table[s + 1], 0] >= 0).sum()) for s in range(h.n_slices)], d


_built = {}


def _case(kind, front_end, dev):
    """(Case, plan with the records, the same plan without) of a kind through a front-end, built once and shared read-only."""
    if (kind, front_end) in _built:
        return _built[(kind, front_end)]
    fe = frontends.get(front_end)
    params = _KINDS[kind][2]
    rp, col = _make(kind)
    c = chunks.Case(rp, col, dev, fe)
    build = lambda: fe.build_plan(c.rp_d, c.col_d, c.bp, c.e2c, c.ht, **params)
    plan, plain = build(), _without_records(build)
    h, h0 = hcspmm.plan_header(plan), hcspmm.plan_header(plain)
    sliced = kind != "slices_off"
    assert h.off_task_sched > 0 and h.off_task_sched_idx > 0 and (h.off_slice_sched_idx > 0) == sliced == (h.n_slices == 8)
    assert h0.off_task_sched == h.off_task_sched and h0.off_task_sched_idx == 0 and h0.off_slice_sched_idx == 0
    assert h0.total_words < h.total_words and torch.equal(plain[64:], plan[64:h0.total_words])
    assert h.n_tasks - h.n_tiny > 0 and h.n_split_rows > 0
    if sliced:
        real, d = _lists(plan, h)
        assert any(r % 8 != 0 for r in real)
        assert d[:, 2].max() > 128
        tail = d[(d[:, 0] >= 0) & (d[:, 1] + d[:, 2] == c.E)]  # the piece that ends column_index is read past its record
        assert len(tail) == 1 and tail[0, 2] > 32
    _built[(kind, front_end)] = (c, plan, plain)
    return _built[(kind, front_end)]


# Ragged lanes and four panels on the plan without slices, one and four panels on the sliced one (four through the extension
# front-end; the ctypes one runs the sliced plan at D = 128 in test_strided_views and test_bf16_and_fp8_features).  Slice lists that
# are empty or shorter than a wave: test_empty_slice_lists.
@pytest.mark.parametrize("front_end,kind,D", [("ctypes", "slices_off", 22), ("ctypes", "slices_off", 128), ("ctypes", "sliced", 32),
                                              ("extension", "sliced", 128)])
def test_fp32_rows_keep_their_bits(oracle_mod, dev, front_end, kind, D):
    c, plan, plain = _case(kind, front_end, dev)
    seq = c.check(oracle_mod, D, plan)
    assert seq.sum() > 100 and (~seq).sum() >= len(LONG)
    c.check(oracle_mod, D, plain)
    X = _t(c.refs(oracle_mod, D)[0], c.dev)
    Z, Z0 = c.fe.forward(X, *c.args(plan))[0], c.fe.forward(X, *c.args(plain))[0]
    assert torch.equal(Z, Z0)


def test_empty_slice_lists(oracle_mod, dev):
    """Eight lists of which some are empty and the others hold one piece, less than a wave: the slice boundaries follow the sliced rows' entries,
    so a list is empty only when there are fewer sampled entries than lists -- one sliced row of 19 entries above a threshold
    of 16, among 3 000 rows of at most 9."""
    fe = frontends.get("ctypes")
    deg = np.resize(np.array([l for l in LENGTHS if l <= 9], np.int64), N_ROWS)
    np.random.default_rng(76).shuffle(deg)
    deg[1234] = 19
    rp, col = _graph(deg, seed=90)
    c = chunks.Case(rp, col, dev, fe)
    build = lambda: fe.build_plan(c.rp_d, c.col_d, c.bp, c.e2c, c.ht, slice_threshold=16, n_slices=8)
    plan, plain = build(), _without_records(build)
    h = hcspmm.plan_header(plan)
    real, _ = _lists(plan, h)
    assert h.n_sliced_rows == 1 and h.off_slice_sched_idx > 0 and real.count(0) >= 2 and 0 < max(real) < 8, real
    D = 128
    c.check(oracle_mod, D, plan)
    c.check(oracle_mod, D, plain)
    X = _t(c.refs(oracle_mod, D)[0], c.dev)
    assert torch.equal(c.fe.forward(X, *c.args(plan))[0], c.fe.forward(X, *c.args(plain))[0])


def test_bf16_and_fp8_features(oracle_mod, dev):
    """D = 128: the 16-bit build (16-lane groups, one rounding of the fp32 sum to bf16) and the 8-bit build (fp32 out) read
    one index per lane from the records."""
    c, plan, plain = _case("sliced", "ctypes", dev)
    D = 128
    Xi = _integer_features(c.N, D)
    want = torch.from_numpy(oracle_mod.spmm_f32(c.rp, c.col, Xi)).to(c.dev)  # exact
    X16 = _t(Xi, c.dev).to(torch.bfloat16)
    Z16 = c.fe.forward(X16, *c.args(plan))[0]
    assert Z16.dtype == torch.bfloat16 and torch.equal(Z16, want.to(torch.bfloat16))
    assert torch.equal(Z16, c.fe.forward(X16, *c.args(plain))[0])
    X8 = _t(Xi, c.dev).to(torch.float8_e4m3fn)
    Z8 = c.fe.forward_fp8(X8, None, *c.args(plan))[0]
    assert Z8.dtype == torch.float32 and torch.equal(Z8, want)
    assert torch.equal(Z8, c.fe.forward_fp8(X8, None, *c.args(plain))[0])


@pytest.mark.parametrize("kind,D,pad,off", [("sliced", 128, 7, 2)])
def test_strided_views(oracle_mod, dev, kind, D, pad, off):
    """hcspmm_forward_strided (hcspmm.forward_into, the ctypes front-end's): X and Z as column slices that start 2-3 floats
    into a wider matrix -- the same bits as the contiguous call, nothing written outside the slice."""
    c, plan, _ = _case(kind, "ctypes", dev)
    fe = c.fe
    X = c.refs(oracle_mod, D)[0]
    Xd = _t(X, dev)
    Xw = torch.full((c.N, D + pad + off), float("nan"), device=dev)
    Zw = torch.full((c.N, D + pad + off), -7.0, device=dev)
    Xv, Zv = Xw[:, off:off + D], Zw[:, off:off + D]
    Xv.copy_(Xd)
    want = fe.forward(Xd, *c.args(plan))[0]
    hcspmm.forward_into(Xv, Zv, *c.args(plan))
    torch.cuda.synchronize()
    assert torch.equal(Zv, want)
    ok, ratio = oracle_mod.check_spmm(Zv.cpu().numpy(), c.rp, c.col, X)
    assert ok, "relative error %.3g x the 1e-5 bar" % ratio
    assert bool((Zw[:, :off] == -7.0).all()) and bool((Zw[:, off + D:] == -7.0).all())
