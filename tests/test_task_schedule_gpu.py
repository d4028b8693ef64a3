"""GPU tests of the binary product on the plan's schedule sections (include/hcspmm.h off_task_sched / off_slice_sched): the
wide and the ordinary regions and the XCD-bound sliced region read their descriptors from copies in exact descending length
order.  What can go wrong is which descriptor a lane group reads (the last wave of a region when the task count is no
multiple of 8 or 32, the padding of a slice list now BEHIND descriptors of another order, the wide-task prefix on the sorted
copy) and a row summed twice or not at all; the sums themselves do not change, so every row keeps its bits.

Graphs as test_index_chunks_gpu.py builds them -- every length 3 ... 256 in shuffled row order -- plus rows of 300-2 000
entries, whose segments (above the split threshold of 512) and column-slice pieces go through the schedule with their partial
slots.  On graphs of this size the launch hands rows above 16 entries to whole waves, so lane groups meet the long
descriptors in the column-sliced plans (pieces are never wide); the banded graph keeps its pieces up to 256 entries long.

References: oracle.spmm_f32 (sequential CSR-order fp32 sum) bit for bit on every row one lane group sums, oracle.check_spmm
(fp64, 1e-5 * sum |x|) on the others, exact integers everywhere (test_index_chunks_gpu.Case.check); and the same plan built
with HCSPMM_TASK_SCHEDULE=0, whose launch reads the lists as before: equal bits."""
import os

import numpy as np
import pytest
import torch

import frontends
import hcspmm
import test_index_chunks_gpu as chunks

pytestmark = pytest.mark.gpu

LONG = [300, 333, 400, 511, 512, 513, 700, 1000, 1025, 1500, 2000]
_t = chunks._t


@pytest.fixture(scope="module", params=["ctypes", "extension"])
def fe(request):
    return frontends.get(request.param)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _degrees(seed):
    """Every length 3 ... 256 nine times (and three more rows, so that no region ends on a whole wave or workgroup), the long
    rows, and 0 / 1 / 2 (tiny tasks: not in the schedule), shuffled."""
    deg = np.array(list(range(3, 257)) * 9 + [17, 40, 100] + LONG * 2 + [0, 1, 2] * 31, np.int64)
    np.random.default_rng(seed).shuffle(deg)
    return deg


def _graph(deg, seed, band=0):
    """CSR with the given row lengths and as many columns as rows, ascending unique ids.  band: rows of at most 256 entries
    draw theirs from one of `band` equal column ranges, so that a column-sliced plan keeps most of them in one piece."""
    rng = np.random.default_rng(seed)
    n = len(deg)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    cols = []
    for i, d in enumerate(deg):
        if band and d <= 256:
            w = n // band
            cols.append((i % band) * w + np.sort(rng.choice(w, size=d, replace=False)))
        else:
            cols.append(np.sort(rng.choice(n, size=d, replace=False)))
    return rp, np.concatenate(cols).astype(np.int32)


def _without_schedule(build):
    keep = os.environ.get("HCSPMM_TASK_SCHEDULE")
    os.environ["HCSPMM_TASK_SCHEDULE"] = "0"  # read by every plan build
    try:
        return build()
    finally:
        if keep is None:
            del os.environ["HCSPMM_TASK_SCHEDULE"]
        else:
            os.environ["HCSPMM_TASK_SCHEDULE"] = keep


@pytest.fixture(scope="module")
def cases(dev, fe):
    """kind -> (Case, plan with the schedule, the same plan without).  slices_off: the plan as the library builds it at this
    size; sliced: rows above 32 entries cut into 8 column slices, column ids anywhere (short pieces, long lists);
    sliced_banded: every row inside one of 8 column ranges (pieces up to 256 entries)."""
    out = {}
    for kind, band, params in (("slices_off", None, dict(slice_threshold=-1)),
                               ("sliced", None, dict(slice_threshold=32, n_slices=8)),
                               ("sliced_banded", 8, dict(slice_threshold=32, n_slices=8))):
        deg = _degrees(seed=51 + len(kind))
        rp, col = _graph(deg, seed=61 + len(kind), band=band)
        c = chunks.Case(rp, col, dev, fe)
        build = lambda: fe.build_plan(c.rp_d, c.col_d, c.bp, c.e2c, c.ht, **params)
        plan, plain = build(), _without_schedule(build)
        h, h0 = hcspmm.plan_header(plan), hcspmm.plan_header(plain)
        assert h.off_task_sched > 0 and (h.off_slice_sched > 0) == (kind != "slices_off")
        assert h0.off_task_sched == 0 and h0.off_slice_sched == 0 and h0.total_words < h.total_words
        assert (h.n_slices, h.n_tiny, h.n_tasks, h.n_partials) == (h0.n_slices, h0.n_tiny, h0.n_tasks, h0.n_partials)
        n_nt = h.n_tasks - h.n_tiny
        assert n_nt % 8 != 0 and n_nt % 32 != 0 and h.n_split_rows > 0
        out[kind] = (c, plan, plain)
    return out


@pytest.mark.parametrize("kind", ["slices_off", "sliced", "sliced_banded"])
@pytest.mark.parametrize("D", [22, 32, 128, 256])
def test_fp32_rows_keep_their_bits(oracle_mod, cases, kind, D):
    c, plan, plain = cases[kind]
    h = hcspmm.plan_header(plan)
    thr = c.fe.wide_threshold(plan, D)
    n_nt = h.n_tasks - h.n_tiny
    if kind == "slices_off":  # the wide prefix and the ordinary region behind it both end in a partial wave
        assert thr in (16, 32, 64, 128, 256)
        n_wide = h.n_len_gt[(16, 32, 64, 128, 256).index(thr)]
        assert 0 < n_wide < n_nt and n_wide % 4 != 0 and (n_nt - n_wide) % 8 != 0
    else:
        words = plan.cpu().numpy()
        table = words[h.off_slice_table:h.off_slice_table + h.n_slices + 1]
        pieces = words[h.off_slice_sched:h.off_slice_sched + 4 * h.n_slice_tasks].reshape(-1, 4)
        real = [int((pieces[table[s]:table[s + 1], 0] >= 0).sum()) for s in range(h.n_slices)]
        assert any(r % 8 != 0 for r in real) and pieces[:, 2].max() > (128 if kind == "sliced_banded" else 32)
    seq = c.check(oracle_mod, D, plan)
    assert seq.sum() > 100 and (~seq).sum() >= len(LONG)
    c.check(oracle_mod, D, plain)
    X = _t(c.refs(oracle_mod, D)[0], c.dev)
    Z, Z0 = c.fe.forward(X, *c.args(plan))[0], c.fe.forward(X, *c.args(plain))[0]
    # the same tasks summed by the same lanes, partial sums added in slot order: equal bits on every row, split ones included
    assert torch.equal(Z, Z0)


def _integer_features(N, D):
    """Integers in [-8, 8]: exact in e4m3 and bf16; a row of 2 000 of them sums below 2^14, exact in fp32 in any order."""
    return ((np.arange(N, dtype=np.int64)[:, None] * 7 + np.arange(D, dtype=np.int64)[None, :] * 3) % 17 - 8).astype(np.float32)


@pytest.mark.parametrize("kind", ["slices_off", "sliced_banded"])
def test_bf16_and_fp8_features(oracle_mod, cases, kind):
    """D = 128: the 16-bit build (one rounding of the fp32 sum to bf16) and the 8-bit build (fp32 out) through the schedule."""
    c, plan, plain = cases[kind]
    D = 128
    Xi = _integer_features(c.N, D)
    want = torch.from_numpy(oracle_mod.spmm_f32(c.rp, c.col, Xi)).to(c.dev)  # exact
    X16 = _t(Xi, c.dev).to(torch.bfloat16)
    assert torch.equal(X16.float().cpu(), torch.from_numpy(Xi))
    Z16 = c.fe.forward(X16, *c.args(plan))[0]
    assert Z16.dtype == torch.bfloat16 and torch.equal(Z16, want.to(torch.bfloat16))
    assert torch.equal(Z16, c.fe.forward(X16, *c.args(plain))[0])
    X8 = _t(Xi, c.dev).to(torch.float8_e4m3fn)
    assert torch.equal(X8.float().cpu(), torch.from_numpy(Xi))
    Z8 = c.fe.forward_fp8(X8, None, *c.args(plan))[0]
    assert Z8.dtype == torch.float32 and torch.equal(Z8, want)
    assert torch.equal(Z8, c.fe.forward_fp8(X8, None, *c.args(plain))[0])


def test_replays_in_a_hip_graph(oracle_mod, cases):
    c, plan, _ = cases["sliced"]
    X = _t(c.refs(oracle_mod, 128)[0], c.dev).clone()
    ref = c.fe.forward(X, *c.args(plan))[0]  # warm-up: plan registry and fingerprint checks happen here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = c.fe.forward(X, *c.args(plan))[0]
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    X.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref * 2.0)  # scaling by two is exact
