"""GPU tests of the sparse-row path's column-index loads (spmm_impl.h sparse_task): fp32 lane groups of 8 lanes -- every
launch with 32-column panels -- of the planned kernel whose wave holds a task of more than 32 entries fetch FOUR consecutive indices per lane with
one dword-aligned 16-byte load, so a chunk is 32 entries and a batch of gathers takes its indices from two lanes' components.
What can go wrong is which index a gather uses (chunk and batch edges, the 2- and 1-entry tail batches, lanes whose four
entries run past their task, waves on either side of the 32-entry switch) and where the 16 bytes come from (a task's first
entry is not 16-byte aligned; the last lanes of the last task must not read past `column_index`).

References: oracle.spmm_f32 (the sequential CSR-order fp32 sum) and oracle.check_spmm (fp64 product, 1e-5 * sum |x| bar).
  * a row that ONE lane group sums -- not split into segments, not cut into column slices, not handed to a whole wave --
    must equal the CSR-order oracle bit for bit (test_spmm_gpu._seq_limit is the same set);
  * every other row keeps the 1e-5 * sum |x| bar;
  * integer-valued X must give the exact result on EVERY row: all partial sums are integers below 2^24, so any order of the
    right entries gives it and any wrong, missing or repeated entry does not.
On a graph of this size the planned launch hands rows above 16 entries to whole waves (hcspmm_wide_threshold; they keep one
index per lane) and the plan-free kernel keeps one index per lane, so lane groups meet the 16-byte path only in the
column-sliced plans, whose pieces are never wide: up to about 50 entries on the mixed graph, and the banded graphs below
keep sliced rows in one piece of up to 256 entries.
"""
import numpy as np
import pytest
import torch

import frontends
import hcspmm

pytestmark = pytest.mark.gpu

# on and around every chunk (8 entries with one index per lane, 32 with four), batch (8, 4, 2, 1) and the 32-entry switch
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256]
WIDTHS = [32, 64, 128, 22, 33]  # L = 8 with one, two and four panels; ragged last lanes


@pytest.fixture(scope="module", params=["ctypes", "extension"])
def fe(request):
    return frontends.get(request.param)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _t(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dev is not None else t


def _graph(deg, n_cols, seed, band=None):
    """CSR with the given row lengths, ascending unique column ids below n_cols.  band: rows draw their ids from one of
    `band` equal column ranges (a column-sliced plan then keeps such a row in one long piece)."""
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    cols = []
    for i, d in enumerate(deg):
        if band:
            w = n_cols // band
            lo = (i % band) * w
            cols.append(lo + np.sort(rng.choice(w, size=d, replace=False)))
        else:
            cols.append(np.sort(rng.choice(n_cols, size=d, replace=False)))
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    return rp, col


def _mixed_degrees(n_rows, seed):
    """Every length of LENGTHS about equally often, shuffled: the tasks of one length class (17..32, say) that share a wave
    differ in length, so its lane groups run out of entries at different batches of a chunk."""
    deg = np.resize(np.array(LENGTHS, np.int64), n_rows)
    np.random.default_rng(seed).shuffle(deg)
    return deg


class Case:
    """One graph, preprocessed with rule 2 (every window takes the sparse-row path), and its references per width -- computed
    once, shared by the tests of the module and left unchanged."""

    def __init__(self, rp, col, dev, fe, col_d=None):
        self.rp, self.col, self.fe, self.dev = rp, col, fe, dev
        self.N, self.E = len(rp) - 1, len(col)
        self.deg = np.diff(rp)
        self.rp_d = _t(rp, dev)
        self.col_d = col_d if col_d is not None else _t(col, dev)
        outs = fe.preprocess(self.col_d, self.rp_d, self.N, self.E, (self.N + 15) // 16, rule=2)
        self.bp, self.e2c, self.e2r, self.ht, self.row_nzr, self.col_nzr = outs
        assert int(self.ht.sum()) == 0, "rule 2 left a dense-tile window"
        self.placeholder = torch.zeros(1, dtype=torch.int32, device=dev)
        self._refs = {}

    def refs(self, oracle_mod, D):
        if D not in self._refs:
            X = np.random.default_rng(1000 + D).standard_normal((self.N, D)).astype(np.float32)
            Xi = ((np.arange(self.N, dtype=np.float32) % 4093)[:, None] + np.arange(D, dtype=np.float32)[None, :])
            r = (X, oracle_mod.spmm_f32(self.rp, self.col, X), Xi, oracle_mod.spmm_f32(self.rp, self.col, Xi))
            for a in r:
                a.setflags(write=False)
            self._refs[D] = r
        return self._refs[D]

    def args(self, row_nzr):
        return (self.rp_d, self.col_d, self.bp, self.e2c, self.e2r, self.ht, row_nzr, self.col_nzr)

    def sequential_rows(self, row_nzr, D):
        """Rows that one lane group sums in CSR order (see the module docstring)."""
        h = self.fe.header(row_nzr)
        lim = self.fe.wide_threshold(row_nzr, D)
        if h is not None:
            lim = min(lim, h.split_threshold)
            if h.n_slices:
                lim = min(lim, h.slice_threshold)
        return self.deg <= lim

    def check(self, oracle_mod, D, row_nzr):
        X, ref, Xi, refi = self.refs(oracle_mod, D)
        Z = self.fe.forward(_t(X, self.dev), *self.args(row_nzr))[0]
        Zi = self.fe.forward(_t(Xi, self.dev), *self.args(row_nzr))[0]
        torch.cuda.synchronize()
        Z, Zi = Z.cpu().numpy(), Zi.cpu().numpy()
        ok, ratio = oracle_mod.check_spmm(Z, self.rp, self.col, X)
        assert ok, "relative error %.3g x the 1e-5 bar" % ratio
        seq = self.sequential_rows(row_nzr, D)
        bad = np.flatnonzero((Z[seq] != ref[seq]).any(axis=1))
        assert bad.size == 0, "rows of lengths %s differ from the CSR-order fp32 sum" % sorted(set(self.deg[seq][bad].tolist()))
        bad = np.flatnonzero((Zi != refi).any(axis=1))
        assert bad.size == 0, "integer X: rows of lengths %s are not exact" % sorted(set(self.deg[bad].tolist()))
        return seq


@pytest.fixture(scope="module")
def mixed(dev, fe):
    n = 2001
    rp, col = _graph(_mixed_degrees(n, seed=11), n, seed=12)
    return Case(rp, col, dev, fe)


@pytest.mark.parametrize("D", WIDTHS)
def test_row_lengths_on_every_chunk_and_batch_edge(oracle_mod, mixed, D):
    """Planned forward, both front-ends: every length of LENGTHS, mixed within the waves, at every width."""
    h = mixed.fe.header(mixed.row_nzr)
    assert h.n_dense == 0 and h.n_slices == 0
    seq = mixed.check(oracle_mod, D, mixed.row_nzr)
    assert set(mixed.deg[seq].tolist()) >= set(l for l in LENGTHS if l <= 16)


@pytest.mark.parametrize("D", WIDTHS)
def test_row_lengths_plan_free(oracle_mod, mixed, D):
    """The plan-free kernel gives every row of at most 64 entries to a lane group (eight chunks of one index per lane)."""
    seq = mixed.check(oracle_mod, D, mixed.placeholder)
    assert set(mixed.deg[seq].tolist()) >= set(l for l in LENGTHS if l <= 64)


@pytest.mark.parametrize("last", [1, 2, 3, 5, 9])
@pytest.mark.parametrize("rows_before", [0, 300])
@pytest.mark.parametrize("pad", [1, 2, 3])
def test_last_row_ends_at_the_last_element_of_column_index(oracle_mod, dev, fe, last, rows_before, pad):
    """The 16-byte load never needs a byte beyond column_index: the tensor holds exactly E elements, as a view that ENDS at
    the end of its storage (and starts `pad` ints into it, so no task is 16-byte aligned either); the last row -- the last
    lanes of the last task -- holds 1, 2, 3, 5 or 9 entries.  rows_before = 0: that row is the whole graph (E = 3: fewer
    entries than one load).  Everything here reads inside the tensor by construction; the result must be exact."""
    deg = np.concatenate([_mixed_degrees(rows_before, seed=last), [last]]).astype(np.int64)
    n = max(len(deg), 300)
    rp, col = _graph(deg, n, seed=20 + last)
    store = torch.empty(pad + len(col), dtype=torch.int32, device=dev)
    col_d = store[pad:]
    col_d.copy_(_t(col))
    assert col_d.numel() == len(col) and col_d.storage_offset() + col_d.numel() == store.numel()
    # (column ids index the rows of X: n of them, whatever the row count)
    rp_full = np.concatenate([rp, np.full(n - len(deg), rp[-1], np.int32)]).astype(np.int32)
    c = Case(rp_full, col, dev, fe, col_d=col_d)
    for D in (32, 128):
        for row_nzr in (c.row_nzr, c.placeholder):
            seq = c.check(oracle_mod, D, row_nzr)
            assert seq[len(deg) - 1]  # the last row is one lane group's (or a tiny task's): exact bits were demanded


@pytest.fixture(scope="module")
def strided_cases(dev):
    """(forward_into, the strided entry point, belongs to the ctypes front-end.)  The mixed graph with its own plan and with
    the plan-free placeholder, and the banded graph with a column-sliced plan: pieces of up to 256 entries, the 16-byte path."""
    fe = frontends.get("ctypes")
    n = 2001
    rp, col = _graph(_mixed_degrees(n, seed=11), n, seed=12)
    mixed = Case(rp, col, dev, fe)
    n = 2048
    rp, col = _graph(_mixed_degrees(n, seed=31), n, seed=32, band=8)
    banded = Case(rp, col, dev, fe)
    sliced = fe.build_plan(banded.rp_d, banded.col_d, banded.bp, banded.e2c, banded.ht, slice_threshold=16, n_slices=8)
    assert _piece_lengths(sliced).max() > 64
    return {"planned": (mixed, mixed.row_nzr), "plan_free": (mixed, mixed.placeholder), "sliced_banded": (banded, sliced)}


@pytest.mark.parametrize("which", ["planned", "plan_free", "sliced_banded"])
@pytest.mark.parametrize("D,pad,off", [(32, 5, 3), (32, 2, 1), (128, 7, 2), (128, 1, 1)])
def test_views_off_the_16_byte_grid(oracle_mod, dev, strided_cases, which, D, pad, off):
    """X and Z as column slices that start 1-3 floats into a wider matrix (as test_spmm_gpu's
    test_forward_parity_on_views_off_the_16_byte_grid): same bits as the contiguous call, nothing written outside the slice."""
    c, row_nzr = strided_cases[which]
    X, ref, _, _ = c.refs(oracle_mod, D)
    Xd = _t(X, dev)
    Xw = torch.full((c.N, D + pad + off), float("nan"), device=dev)
    Zw = torch.full((c.N, D + pad + off), -7.0, device=dev)
    Xv, Zv = Xw[:, off:off + D], Zw[:, off:off + D]
    Xv.copy_(Xd)
    want = c.fe.forward(Xd, *c.args(row_nzr))[0]
    hcspmm.forward_into(Xv, Zv, *c.args(row_nzr))
    torch.cuda.synchronize()
    assert torch.equal(Zv, want)
    ok, ratio = oracle_mod.check_spmm(Zv.cpu().numpy(), c.rp, c.col, X)
    assert ok, "relative error %.3g x the 1e-5 bar" % ratio
    seq = c.sequential_rows(row_nzr, D)
    assert np.array_equal(Zv.cpu().numpy()[seq], ref[seq])
    assert bool((Zw[:, :off] == -7.0).all()) and bool((Zw[:, off + D:] == -7.0).all())


def _piece_lengths(row_nzr):
    h = hcspmm.plan_header(row_nzr)
    words = row_nzr.cpu().numpy()
    d = words[h.off_slice_tasks:h.off_slice_tasks + 4 * h.n_slice_tasks].reshape(-1, 4)
    return d[d[:, 0] >= 0, 2]


@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("band", [0, 8], ids=["spread", "banded"])
def test_column_sliced_pieces(oracle_mod, dev, fe, mixed, D, band):
    """hcspmm_plan_params slice_threshold = 16, n_slices = 8: the XCD-bound region's descriptors go through the same index
    path and are never wide.  spread: column ids anywhere, pieces of 1-40 entries.  banded: every row inside one of eight
    column ranges, so that most sliced rows stay in one piece of up to 256 entries -- eight 32-entry chunks of one lane group,
    in waves that hold pieces on both sides of the 32-entry switch."""
    if band:
        n = 2048
        rp, col = _graph(_mixed_degrees(n, seed=31), n, seed=32, band=band)
        c = Case(rp, col, dev, fe)
    else:
        c = mixed
    plan = fe.build_plan(c.rp_d, c.col_d, c.bp, c.e2c, c.ht, slice_threshold=16, n_slices=8)
    h = fe.header(plan)
    assert h.n_slices == 8 and h.slice_threshold == 16 and h.n_sliced_rows == int((c.deg > 16).sum())
    pieces = _piece_lengths(plan)
    assert pieces.min() >= 1 and (pieces.max() > 64 if band else pieces.max() > 16), (pieces.min(), pieces.max())
    c.check(oracle_mod, D, plan)
    X = _t(c.refs(oracle_mod, D)[0], dev)
    assert torch.equal(fe.forward(X, *c.args(plan))[0], fe.forward(X, *c.args(plan))[0])  # no atomics: same bits twice


@pytest.mark.parametrize("last", [33, 34, 35, 37, 41, 64, 65, 66, 67, 69, 73, 96, 97])
@pytest.mark.parametrize("pad", [0, 1, 3])
def test_long_last_piece_ends_at_the_last_element_of_column_index(oracle_mod, dev, fe, last, pad):
    """The same end-of-array property where the 16-byte loads actually run: the LAST task of column_index is one sliced piece
    of 32 + or 64 + {1, 2, 3, 5, 9} entries (its last lane holds 1-3 entries that the array still has, or four) or of 64 / 96 /
    97 (whole last chunks / one entry into a fourth), in a tensor of exactly E elements that ends at the end of its storage."""
    n = 2048
    deg = np.concatenate([_mixed_degrees(303, seed=last), [last]]).astype(np.int64)  # row 303 draws from band 303 % 8 = 7
    deg = np.concatenate([deg, np.zeros(n - len(deg), np.int64)])
    rp, col = _graph(deg, n, seed=40 + last, band=8)
    # the last row well inside the last column range, whatever the slice boundaries' balance: it stays one piece
    col[-last:] = n - 128 + np.sort(np.random.default_rng(last).choice(128, size=last, replace=False))
    store = torch.empty(pad + len(col), dtype=torch.int32, device=dev)
    col_d = store[pad:]
    col_d.copy_(_t(col))
    assert col_d.storage_offset() + col_d.numel() == store.numel()
    c = Case(rp, col, dev, fe, col_d=col_d)
    plan = fe.build_plan(c.rp_d, c.col_d, c.bp, c.e2c, c.ht, slice_threshold=16, n_slices=8)
    h = hcspmm.plan_header(plan)
    d = plan.cpu().numpy()[h.off_slice_tasks:h.off_slice_tasks + 4 * h.n_slice_tasks].reshape(-1, 4)
    tail = d[(d[:, 0] == 303) & (d[:, 1] + d[:, 2] == len(col))]
    assert len(tail) == 1 and tail[0, 2] == last, "the last row was cut: the piece that ends the array is not %d long" % last
    for D in (32, 128):
        c.check(oracle_mod, D, plan)
