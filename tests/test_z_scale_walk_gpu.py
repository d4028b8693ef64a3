"""The five kernel families on the shared CSR schedule walk (csrc/csr_schedule.h) -- multi-aggregate, softmax aggregation, its
backward, edge-feature messages, gated aggregation -- behind the launch decisions that only large graphs take, at their shipped
defaults, on an MI355X.

On the graphs of the families' own modules (1 200 - 16 000 rows) capi.hip wide_choice returns 16 wherever a wave holds more than
one lane group, so the non-wide task body task<false> at L = 4 ... 32 never sums more than 16 entries on a planned launch there.
test_scale_paths_gpu.py closed that hole (its gates B, C, D) for the binary, weighted, multi-head and extremum kernels; this
module does it for the walk's other users, on that module's 300 000-row / 6 M-entry power-law graph (imported, not copied).

Three plan forms: `no_slices` (slice_threshold = -1: gate B alone), `auto` (the plan as the library builds it: automatic column
slices, split rows, panels chosen at launch) and `one_pass` (the plan's own panel_cols = -1, a plan parameter: without it L = 16
and 32 are reached only where X passes 256 MiB, since 32-column panels run at L = 8).  A cell is (form, D);
test_every_cell_is_past_its_gate asserts the table through fe.wide_threshold and hcspmm.plan_header:

  form, D          panel, L          wide threshold (rows up to it: one lane group, CSR order)
  no_slices  32    one pass, 8       32
  auto       32    one pass, 8       32   rows above slice_threshold cut into column slices
  no_slices  64    32 columns, 8     64
  one_pass   64    one pass, 16      64
  no_slices 128    32 columns, 8     128
  one_pass  128    one pass, 32      128
  no_slices 256    64 columns, 16    256  (X = 307 MB > 256 MiB: gate C)
  auto      256    64 columns, 16    2^31 - 1: the slices took every row above 256 entries, so no task is wide and rows up to
                                     slice_threshold = 256 stay on one lane group; slices, split rows and the fix-up pass

Out of scope: L = 4 with a threshold above 16 needs more than about 8.4 M sparse entries (0.25 * nnz / (16 * 4096) >= 32), too
large for tests of a few seconds; L = 64 has no wide task at all and is covered by the small graphs.

The plan sorts its tasks, and the pieces of every slice list, by descending power-of-two length class (plan_host.cpp), so the
lane groups of one planned wave differ by less than a factor of four in length: a task of 3 entries never sits next to one of
250 (that mix is what the forced-dense forms of the families' own modules run: csr_window_rows takes a window's rows in row
order, whatever their lengths).  What the class order allows, and the coverage test asserts from the plan's own task list, is a
wave whose lane groups need different numbers of index chunks: under the wave's nmax one of them then runs a whole chunk with
idx = -1 in every lane while another still sums.  The test prints the widest mix it finds in both regions.

The criteria are the sibling modules' own, restated on device tensors; no tolerance is new.  References are plain torch on the
device: fp64 per-entry terms summed by index_add, 16 columns at a time; where a sibling uses an fp32 numpy yardstick, a
sequential fp32 sum, one CSR position at a time over all rows that still have one (never index_add: its order is not fixed).
The siblings' row groups (at most 64 entries / longer) marked, on their graphs, the rows one lane group sums; here the boundary
is the cell's own sequential limit (test_scale_paths_gpu._seq_limit).
"""
import ctypes

import numpy as np
import pytest
import torch

import frontends
import hcspmm
import test_scale_paths_gpu as scale
from hcspmm import capi
from test_multi_aggr_gpu import _direct as _multi_direct
from test_softmax_aggr_gpu import _beta
from test_softmax_aggr_gpu import _direct as _softmax_direct
from test_z_gated_gpu import _direct as _gated_direct

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KIND = "power_law"
# D-major: the references of one width are computed once, shared by its cells, and dropped when the width changes
CELLS = [("no_slices", 32), ("auto", 32), ("no_slices", 64), ("one_pass", 64), ("no_slices", 128), ("one_pass", 128),
         ("no_slices", 256), ("auto", 256)]
NO_WIDE_TASK = 2 ** 31 - 1  # what wide_choice answers where the plan has no task above the threshold it arrives at
# (form, D) -> (panel columns, L, wide threshold): arithmetic from capi.hip, asserted against the library's answers
EXPECTED = {("no_slices", 32): (32, 8, 32), ("auto", 32): (32, 8, 32), ("no_slices", 64): (32, 8, 64), ("one_pass", 64): (64, 16, 64),
            ("no_slices", 128): (32, 8, 128), ("one_pass", 128): (128, 32, 128), ("no_slices", 256): (64, 16, 256),
            ("auto", 256): (64, 16, NO_WIDE_TASK)}
ONE_PASS = dict(panel_cols=-1)
CELL_IDS = ["%s-%d" % c for c in CELLS]
# one cell per family for the second front-end and for the framed operands: every form and every L among them
EXT_CELL = {"multi": ("one_pass", 64), "softmax": ("auto", 256), "softmax_backward": ("no_slices", 128), "edge": ("auto", 32),
            "gated": ("one_pass", 128)}
FRAME_CELL = {"multi": ("auto", 256), "softmax": ("one_pass", 128), "softmax_backward": ("one_pass", 64), "edge": ("no_slices", 128),
              "gated": ("auto", 32)}
FAMILIES = list(EXT_CELL)
OPS = ("mul", "add_relu", "copy")
F_ROWS = 4096  # rows of the edge-feature table: a direct [E, 256] F would be 6 GB
SENTINEL = -777.0

_PLANS = {}
_REFS = {}   # one key at a time: (family, D) -> operands and references
_WALK = {}
_WORST = {}  # (family, output, row group) -> the largest error / bound of the continuous-data checks


@pytest.fixture(scope="module")
def fe():
    """the ctypes front-end runs every cell; the extension runs test_the_extension_gives_the_ctypes_bits"""
    return frontends.get("ctypes")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    yield torch.device("cuda:0")
    for key in sorted(_WORST):  # per family, output and row group (below / above the sequential limit)
        print("%s %s, rows %s limit: largest error / bound %.3f" % (key + (_WORST[key],)))
    _REFS.clear()
    _PLANS.clear()
    _WALK.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- graph, plans, caches
def _plan(fe, dev, form):
    """test_scale_paths_gpu's graph and plans (its cache, so a session builds them once); one_pass: the same windows, and a
    plan that differs in its panel_cols alone"""
    if form != "one_pass":
        return scale._setup(fe, dev, KIND, form)
    key = (fe.name, form)
    if key not in _PLANS:
        g = dict(scale._setup(fe, dev, KIND, "auto"))
        rp_d, col_d, bp, e2c, e2r, ht, _, col_nzr = g["args"]
        g["row_nzr"] = fe.build_plan(rp_d, col_d, bp, e2c, ht, **ONE_PASS)
        g["args"] = (rp_d, col_d, bp, e2c, e2r, ht, g["row_nzr"], col_nzr)
        _PLANS[key] = g
    return _PLANS[key]


def _cached(key, make):
    if key not in _REFS:
        _REFS.clear()
        torch.cuda.empty_cache()
        _REFS[key] = make()
    return _REFS[key]


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _is_plus_zero(t):
    return not bool(_bits(t).any())


def _panel_cols(h, D):
    """capi.hip panel_choice, fp32, no environment override"""
    if h.panel_cols != 0:
        return D if h.panel_cols < 0 else min(h.panel_cols, D)
    if D < 64 or h.n_tasks <= 0 or h.nnz_sparse / (h.n_tasks + h.n_slice_tasks) < 8.0:
        return D
    cols = 64 if h.num_columns * D * 4 > 256 * 1048576 else 32
    return cols if D >= 2 * cols else D


# ------------------------------------------------------------------------------------------- references on the device
def _walk(g):
    """rows by descending length (the rows that still have a k-th entry are a prefix), their first entries, and the prefix
    lengths, counted on the host: the loop below never waits for the device"""
    if "walk" not in _WALK:
        order = torch.argsort(g["deg_d"], descending=True, stable=True)
        starts = g["rp_d"].long()[order]
        asc = np.sort(g["deg"])
        counts = g["N"] - np.searchsorted(asc, np.arange(int(asc[-1]) + 1), side="right")  # counts[k]: rows longer than k
        _WALK["walk"] = (order, starts, counts)
    return _WALK["walk"]


def _sequential(g, width, term, limit=None):
    """fp32 row sums, one CSR position at a time: acc = fl(acc + term(r, e)) for the k-th entry e of every row r that has one,
    k = 0, 1, ...; term returns float32 [len(r), width].  limit: only the rows of at most that many entries (the others stay 0)"""
    order, starts, counts = _walk(g)
    skip = int(counts[limit]) if limit is not None and limit < len(counts) else 0
    acc = torch.zeros((g["N"], width), dtype=torch.float32, device=order.device)
    for k in range(len(counts) - 1):
        n = int(counts[k])
        if n <= skip:
            break
        acc[skip:n] += term(order[skip:n], starts[skip:n] + k)
    out = torch.empty_like(acc)
    out[order] = acc
    return out


def _fp64_sums(g, D, terms, n_out, chunk=16):
    """n_out float64 [N, D] row sums of the per-entry terms; terms(column slice) -> n_out float64 [E, c] tensors"""
    dev = g["rows"].device
    out = [torch.empty((g["N"], D), dtype=torch.float64, device=dev) for _ in range(n_out)]
    for c0 in range(0, D, chunk):
        sl = slice(c0, min(c0 + chunk, D))
        for o, t in zip(out, terms(sl)):
            o[:, sl] = torch.zeros((g["N"], t.size(1)), dtype=torch.float64, device=dev).index_add_(0, g["rows"], t)
    return out


def _yard(ref64, yard32):
    """what a bound needs of a reference and its yardstick: the reference, the yardstick's error per row, 1e-6 max|ref|"""
    return ref64, (yard32.double() - ref64).abs().amax(1), 1e-6 * float(ref64.abs().max())


def _groups(g, limit):
    seq = g["deg_d"] <= limit
    return (("rows <= %d" % limit, seq), ("rows > %d" % limit, ~seq))


def _note(family, name, group, ratio, detail=""):
    key = (family, name, group.split()[1])
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    print("%s %s, %s: error / bound = %.3f%s" % (family, name, group, ratio, detail))


def _check_yard_bound(family, name, got, yard, g, limit, tag):
    """test_softmax_aggr_gpu._bounds / _check_bound: the library may err by 4 x the yardstick's maximum error + 1e-6 max|ref|,
    taken separately over the rows one lane group sums and over the others"""
    ref64, yerr, floor = yard
    err = (got.double() - ref64).abs().amax(1)
    for group, mask in _groups(g, limit):
        assert bool(mask.any()), (tag, group)
        y, e = float(yerr[mask].max()), float(err[mask].max())
        bound = 4.0 * y + floor
        _note(family, name, group, e / bound, " (library %.3e, yardstick %.3e, bound %.3e) %s" % (e, y, bound, tag))
        assert e <= bound, (tag, name, group, e, y, bound)


def _check_elementwise_bound(family, name, got, exact, bound, g, limit, tag):
    """|got - exact| <= bound for every element; error / bound printed per row group"""
    err = (got.double() - exact).abs()
    ratio = (err / bound.clamp(min=1e-300)).amax(1)
    for group, mask in _groups(g, limit):
        _note(family, name, group, float(ratio[mask].max()), " %s" % (tag,))
    assert bool((err <= bound).all()), (tag, name, float(ratio.max()))


def _int_features(gen, rows, D, dev):
    """test_multi_aggr_gpu._tie_features without specials: small integers (many ties), half of the zeros negative"""
    X = torch.randint(-3, 4, (rows, D), device=dev, generator=gen).float()
    X[(X == 0) & (torch.rand((rows, D), device=dev, generator=gen) < 0.5)] = -0.0
    return X


def _beta_d(D, dev):
    return torch.from_numpy(_beta("vector", D)).to(dev)


# ------------------------------------------------------------------------------------------- coverage
def _wave_spans(lens, R):
    """(shortest, longest) task of every wave of R consecutive descriptors; a descriptor the last wave lacks counts as 0"""
    pad = (-len(lens)) % R
    w = np.concatenate([lens, np.zeros(pad, lens.dtype)]).reshape(-1, R)
    return w.min(1), w.max(1)


def test_every_cell_is_past_its_gate(fe, dev):
    """none of this is a measurement: rebuilding a plan small, or removing a cell, fails here"""
    scale._assert_defaults()
    assert set(CELLS) == set(EXPECTED) and len(CELLS) == len(EXPECTED)
    assert all(EXT_CELL[f] in EXPECTED and FRAME_CELL[f] in EXPECTED for f in FAMILIES)
    table, mixed = {}, {}
    for form, D in CELLS:
        g = _plan(fe, dev, form)
        h = scale._header(g)
        panel = _panel_cols(h, D)
        thr = fe.wide_threshold(g["row_nzr"], D)
        table[form, D] = (panel, scale._pick_L(panel, 4), thr)
        limit = scale._seq_limit(g, D)
        print("cell %-9s D=%-3d panel %3d L %2d wide threshold %3d sequential limit %3d | n_slices %d slice_threshold %d "
              "n_slice_tasks %d n_split_rows %d n_dense %d n_tiny %d n_tasks %d nnz_sparse %d"
              % (form, D, panel, table[form, D][1], thr, limit, h.n_slices, h.slice_threshold, h.n_slice_tasks, h.n_split_rows,
                 h.n_dense, h.n_tiny, h.n_tasks, h.nnz_sparse))
        assert h.panel_cols == (-1 if form == "one_pass" else 0), (form, h.panel_cols)
        assert thr >= 32 and limit == (min(thr, h.slice_threshold) if h.n_slices else thr) <= 256, (form, D, thr, limit)
        for lo, hi in scale.LENGTH_CLASSES:  # every length class one lane group sums in this cell is well filled
            if hi <= limit:
                assert int(((g["deg"] > lo) & (g["deg"] <= hi)).sum()) > 1000, (form, D, lo, hi)
        # the waves of the ordinary region, from the plan's own task list: descriptors (row, first entry, length, slot), the
        # wide tasks (longer than the threshold) a prefix, the tiny ones a suffix; R = 64 / L consecutive ones share a wave
        words = g["row_nzr"].cpu().numpy()
        tasks = words[h.off_tasks:h.off_tasks + 4 * h.n_tasks].reshape(-1, 4)
        n_wide = h.n_len_gt[(16, 32, 64, 128, 256).index(thr)] if thr != NO_WIDE_TASK else 0
        ordinary = tasks[n_wide:h.n_tasks - h.n_tiny, 2]
        if thr == NO_WIDE_TASK:
            assert h.n_len_gt[4] == 0 and h.n_slices > 0 and h.slice_threshold == 256, (form, D)
        else:
            assert n_wide > 0 and tasks[:n_wide, 2].min() > thr, (form, D)
        assert 2 < ordinary.min() and limit * 3 // 4 < ordinary.max() <= limit, (form, D)
        L = table[form, D][1]
        R = 64 // L
        lo, hi = _wave_spans(ordinary, R)
        chunks = lambda n: (n + L - 1) // L  # noqa: E731  (index chunks of a task: the task bodies' STRIDE is L)
        idle = int((chunks(hi) - chunks(lo))[lo > 0].max())
        print("    ordinary region: %d tasks, %d waves of %d; longest task %d = %d index chunks; in one wave: largest (longest - "
              "shortest) %d entries, %d chunks; waves mixing <= 4 with > 64 entries: %d"
              % (len(ordinary), len(lo), R, int(ordinary.max()), chunks(int(ordinary.max())), int((hi - lo)[lo > 0].max()), idle,
                 int(((lo <= 4) & (hi > 64) & (lo > 0)).sum())))
        # a third chunk at L = 8, a second one at L = 16 and 32 (a first one is all the small graphs' planned launches take) ...
        assert chunks(int(ordinary.max())) >= (3 if L == 8 else 2), (form, D)
        # ... and a wave in which a lane group has no entry left (idx = -1 in every lane) for a whole chunk another still sums
        assert idle >= 1, (form, D)
        if h.n_slices:
            table_s = words[h.off_slice_table:h.off_slice_table + h.n_slices + 1]
            pieces = words[h.off_slice_tasks:h.off_slice_tasks + 4 * h.n_slice_tasks].reshape(-1, 4)
            n_mixed = 0
            for s in range(h.n_slices):
                ln = np.where(pieces[table_s[s]:table_s[s + 1], 0] >= 0, pieces[table_s[s]:table_s[s + 1], 2], 0)
                plo, phi = _wave_spans(ln, R)
                n_mixed += int(((plo <= 4) & (phi > 64)).sum())
            print("    sliced region: %d pieces in %d lists, longest %d; waves mixing <= 4 with > 64 entries: %d"
                  % (h.n_slice_tasks, h.n_slices, int(pieces[:, 2].max()), n_mixed))
            mixed[form, D] = n_mixed
    print("cells as queried: %s" % table)
    assert table == EXPECTED
    assert all(c[2] >= 32 for c in table.values())
    for L in (8, 16, 32):
        assert any(c[1] == L and 64 <= c[2] <= 256 for c in table.values()), L
    assert {c[2] for c in table.values()} >= {32, 64, 128, 256}
    assert set(mixed) == {("auto", 32), ("auto", 256), ("one_pass", 64), ("one_pass", 128)}  # the cells with a sliced region
    h = scale._header(_plan(fe, dev, "no_slices"))
    assert h.n_slices == 0
    for form in ("auto", "one_pass"):
        h = scale._header(_plan(fe, dev, form))
        assert h.n_slices > 0 and h.n_slice_tasks > 0 and h.n_split_rows > 0, form
    assert h.num_columns * 256 * 4 > 256 * 1048576  # X at D = 256 is beyond the Infinity Cache: gate C
    g = _plan(fe, dev, "auto")
    assert int((g["deg"] == 0).sum()) > 0  # rows without entries: the framed tests look at them
    assert int(g["deg"].max()) * 64 < 2 ** 24  # integer messages up to 64: every partial sum is an integer fp32 holds


# ------------------------------------------------------------------------------------------- multi-aggregate
def _multi_int_refs(g, D, dev, specials):
    def make():
        gen = _gen(dev, 1100 + D + (300 if specials else 0))
        X = scale._tie_features(gen, g["N"], D, dev) if specials else _int_features(gen, g["N"], D, dev)
        r = dict(max=scale._extremum_reference(g, X, "max"), min=scale._extremum_reference(g, X, "min"))
        if not specials:
            def terms(sl):
                v = X[:, sl][g["cols"]]
                return v.double(), (v * v).double()
            r["sum"], r["sumsq"] = (t.float() for t in _fp64_sums(g, D, terms, 2))  # integers: exact, and +0 where empty
        return X, r
    return _cached(("multi", "special" if specials else "int", D), make)


def _check_extrema(out, r, tag):
    for k, name in ((2, "max"), (3, "min")):
        assert torch.equal(out[k + 2], r[name][1]), tag + (name, "arg")
        assert _same_bits(out[k], r[name][0]), tag + (name,)


@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_multi_all_six_outputs_bit_for_bit_on_integer_data(fe, dev, form, D):
    """test_multi_aggr_gpu's: sums exact, max / min bits, arg ties to the lowest entry -- across index chunks here"""
    g = _plan(fe, dev, form)
    X, r = _multi_int_refs(g, D, dev, False)
    out = fe.forward_multi(X, *g["args"])
    assert len(out) == 6 and all(o.shape == (g["N"], D) and o.is_contiguous() for o in out)
    assert [o.dtype for o in out] == [torch.float32] * 4 + [torch.int32] * 2
    _check_extrema(out, r, (form, D))
    assert _same_bits(out[0], r["sum"]), (form, D, "sum")
    assert _same_bits(out[1], r["sumsq"]), (form, D, "sumsq")


@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_multi_specials_keep_the_extremum_contract(fe, dev, form, D):
    """2 % NaN, 2 % +-inf, signed zeros: max, min and both args stay bit-exact (the sums are not compared here)"""
    g = _plan(fe, dev, form)
    X, r = _multi_int_refs(g, D, dev, True)
    _check_extrema(fe.forward_multi(X, *g["args"]), r, (form, D))


def _multi_randn_refs(g, D, dev):
    def make():
        X = torch.randn((g["N"], D), device=dev, generator=_gen(dev, 1700 + D))

        def terms(sl):
            v = X[:, sl][g["cols"]]
            v64 = v.double()
            return v64, (v * v).double(), v64.abs(), v64 * v64
        return (X,) + tuple(_fp64_sums(g, D, terms, 4))
    return _cached(("multi", "randn", D), make)


@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_multi_continuous_data_bounds_and_determinism(fe, dev, form, D):
    """randn: sum within 1e-5 * sum|x| and sumsq within 1e-5 * sum x^2 of fp64, per element; max / min / args the bits of
    forward_max / forward_min (pinned at this scale by test_scale_paths_gpu); two calls give the same bits"""
    g = _plan(fe, dev, form)
    X, s64, q64, a64, sq64 = _multi_randn_refs(g, D, dev)
    limit = scale._seq_limit(g, D)
    out = fe.forward_multi(X, *g["args"])
    _check_elementwise_bound("multi", "sum", out[0], s64, 1e-5 * a64, g, limit, (form, D))
    _check_elementwise_bound("multi", "sumsq", out[1], q64, 1e-5 * sq64, g, limit, (form, D))
    for a, b in zip(out, fe.forward_multi(X, *g["args"])):
        assert _same_bits(a, b), (form, D)
    zx, ax = fe.forward_max(X, *g["args"])
    zn, an = fe.forward_min(X, *g["args"])
    for a, b in ((out[2], zx), (out[3], zn), (out[4], ax), (out[5], an)):
        assert _same_bits(a, b), (form, D)


# ------------------------------------------------------------------------------------------- softmax aggregation
@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_softmax_exact_cases_on_integer_data(fe, dev, form, D):
    """integers in [-3, 3]: beta = 1000 gives forward_max's values and beta = -1000 forward_min's, everything finite (the
    running maximum carried over hundreds of entries by one lane group); beta = 0 gives L = the row length and M = 0 exactly
    and Z within 1 ulp of fl(sum / n)"""
    g = _plan(fe, dev, form)
    X = torch.randint(-3, 4, (g["N"], D), device=dev, generator=_gen(dev, 4000 + D)).float()
    nonempty = g["deg_d"] > 0
    for beta, ext in ((1000.0, fe.forward_max), (-1000.0, fe.forward_min)):
        Z, M, L, Q = fe.forward_softmax(X, beta, *g["args"])
        tag = (form, D, beta)
        assert _same_bits(Z, ext(X, *g["args"], return_arg=False)[0]), tag
        assert all(bool(torch.isfinite(t).all()) for t in (Z, L, Q, M[nonempty])), tag
        assert torch.equal(M[nonempty], beta * Z[nonempty]) and torch.equal(Q, Z * Z), tag
    Z, M, L, Q = fe.forward_softmax(X, 0.0, *g["args"])
    tag = (form, D, 0.0)
    assert torch.equal(L, g["deg_d"].float()[:, None].expand_as(L)), tag
    assert bool((M[nonempty] == 0).all()) and bool(torch.isneginf(M[~nonempty]).all()), tag
    total = _fp64_sums(g, D, lambda sl: (X[:, sl][g["cols"]].double(),), 1)[0]
    mean = (total / g["deg_d"].clamp(min=1).double()[:, None]).float()
    ulp = torch.nextafter(mean.abs(), torch.full_like(mean, float("inf"))) - mean.abs()
    assert bool(((Z - mean).abs() <= ulp).all()), tag


def _softmax_refs(g, D, dev):
    def make():
        X = torch.randn((g["N"], D), device=dev, generator=_gen(dev, 2000 + D))
        b = _beta_d(D, dev)
        rows, cols, N, E = g["rows"], g["cols"], g["N"], g["E"]
        M = torch.empty((N, D), device=dev)
        for c0 in range(0, D, 16):  # max over each row of fl32(beta x), -inf on rows without entries: exact
            sl = slice(c0, min(c0 + 16, D))
            s = X[:, sl][cols] * b[sl]
            M[:, sl] = torch.full((N, s.size(1)), float("-inf"), device=dev).scatter_reduce_(
                0, rows[:, None].expand(E, s.size(1)).contiguous(), s, "amax", include_self=True)

        def terms(sl):
            x = X[:, sl][cols]
            w = torch.exp((x * b[sl]).double() - M[:, sl][rows].double())
            x = x.double()
            return w, w * x, w * (x * x)

        def term32(r, e):  # test_softmax_aggr_gpu.forward_reference in fp32, sequential sums
            x = X[cols[e]]
            w = torch.exp(x * b - M[r])
            return torch.cat([w, w * x, w * (x * x)], 1)
        L64, S64, Q64 = _fp64_sums(g, D, terms, 3)
        safe = torch.where(L64 > 0, L64, torch.ones_like(L64))
        acc = _sequential(g, 3 * D, term32)
        L32 = acc[:, :D]
        safe32 = torch.where(L32 > 0, L32, torch.ones_like(L32))
        return X, b, M, dict(Z=_yard(S64 / safe, acc[:, D:2 * D] / safe32), L=_yard(L64, L32), Q=_yard(Q64 / safe, acc[:, 2 * D:] / safe32))
    return _cached(("softmax", D), make)


@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_softmax_forward_on_continuous_data(fe, dev, form, D):
    """randn features, the per-column beta vector: M equal to max fl32(beta x) everywhere; Z, L, Q within 4 x the fp32
    yardstick's error + 1e-6 max|ref| of fp64, per row group; two calls give the same bits"""
    g = _plan(fe, dev, form)
    X, b, M, yards = _softmax_refs(g, D, dev)
    limit = scale._seq_limit(g, D)
    out = fe.forward_softmax(X, b, *g["args"])
    assert len(out) == 4 and all(o.shape == (g["N"], D) and o.is_contiguous() and o.dtype == torch.float32 for o in out)
    assert torch.equal(out[1], M), (form, D)
    for o, name in ((out[0], "Z"), (out[2], "L"), (out[3], "Q")):
        _check_yard_bound("softmax", name, o, yards[name], g, limit, (form, D))
    for x, y in zip(out, fe.forward_softmax(X, b, *g["args"])):
        assert _same_bits(x, y), (form, D)


def _softmax_backward_operands(g, D, dev):
    """test_softmax_aggr_gpu._backward_refs' synthetic operands: any G and Z, L >= 1, and M at or above every beta x of its
    column, so the exponent is never positive"""
    gen = _gen(dev, 3000 + D)
    N = g["N"]
    X = torch.randn((N, D), device=dev, generator=gen)
    b = _beta_d(D, dev)
    G = torch.randn((N, D), device=dev, generator=gen)
    Z = torch.randn((N, D), device=dev, generator=gen)
    L = 1.0 + 19.0 * torch.rand((N, D), device=dev, generator=gen)
    M = (X * b).amax(0, keepdim=True) + 0.5 * torch.rand((N, D), device=dev, generator=gen)
    return X, b, G, Z, M, L


def _softmax_backward_refs(g, D, dev):
    def make():
        X, b, G, Z, M, L = _softmax_backward_operands(g, D, dev)
        rows, cols = g["rows"], g["cols"]
        S = X * b  # fl32(beta x), as the kernels and the forward form it

        def terms(sl):
            x, bt = X[:, sl][rows].double(), b[sl].double()
            w = torch.exp(S[:, sl][rows].double() - M[:, sl][cols].double()) / L[:, sl][cols].double()
            return (w * G[:, sl][cols].double() * (1 + bt * (x - Z[:, sl][cols].double())),)

        def term32(r, e):  # test_softmax_aggr_gpu.backward_reference in fp32
            c, x = cols[e], X[r]
            return torch.exp(S[r] - M[c]) / L[c] * G[c] * (1 + b * (x - Z[c]))
        return X, b, G, Z, M, L, _yard(_fp64_sums(g, D, terms, 1)[0], _sequential(g, D, term32))
    return _cached(("softmax_backward", D), make)


@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_softmax_backward_on_continuous_data(fe, dev, form, D):
    """softmax_backward as the function of its operands that hcspmm.h states, this graph the walked one: dX within the
    forward's bound; two calls give the same bits"""
    g = _plan(fe, dev, form)
    X, b, G, Z, M, L, yard = _softmax_backward_refs(g, D, dev)
    dX = fe.softmax_backward(G, Z, M, L, X, b, *g["args"])
    assert dX.shape == (g["N"], D) and dX.dtype == torch.float32 and dX.is_contiguous()
    _check_yard_bound("softmax_backward", "dX", dX, yard, g, scale._seq_limit(g, D), (form, D))
    assert _same_bits(dX, fe.softmax_backward(G, Z, M, L, X, b, *g["args"])), (form, D)


# ------------------------------------------------------------------------------------------- edge-feature messages
def _f_index(g, dev):
    return torch.randint(0, F_ROWS, (g["E"],), device=dev, generator=_gen(dev, 140)).int()


def _messages(op, xc, fe_):
    """test_edge_messages_gpu._messages: the per-entry messages in the operands' dtype"""
    if op == "mul":
        return xc * fe_
    if op == "add_relu":
        return (xc + fe_).clamp(min=0)
    return fe_


def _edge_int_operands(g, D, dev):
    gen = _gen(dev, 141 + D)
    return (torch.randint(-8, 9, (g["N"], D), device=dev, generator=gen).float(),
            torch.randint(-8, 9, (F_ROWS, D), device=dev, generator=gen).float(), _f_index(g, dev))


@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_edge_messages_integer_sums_are_exact_on_every_row(fe, dev, form, D):
    """integers in [-8, 8], F a table of 4096 rows behind a random int32 f_index: |m| <= 64, so every partial sum is an
    integer fp32 holds in any order (the coverage test has the longest row) -- exact on ALL rows"""
    g = _plan(fe, dev, form)

    def make():
        X, F, fi = _edge_int_operands(g, D, dev)
        fl = fi.long()

        def terms(sl):  # (one gather for the three ops)
            xc, f = X[:, sl][g["cols"]].double(), F[:, sl][fl].double()
            return [_messages(op, xc, f) for op in OPS]
        return X, F, fi, [t.float() for t in _fp64_sums(g, D, terms, 3)]
    X, F, fi, wants = _cached(("edge", "int", D), make)
    for op, want in zip(OPS, wants):
        got = fe.forward_edge_messages(None if op == "copy" else X, F, *g["args"], op, fi)[0]
        assert got.shape == (g["N"], D) and got.dtype == torch.float32
        assert torch.equal(got, want), (form, D, op)


@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_edge_messages_unsplit_rows_have_the_bits_of_the_csr_recurrence(fe, dev, form, D):
    """dyadic data (12-bit X, 8-bit F: products exact, so fmaf rounds once, as the recurrence does): the rows one lane group
    sums -- not wide, not split, not sliced -- have the bits of the sequential fp32 sum in CSR order, whatever the number of
    index chunks.  The sharpest pin on order and chunk boundaries"""
    g = _plan(fe, dev, form)
    limit = scale._seq_limit(g, D)
    gen = _gen(dev, 142 + D)
    X, F = scale._short(gen, (g["N"], D), 12, dev), scale._short(gen, (F_ROWS, D), 8, dev)
    fi = _f_index(g, dev)
    fl, cols = fi.long(), g["cols"]
    ordered = g["deg_d"] <= limit
    assert int(ordered.sum()) >= int((g["deg"] <= 32).sum())
    zero = torch.zeros((), device=dev)
    recurrence = {"mul": lambda r, e: F[fl[e]] * X[cols[e]],
                  "add_relu": lambda r, e: torch.where(X[cols[e]] + F[fl[e]] < 0, zero, X[cols[e]] + F[fl[e]]),
                  "copy": lambda r, e: F[fl[e]]}
    for op in OPS:
        got = fe.forward_edge_messages(X, F, *g["args"], op, fi)[0]
        want = _sequential(g, D, recurrence[op], limit=limit)
        assert _same_bits(got[ordered], want[ordered]), (form, D, op, limit)


@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_edge_messages_normal_data_within_the_rounding_bound(fe, dev, form, D):
    """test_edge_messages_gpu's bound: |got - exact| <= k u / (1 - k u) * sum |m|, k the row length (+ 2 for add_relu: the
    entry's own add, then the sum)"""
    g = _plan(fe, dev, form)

    def make():
        gen = _gen(dev, 143 + D)
        X = torch.randn((g["N"], D), device=dev, generator=gen)
        F = torch.randn((F_ROWS, D), device=dev, generator=gen)
        fi = _f_index(g, dev)
        fl = fi.long()

        def terms(sl):  # (one gather for the three ops) exact messages, then what the bound scales with: |x f|, |x + f|, |f|
            xc, f = X[:, sl][g["cols"]].double(), F[:, sl][fl].double()
            return [_messages(op, xc, f) for op in OPS] + [(xc * f).abs(), (xc + f).abs(), f.abs()]
        return X, F, fi, _fp64_sums(g, D, terms, 6)
    X, F, fi, sums = _cached(("edge", "randn", D), make)
    deg = g["deg_d"].double()[:, None]
    limit = scale._seq_limit(g, D)
    for i, op in enumerate(OPS):
        exact, mag = sums[i], sums[3 + i]
        k = deg + 2 if op == "add_relu" else deg
        got = fe.forward_edge_messages(X, F, *g["args"], op, fi)[0]
        _check_elementwise_bound("edge", op, got, exact, k * U / (1 - k * U) * mag, g, limit, (form, D))


# ------------------------------------------------------------------------------------------- gated aggregation
def _checker(n, D, dev, offset=0):
    i, d = torch.arange(n, device=dev)[:, None], torch.arange(D, device=dev)[None, :]
    return torch.where((i + d + offset) % 2 == 0, 200.0, -200.0).float()


@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_gated_saturated_gates_select_exactly(fe, dev, form, D):
    """test_z_gated_gpu's pins: integer V and gates of +-200.  In P (Q = 0): Z_gate is the integer neighbour sum where P is
    +200 and exactly +0 where it is -200 (the own-row lookup).  In Q (P = 0): the integer sum over the selected neighbours
    (the gathered-row lookup).  Z_dgate is exactly +0 both times"""
    g = _plan(fe, dev, form)
    N, cols = g["N"], g["cols"]
    V = torch.randint(-3, 4, (N, D), device=dev, generator=_gen(dev, 7100 + D)).float()
    zero = torch.zeros((N, D), device=dev)
    own, sel = _checker(N, D, dev), _checker(N, D, dev, 1)

    def terms(sl):
        v = V[:, sl][cols].double()
        return v, torch.where(sel[:, sl][cols] > 0, v, torch.zeros_like(v))
    sums, picked = (t.float() for t in _fp64_sums(g, D, terms, 2))
    Zg, Zd = fe.forward_gated(own, zero, V, *g["args"], outputs=("gate", "dgate"))
    assert _same_bits(Zg, torch.where(own > 0, sums, zero) + 0.0), (form, D, "P")
    assert _is_plus_zero(Zd), (form, D, "P")
    Zg, Zd = fe.forward_gated(zero, sel, V, *g["args"], outputs=("gate", "dgate"))
    assert _same_bits(Zg, picked + 0.0), (form, D, "Q")
    assert _is_plus_zero(Zd), (form, D, "Q")


def _gated_operands(g, D, dev, seed=7000):
    gen = _gen(dev, seed + D)
    N = g["N"]
    return (2.0 * torch.randn((N, D), device=dev, generator=gen), 2.0 * torch.randn((N, D), device=dev, generator=gen),
            torch.randn((N, D), device=dev, generator=gen))


def _gate(z):
    """test_z_gated_gpu.gated_reference in z's dtype: (sigma, sigma') from t = exp(-|z|), r = 1 / (1 + t)"""
    t = torch.exp(-z.abs())
    r = 1 / (1 + t)
    tr = t * r
    return torch.where(z >= 0, r, tr), tr * r


def _gated_refs(g, D, dev):
    def make():
        P, Q, V = _gated_operands(g, D, dev)
        rows, cols = g["rows"], g["cols"]

        def terms(sl):
            s, ds = _gate((P[:, sl][rows] + Q[:, sl][cols]).double())  # one fp32 add, then widened
            v = V[:, sl][cols].double()
            return s * v, ds * v

        def term32(r, e):
            c = cols[e]
            s, ds = _gate(P[r] + Q[c])
            return torch.cat([s * V[c], ds * V[c]], 1)
        r64 = _fp64_sums(g, D, terms, 2)
        acc = _sequential(g, 2 * D, term32)
        return P, Q, V, dict(gate=_yard(r64[0], acc[:, :D]), dgate=_yard(r64[1], acc[:, D:]))
    return _cached(("gated", D), make)


@pytest.mark.parametrize("form,D", CELLS, ids=CELL_IDS)
def test_gated_both_outputs_on_continuous_data(fe, dev, form, D):
    """randn V, 2 randn P and Q: both outputs within 4 x the fp32 yardstick's error + 1e-6 max|ref| of fp64, per row group;
    two calls give the same bits, and a single-output call has the bits of the two-output call"""
    g = _plan(fe, dev, form)
    P, Q, V, yards = _gated_refs(g, D, dev)
    limit = scale._seq_limit(g, D)
    both = fe.forward_gated(P, Q, V, *g["args"], outputs=("gate", "dgate"))
    assert len(both) == 2 and all(o.shape == (g["N"], D) and o.is_contiguous() and o.dtype == torch.float32 for o in both)
    for o, name in zip(both, ("gate", "dgate")):
        _check_yard_bound("gated", name, o, yards[name], g, limit, (form, D))
    again = fe.forward_gated(P, Q, V, *g["args"], outputs=("gate", "dgate"))
    assert _same_bits(both[0], again[0]) and _same_bits(both[1], again[1]), (form, D)
    gate = fe.forward_gated(P, Q, V, *g["args"])  # the default: Z_gate alone
    dgate = fe.forward_gated(P, Q, V, *g["args"], outputs=("dgate",))
    assert gate[1] is None and dgate[0] is None
    assert _same_bits(both[0], gate[0]) and _same_bits(both[1], dgate[1]), (form, D)


def test_gated_operands_as_column_blocks_of_one_projection(fe, dev):
    """P, Q and V as column blocks of one [N, 4 D] tensor at D = 32, as ResGatedGraphConv hands them over: the contiguous
    call's bits"""
    form, D = "auto", 32
    g = _plan(fe, dev, form)
    P, Q, V = _gated_operands(g, D, dev)
    proj = torch.randn((g["N"], 4 * D), device=dev, generator=_gen(dev, 7600))
    blocks = [proj[:, k * D:(k + 1) * D] for k in range(3)]
    for blk, src in zip(blocks, (P, Q, V)):
        blk.copy_(src)
    assert blocks[1].stride(0) == 4 * D and not blocks[1].is_contiguous()
    want = fe.forward_gated(P, Q, V, *g["args"], outputs=("gate", "dgate"))
    got = fe.forward_gated(*blocks, *g["args"], outputs=("gate", "dgate"))
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])


# ------------------------------------------------------------------------------------------- both front-ends
def _launch(family, f, g, D, dev):
    """the family's launch on seeded operands (made on the device: no reference is needed here) -> its outputs"""
    if family == "multi":
        return f.forward_multi(torch.randn((g["N"], D), device=dev, generator=_gen(dev, 1700 + D)), *g["args"])
    if family == "softmax":
        return f.forward_softmax(torch.randn((g["N"], D), device=dev, generator=_gen(dev, 2000 + D)), _beta_d(D, dev), *g["args"])
    if family == "softmax_backward":
        X, b, G, Z, M, L = _softmax_backward_operands(g, D, dev)
        return [f.softmax_backward(G, Z, M, L, X, b, *g["args"])]
    if family == "edge":
        X, F, fi = _edge_int_operands(g, D, dev)
        Xr = torch.randn((g["N"], D), device=dev, generator=_gen(dev, 143 + D))
        return [f.forward_edge_messages(Xr if op == "mul" else X, F, *g["args"], op, fi)[0] for op in OPS]
    return f.forward_gated(*_gated_operands(g, D, dev), *g["args"], outputs=("gate", "dgate"))


@pytest.mark.parametrize("family", FAMILIES)
def test_the_extension_gives_the_ctypes_bits(dev, family):
    """one cell per family through the torch extension, on its own plan of the same graph: the ctypes front-end's bits, which
    the tests above pin"""
    form, D = EXT_CELL[family]
    fc, fx = frontends.get("ctypes"), frontends.get("extension")
    gc, gx = _plan(fc, dev, form), _plan(fx, dev, form)
    assert torch.equal(gc["ht"], gx["ht"]) and fc.wide_threshold(gc["row_nzr"], D) == fx.wide_threshold(gx["row_nzr"], D)
    a, b = _launch(family, fc, gc, D, dev), _launch(family, fx, gx, D, dev)
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and _same_bits(x, y), (family, form, D, k)


# ------------------------------------------------------------------------------------------- framed operands
def _in_a_nan_frame(t, left, right):
    """a view with t's values inside a wider matrix that is NaN everywhere else"""
    wide = torch.full((t.size(0), left + t.size(1) + right), float("nan"), device=t.device)
    wide[:, left:left + t.size(1)] = t
    return wide[:, left:left + t.size(1)]


def _guarded(dev, N, D, n=1, dtype=torch.float32):
    """n sentinel-filled [N, D + 9] buffers and the pointers of their inner blocks, 5 elements in (off the 16-byte grid)"""
    bufs = [torch.full((N, D + 9), SENTINEL, dtype=dtype, device=dev) for _ in range(n)]
    return bufs, [b[:, 5:].data_ptr() for b in bufs]


def _check_guarded(bufs, full, D, tag):
    for k, (b, want) in enumerate(zip(bufs, full)):
        assert bool((b[:, :5] == SENTINEL).all()) and bool((b[:, 5 + D:] == SENTINEL).all()), tag + (k, "guard columns")
        assert _same_bits(b[:, 5:5 + D], want), tag + (k,)  # (every element of the slice written: an unwritten one keeps -777)


def _raw(g, D, src_rows, dev, ws_fn, launch):
    """one C entry point with raw pointers: launch(lib, c) with c the _planned_call of this graph and width"""
    c = hcspmm._planned_call(g["args"][:6], g["args"][6], D, src_rows, dev, ws_fn=ws_fn)
    with c:
        rc = launch(capi.lib(), c)
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("family", FAMILIES)
def test_framed_operands_every_row_written_and_nothing_else(fe, dev, family):
    """one cell per family, through the C entry points: every input a view inside a NaN-filled wider matrix, every output
    inside a sentinel-filled one (ldz = D + 9, its base 5 elements in).  The contiguous call's bits -- so nothing outside an
    input view is read -- in every row of the slice, the sentinel everywhere around it, and +0 (M: -inf, args: -1) in the rows
    without entries"""
    form, D = FRAME_CELL[family]
    g = _plan(fe, dev, form)
    N, ld, vp = g["N"], D + 9, ctypes.c_void_p
    empty = g["deg_d"] == 0
    assert bool(empty.any())
    tag = (family, form, D)
    if family == "multi":
        X = _int_features(_gen(dev, 1100 + D), N, D, dev)
        full = fe.forward_multi(X, *g["args"])
        zb, zp = _guarded(dev, N, D, 4)
        ab, ap = _guarded(dev, N, D, 2, torch.int32)
        _multi_direct(g, _in_a_nan_frame(X, 5, 8), D, zp, ld, ap, ld)
        _check_guarded(zb + ab, full, D, tag)
        assert all(_is_plus_zero(o[empty]) for o in full[:4]) and all(bool((o[empty] == -1).all()) for o in full[4:]), tag
    elif family == "softmax":
        X = torch.randn((N, D), device=dev, generator=_gen(dev, 2000 + D))
        b = _beta_d(D, dev)
        full = fe.forward_softmax(X, b, *g["args"])
        zb, zp = _guarded(dev, N, D, 4)
        _softmax_direct(g, _in_a_nan_frame(X, 5, 8), b, D, zp, ld)
        _check_guarded(zb, full, D, tag)
        assert all(_is_plus_zero(full[k][empty]) for k in (0, 2, 3)) and bool(torch.isneginf(full[1][empty]).all()), tag
    elif family == "softmax_backward":
        X, b, G, Z, M, L = _softmax_backward_operands(g, D, dev)
        full = [fe.softmax_backward(G, Z, M, L, X, b, *g["args"])]
        Gv, Zv, Mv, Lv = (_in_a_nan_frame(t, 3, 10) for t in (G, Z, M, L))  # (the four share one leading dimension)
        Xv = _in_a_nan_frame(X, 5, 8)
        zb, zp = _guarded(dev, N, D)
        _raw(g, D, N, dev, hcspmm._ws_bytes, lambda lib, c: lib.hcspmm_softmax_backward(
            vp(Gv.data_ptr()), vp(Zv.data_ptr()), vp(Mv.data_ptr()), vp(Lv.data_ptr()), Gv.stride(0), N, vp(Xv.data_ptr()), Xv.stride(0),
            vp(b.data_ptr()), vp(zp[0]), ld, *c.graph, *c.ws))
        _check_guarded(zb, full, D, tag)
        assert _is_plus_zero(full[0][empty]), tag
    elif family == "edge":
        X, F, fi = _edge_int_operands(g, D, dev)
        Xv, Fv = _in_a_nan_frame(X, 5, 8), _in_a_nan_frame(F, 3, 4)
        for op in OPS:
            full = fe.forward_edge_messages(X, F, *g["args"], op, fi)
            zb, zp = _guarded(dev, N, D)
            _raw(g, D, N, dev, hcspmm._ws_bytes, lambda lib, c: lib.hcspmm_forward_edge_messages(
                vp(Xv.data_ptr()), N, Xv.stride(0), vp(Fv.data_ptr()), F_ROWS, Fv.stride(0), vp(fi.data_ptr()), hcspmm.EDGE_OPS[op],
                vp(zp[0]), ld, *c.graph, *c.ws))
            _check_guarded(zb, full, D, tag + (op,))
            assert _is_plus_zero(full[0][empty]), tag + (op,)
    else:
        P, Q, V = _gated_operands(g, D, dev)
        full = fe.forward_gated(P, Q, V, *g["args"], outputs=("gate", "dgate"))
        zb, zp = _guarded(dev, N, D, 2)
        _gated_direct(g, _in_a_nan_frame(P, 5, 8), _in_a_nan_frame(Q, 3, 4), _in_a_nan_frame(V, 1, 6), D, zp, ld)
        _check_guarded(zb, full, D, tag)
        assert all(_is_plus_zero(o[empty]) for o in full), tag
    assert not any(bool(torch.isnan(o.float()).any()) for o in full), tag
