"""The launch paths that only large graphs reach, at their shipped defaults, on an MI355X through both Python front-ends.

Several launchers pick another kernel, or another loop inside a kernel, once the graph is large enough; on the graphs of the
sibling files (1 200 - 16 000 rows) every one of these decisions falls the same way.  The gates, and what runs behind them:

  A  own tiny launch (spmm_impl.h own_tiny_launch): n_tiny >= 524 288 -> tiny_kernel / tiny_w_kernel / tiny_wh_kernel;
  B  wide threshold (capi.hip wide_choice): 32 ... 256 -> rows of 17 ... 256 entries summed by ONE lane group in CSR order
     (the small graphs reach such rows only where a wave is a single lane group, L = 64, and no task is wide);
  C  panel width (capi.hip panel_choice): X beyond 256 MiB -> two cache lines per gathered row and pass;
  D  automatic column slices (plan_host.cpp): the XCD-affine sliced region without being asked;
  E  GATv2 backward tiles (gatv2_attention.hip kGradMaxBlocks): more than 4096 tiles -> a workgroup walks several;
  F  edge_norm grid cap (spmm_weighted.hip): more than 65 536 * 256 entries -> second round of the grid-stride loop.
Gates B, C and D for the other users of the shared CSR walk (multi-aggregate, softmax aggregation and its backward, edge
messages, gated aggregation) are test_z_scale_walk_gpu.py's, on this module's power-law graph.

The coverage tests assert, through the library's own queries, that every graph below really is on the far side of its gate
(no environment override: the shipped defaults are the subject).  The value tests restate the criteria of the sibling files
(test_spmm_gpu._check / _check_h16, the four checks of test_weighted_gpu, test_heads_gpu, test_extremum_gpu, the three bounds
of test_gatv2_gpu); none is new, except the fp16 form of the gamma_n bound, derived where it is used.  References that the
host oracle cannot finish quickly at these sizes are plain torch on the device: fp64 products summed by index_add, and for
the CSR-order checks a sequential fp32 sum, one CSR position at a time (products exact by construction, one rounding per add).
"""
import math
import os

import numpy as np
import pytest
import torch

import frontends
import hcspmm
from hcspmm import capi, graphs

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126
SLOPE = 0.2
SLOPE64 = float(np.float32(SLOPE))
OVERRIDES = ("HCSPMM_TINY_KERNEL_MIN_TASKS", "HCSPMM_PANEL_COLS", "HCSPMM_SLICE_THRESHOLD", "HCSPMM_SLICES")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
_IBITS = {F32: torch.int32, F16: torch.int16, BF16: torch.int16}


@pytest.fixture(scope="module", params=["ctypes", "extension"])
def fe(request):
    return frontends.get(request.param)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


def _free(*_):
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- graphs
def _short_rows(N, seed=9):
    """test_spmm_gpu._tiny_graph's recipe, vectorised: mostly rows of 0, 1 and 2 entries (descriptors with inline indices),
    a sprinkling of longer ones, and three hubs of exactly 513 / 514 / 770 entries (last segments of 1 / 2 / 2 entries)."""
    rng = np.random.default_rng(seed)
    deg = rng.choice([0, 1, 2, 3, 7, 40], size=N, p=[0.35, 0.3, 0.2, 0.1, 0.04, 0.01])
    hubs = {5: 513, N // 2 + 1700: 514, N - 1: 770}
    for r, d in hubs.items():
        deg[r] = d
    rows = np.repeat(np.arange(N, dtype=np.int64), deg)
    cols = rng.integers(0, N, rows.shape[0])
    start = np.concatenate([[0], np.cumsum(deg)])
    for r, d in hubs.items():  # distinct, no self loop: the merge of duplicates must not shorten a hub
        c = rng.choice(N - 1, d, replace=False)
        cols[start[r]:start[r] + d] = c + (c >= r)
    return rows, cols, hubs


def _build(kind):
    if kind == "short_rows":
        rows, cols, hubs = _short_rows(700000)
        rp, col = graphs._to_csr(rows, cols, 700000)
        assert [int(rp[r + 1] - rp[r]) for r in hubs] == list(hubs.values())
        return rp, col
    if kind == "power_law":
        return graphs.powerlaw_graph(300000, 6000000, seed=3, max_degree_frac=0.02)
    if kind == "short_rows_symmetric":  # the pattern of A + A^T of the short-row recipe
        N = 1100000
        rows, cols, _ = _short_rows(N, seed=10)
        return graphs._to_csr(np.concatenate([rows, cols]), np.concatenate([cols, rows]), N)
    raise KeyError(kind)


PLANS = {"auto": {}, "no_slices": dict(slice_threshold=-1), "panel32": dict(panel_cols=32)}
_GRAPHS, _CACHE = {}, {}


def _graph(kind):
    if kind not in _GRAPHS:
        _GRAPHS[kind] = _build(kind)
    return _GRAPHS[kind]


def _setup(fe, dev, kind, form="auto"):
    key = (fe.name, kind, form)
    if key in _CACHE:
        return _CACHE[key]
    rp, col = _graph(kind)
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    bp, e2c, e2r, ht, row_nzr, col_nzr = fe.preprocess(col_d, rp_d, N, E, (N + 15) // 16, rule=3)
    if PLANS[form]:
        row_nzr = fe.build_plan(rp_d, col_d, bp, e2c, ht, **PLANS[form])
    deg = np.diff(rp)
    g = dict(fe=fe, rp=rp, col=col, N=N, E=E, deg=deg, ht=ht, row_nzr=row_nzr, rp_d=rp_d, col_d=col_d,
             args=(rp_d, col_d, bp, e2c, e2r, ht, row_nzr, col_nzr), cols=col_d.long(), deg_d=torch.from_numpy(deg).to(dev),
             rows=torch.repeat_interleave(torch.arange(N, device=dev), torch.from_numpy(deg).to(dev).long()))
    _CACHE[key] = g
    return g


def _header(g):
    return hcspmm.plan_header(g["row_nzr"])  # (reads the plan tensor: serves the plans of both front-ends)


def _seq_limit(g, D, dtype=F32):
    """test_spmm_gpu._seq_limit: rows of at most this many entries are summed in CSR order by one lane group -- not handed
    to a whole wave, not split into segments, not cut into column slices."""
    h = _header(g)
    lim = min(h.split_threshold, g["fe"].wide_threshold(g["row_nzr"], D, dtype))
    return min(lim, h.slice_threshold) if h.n_slices else lim


# ------------------------------------------------------------------------------------------- the dispatch, mirrored
def _pick_vec(dtype, D):
    """capi.hip pick_vec for contiguous, aligned operands"""
    if dtype == F32:
        return 4 if D >= 4 else 2 if D >= 2 else 1
    return 8 if D % 2 == 0 and D >= 32 else 4 if D % 2 == 0 and D >= 4 else 1


def _pick_L(width, vec):
    """spmm_impl.h pick_L"""
    slots, L = (width + vec - 1) // vec, 4
    while L < slots and L < 64:
        L <<= 1
    return L


def _cell(dtype, D, panel=None):
    vec = _pick_vec(dtype, D)
    return (16 if dtype != F32 else 32, vec, _pick_L(D if panel is None else min(panel, D), vec))


F32_WIDTHS = [1, 3, 6, 16, 22, 33, 64, 70, 128, 130, 256]
H16_WIDTHS = [3, 7, 9, 17, 33, 6, 22, 30, 32, 64, 128, 256, 520]
# (plan form, dtype, D): every (element size, VEC, L) build of the one-pass dispatch, and one plan with four column panels
TINY_CASES = [("auto", F32, D) for D in F32_WIDTHS] + [("auto", dt, D) for dt in (F16, BF16) for D in H16_WIDTHS] + \
             [("panel32", F32, 128)]
HEAD_CASES = [("auto", 2, 4), ("auto", 4, 8), ("auto", 4, 16), ("auto", 8, 16), ("auto", 8, 32), ("auto", 3, 4), ("panel32", 8, 16)]
_case_id = lambda c: "%s-%s-%s" % (c[0], _NAME.get(c[1], c[1]), c[2])
WIDE_WIDTHS = [16, 32, 64, 128, 256]
LENGTH_CLASSES = [(16, 32), (32, 64), (64, 128), (128, 256), (256, 1 << 30)]
GATV2_SHAPES = [(4, 4), (4, 16), (4, 64), (1, 320)]


# ------------------------------------------------------------------------------------------- coverage
def _assert_defaults():
    """the subject is the shipped defaults: with one of these set the module would silently test something else"""
    found = [k for k in OVERRIDES if k in os.environ]
    assert not found, "unset %s: this module pins the launch decisions the library takes by default at scale" % ", ".join(found)


def test_gate_a_every_tiny_kernel_build_is_reached(fe, dev):
    _assert_defaults()
    for form in ("auto", "panel32"):
        g = _setup(fe, dev, "short_rows", form)
        h = _header(g)
        assert h.n_dense == 0 and not bool(g["ht"].any())
        assert h.n_split_rows == 3 and h.n_slices == 0
        assert h.n_tiny == int((g["deg"] <= 2).sum()) + 3  # (the hubs' last segments)
        assert hcspmm.own_tiny_launch(g["row_nzr"]) is True, "n_tiny = %d does not take the own launch" % h.n_tiny
        assert hcspmm.own_tiny_launch(g["row_nzr"], fused=True) is False  # the fused operators never do
        assert capi.lib().hcspmm_own_tiny_launch(None, 0) == 0
        assert h.nnz_sparse / (h.n_tasks + h.n_slice_tasks) < 8.0  # short rows: capi.hip panel_choice keeps one pass ...
        assert h.panel_cols == PLANS[form].get("panel_cols", 0)   # ... unless the plan names a panel width
    g = _setup(fe, dev, "power_law", "no_slices")
    assert 0 < _header(g).n_tiny < 524288 and hcspmm.own_tiny_launch(g["row_nzr"]) is False  # the query can say no
    # the table reaches every (element size, VEC, L) the dispatch can produce
    for dts, widths in (((F32,), F32_WIDTHS), ((F16, BF16), H16_WIDTHS)):
        for dt in dts:
            possible = {_cell(dt, D) for D in range(1, 1025)}
            assert {_cell(dt, D) for D in widths} == possible, (dt, possible)
    assert {_cell(F32, h * dh) for form, h, dh in HEAD_CASES if form == "auto"} == {(32, 4, L) for L in (4, 8, 16, 32, 64)}
    assert _cell(F32, 128, panel=32) == (32, 4, 8) and math.ceil(128 / 32) == 4  # the panel plan: four column panels


def test_gate_b_every_wide_threshold_is_reached(fe, dev):
    _assert_defaults()
    g = _setup(fe, dev, "power_law", "no_slices")
    assert _header(g).n_slices == 0
    assert {fe.wide_threshold(g["row_nzr"], D) for D in WIDE_WIDTHS} == {16, 32, 64, 128, 256}
    assert len({fe.wide_threshold(g["row_nzr"], D, BF16) for D in WIDE_WIDTHS}) >= 3
    for lo, hi in LENGTH_CLASSES:
        assert int(((g["deg"] > lo) & (g["deg"] <= hi)).sum()) > 1000, (lo, hi)
    # the extremum backward walks A^T through the transpose permutation: the generator's graph is pattern-symmetric
    rows, col = np.repeat(np.arange(g["N"], dtype=np.int64), g["deg"]), g["col"].astype(np.int64)
    assert np.array_equal(np.sort(rows * g["N"] + col), np.sort(col * g["N"] + rows))


def test_gates_c_and_d_wide_panels_and_automatic_slices(fe, dev):
    _assert_defaults()
    g = _setup(fe, dev, "power_law", "auto")
    h = _header(g)
    assert h.n_slices > 0 and h.n_slice_tasks > 0 and h.n_split_rows > 0  # gate D, without being asked
    assert h.panel_cols == 0 and h.nnz_sparse / (h.n_tasks + h.n_slice_tasks) >= 8.0  # panels chosen at launch ...
    assert h.num_columns * 256 * 4 > 256 * 1048576  # ... and X at D = 256 is beyond the Infinity Cache: gate C


def test_gate_e_more_tiles_than_workgroups():
    N, E = len(_graph("short_rows_symmetric")[0]) - 1, len(_graph("short_rows_symmetric")[1])
    deg = np.diff(_graph("short_rows_symmetric")[0])
    assert N > 1048576 and (deg > 256).sum() >= 3 and (deg > 32).sum() > 1000 and (deg == 0).sum() > 1000
    for heads, dh in GATV2_SHAPES:
        D = heads * dh
        assert capi.lib().hcspmm_gatv2_backward_workspace_bytes(N, E, D, heads) == 4096 * D * 4
        assert math.ceil(N / (1024 // _pick_L(D, 4))) > 4096, D


# ------------------------------------------------------------------------------------------- gate A: binary forward
def _check_f32(oracle_mod, g, X, Z):
    """test_spmm_gpu._check"""
    ok, ratio = oracle_mod.check_spmm(Z, g["rp"], g["col"], X)
    assert ok, "relative error %.3g x the 1e-5 bar" % ratio
    seq = g["deg"] <= _seq_limit(g, X.shape[1])
    assert np.array_equal(Z[seq], oracle_mod.spmm_f32(g["rp"], g["col"], X)[seq]), "CSR-order rows differ from the fp32 oracle"
    return seq


def _check_h16(oracle_mod, g, X16, Z16):
    """test_spmm_gpu._check_h16"""
    dtype = X16.dtype
    assert Z16.dtype == dtype
    Xf = X16.float().cpu().numpy()
    want = torch.from_numpy(oracle_mod.spmm_f32(g["rp"], g["col"], Xf)).to(dtype)
    seq = torch.from_numpy(g["deg"] <= _seq_limit(g, Xf.shape[1], dtype))
    got = Z16.cpu()
    assert torch.equal(got[seq].view(torch.int16), want[seq].view(torch.int16))
    ref64 = oracle_mod.spmm_f64(g["rp"], g["col"], Xf)
    mag = oracle_mod.spmm_f64(g["rp"], g["col"], Xf, absolute=True)
    eps = 2.0 ** -8 if dtype == BF16 else 2.0 ** -10
    assert np.all(np.abs(got.double().numpy() - ref64) <= 1e-5 * mag + eps * np.abs(ref64) + 1e-30)
    return seq.numpy()


@pytest.mark.parametrize("form,dtype,D", TINY_CASES, ids=[_case_id(c) for c in TINY_CASES])
def test_tiny_launch_binary_forward(oracle_mod, dev, form, dtype, D):
    """exact on integer-valued X, the 1e-5 / 16-bit criteria on random X; the second front-end must give the first one's bits"""
    g = _setup(frontends.get("ctypes"), dev, "short_rows", form)
    g2 = _setup(frontends.get("extension"), dev, "short_rows", form)
    assert hcspmm.own_tiny_launch(g["row_nzr"]) and hcspmm.own_tiny_launch(g2["row_nzr"])
    N, rp, col = g["N"], g["rp"], g["col"]
    if dtype == F32:  # (every partial sum is an integer below 2^24: 770 x 4095)
        Xi = (np.arange(N, dtype=np.float32) % 4093)[:, None] + (np.arange(D, dtype=np.float32) % 3)[None, :]
        Xi_d = torch.from_numpy(Xi).to(dev)
    else:  # small enough for the format: exact fp32 sums, one rounding
        Xi_d = ((torch.arange(N, device=dev)[:, None] + torch.arange(D, device=dev)[None, :]) % 4).to(dtype)
        Xi = Xi_d.float().cpu().numpy()
    Zi = g["fe"].forward(Xi_d, *g["args"])[0]
    want = torch.from_numpy(oracle_mod.spmm_f32(rp, col, Xi)).to(dtype)
    assert torch.equal(Zi.cpu().view(_IBITS[dtype]), want.view(_IBITS[dtype]))
    assert torch.equal(g2["fe"].forward(Xi_d, *g2["args"])[0], Zi)
    X = torch.randn((N, D), device=dev, generator=torch.Generator(device=dev).manual_seed(D)).to(dtype)
    Z = g["fe"].forward(X, *g["args"])[0]
    seq = _check_f32(oracle_mod, g, X.cpu().numpy(), Z.cpu().numpy()) if dtype == F32 else _check_h16(oracle_mod, g, X, Z)
    assert int(seq.sum()) >= int((g["deg"] <= 16).sum())  # (wide_threshold is never below 16)
    Z2 = g2["fe"].forward(X, *g2["args"])[0]
    assert torch.equal(Z2.view(_IBITS[dtype]), Z.view(_IBITS[dtype]))
    del X, Z, Z2, Zi, Xi_d
    _free()


@pytest.mark.parametrize("form,dtype,D,off", [("auto", F32, 22, 3), ("auto", F32, 128, 8), ("panel32", F32, 128, 4),
                                              ("auto", BF16, 64, 2), ("auto", F16, 7, 1), ("auto", F16, 520, 8)],
                         ids=lambda v: _NAME.get(v, str(v)))
def test_tiny_launch_writes_every_row_and_nothing_else(fe, dev, form, dtype, D, off):
    """forward_into a NaN-filled wider Z: every row of the slice is written, the 245 000 empty ones included (their zeros
    come from the tiny launch as well), and no element outside it"""
    g = _setup(fe, dev, "short_rows", form)
    assert int((g["deg"] == 0).sum()) > 200000
    X = torch.randn(g["N"], D, device=dev).to(dtype)
    Z = torch.full((g["N"], D + off + 6), float("nan"), device=dev, dtype=dtype)
    fe.forward_into(X, Z[:, off:off + D], *g["args"])
    torch.cuda.synchronize()
    want = fe.forward(X, *g["args"])[0]
    assert torch.equal(Z[:, off:off + D].contiguous().view(_IBITS[dtype]), want.view(_IBITS[dtype]))
    assert not bool(torch.isnan(want).any())
    assert bool(torch.isnan(Z[:, :off]).all()) and bool(torch.isnan(Z[:, off + D:]).all())
    assert bool((want[torch.from_numpy(g["deg"] == 0).to(dev)] == 0).all())
    del X, Z, want
    _free()


# ------------------------------------------------------------------------------------------- weighted: shared references
def _short(gen, shape, bits, dev):
    """test_weighted_gpu._short on the device: at most `bits` significant bits, exponents in a narrow range"""
    m = torch.randint(-(1 << (bits - 1)), 1 << (bits - 1), shape, device=dev, generator=gen)
    e = torch.randint(-bits - 2, -bits + 3, shape, device=dev, generator=gen)
    return torch.ldexp(m.float(), e)


def _csr_order_sum(g, X, V, limit):
    """Sequential fp32 sum, one CSR position at a time, of the rows of at most `limit` entries (other rows stay 0).  V: [E]
    or [heads, E] (head h weights columns [h * Dh, (h + 1) * Dh)).  Products must be exact: one rounding per addition."""
    N, D = X.shape
    deg = g["deg_d"]
    order = torch.argsort(deg, descending=True)
    order = order[deg[order] <= limit]  # longest first: the rows with more than k entries are a prefix
    lens = deg[order]
    rp = g["rp_d"].long()
    want = torch.zeros((N, D), dtype=torch.float32, device=X.device)
    for k in range(int(lens[0]) if order.numel() else 0):
        r = order[:int((lens > k).sum())]
        e = rp[r] + k
        w = V[e][:, None] if V.dim() == 1 else V[:, e].t().repeat_interleave(D // V.size(0), 1)
        want[r] = want[r] + w * X[g["cols"][e]]
    return want, deg <= limit


def _fp64_product(g, X, vals, chunk=16):
    """sum_e v_e x_e and sum_e |v_e x_e| per row in fp64 (index_add over the entries, a column chunk at a time)"""
    N, D = X.shape
    exact = torch.empty((N, D), dtype=torch.float64, device=X.device)
    absum = torch.empty_like(exact)
    v64 = vals.double()[:, None]
    for c0 in range(0, D, chunk):
        prod = v64 * X[:, c0:c0 + chunk].double()[g["cols"]]
        z = torch.zeros((N, prod.size(1)), dtype=torch.float64, device=X.device)
        exact[:, c0:c0 + chunk] = z.clone().index_add_(0, g["rows"], prod)
        absum[:, c0:c0 + chunk] = z.index_add_(0, g["rows"], prod.abs())
    return exact, absum


def _check_fma_bound(g, X, vals, got):
    """check 4 of test_weighted_gpu: |got - exact| <= gamma_n sum |v x|, gamma_n = n u / (1 - n u), u = 2^-24.  16-bit
    features: the fp32 sum s is then rounded once to the format (unit roundoff u16 = 2^-11 for fp16: 11 significant bits,
    round to nearest; half the subnormal spacing 2^-25 below the normal range), so
        |fl16(s) - exact| <= |s - exact| + u16 |s| + 2^-25 <= gamma_n A (1 + u16) + u16 |exact| + 2^-25,  A = sum |v x|."""
    exact, absum = _fp64_product(g, X, vals)
    n = g["deg_d"].double()[:, None]
    gamma = n * U / (1 - n * U)
    bound = gamma * absum
    if X.dtype == F16:
        u16 = 2.0 ** -11
        bound = bound * (1 + u16) + u16 * exact.abs() + 2.0 ** -25
    else:
        assert X.dtype == F32
    err = (got.double() - exact).abs()
    worst = float((err / (bound + TINY)).max())
    print("weighted %s D=%d: worst error / bound = %.3f" % (_NAME[X.dtype], X.shape[1], worst))
    assert bool((err <= bound).all()), worst
    assert not bool((got[g["deg_d"] == 0] != 0).any())


def _power_of_two_inputs(g, dtype, D, seed, dev, heads=1):
    """values[h][e] = 2^(a_h[row] + b_h[col]) and features for which scaling by them commutes with every rounding.  fp32 and
    bf16 (8 exponent bits): normal deviates, exponents -3 ... 3 (test_weighted_gpu's).  fp16: 5 significant bits with
    magnitudes in [1/8, 2) and exponents -2 ... 2, so that every partial sum is a multiple of 2^-11 (nothing falls into
    the subnormal range, where a scaled rounding is no longer the rounding scaled) below 770 * 2 * 16 < 65 504."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    lim = 2 if dtype == F16 else 3
    a = torch.randint(-lim, lim + 1, (heads, g["N"]), device=dev, generator=gen)
    b = torch.randint(-lim, lim + 1, (heads, g["N"]), device=dev, generator=gen)
    V = torch.ldexp(torch.ones((heads, g["E"]), device=dev), a[:, g["rows"]] + b[:, g["cols"]])
    if dtype == F16:
        m = torch.randint(16, 32, (g["N"], D), device=dev, generator=gen).float() / 16
        X = torch.ldexp(m, torch.randint(-3, 1, (g["N"], D), device=dev, generator=gen))
        X = X * (torch.randint(0, 2, (g["N"], D), device=dev, generator=gen).float() * 2 - 1)
    else:
        X = torch.randn((g["N"], D), device=dev, generator=gen)
    one = torch.ones(g["N"], device=dev)
    return X, V, torch.ldexp(one, a)[:, :, None], torch.ldexp(one, b)[:, :, None]


def _check_ones_and_powers_of_two(g, dtype, D, dev):
    """checks 1 and 2 of test_weighted_gpu"""
    fe = g["fe"]
    X, V, sa, sb = _power_of_two_inputs(g, dtype, D, 12 + D, dev)
    Xt = X.to(dtype)
    want = fe.forward(Xt, *g["args"])[0]
    got = fe.forward_weighted(Xt, torch.ones(g["E"], device=dev), *g["args"])[0]
    assert got.dtype == dtype and torch.equal(got.view(_IBITS[dtype]), want.view(_IBITS[dtype])), "ones"
    want = (sa[0] * fe.forward((sb[0] * X).to(dtype), *g["args"])[0].float()).to(dtype)
    got = fe.forward_weighted(Xt, V[0].contiguous(), *g["args"])[0]
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())
    assert bool(torch.isfinite(want).all()) and int((want != 0).sum()) > g["N"] // 4


# ------------------------------------------------------------------------------------------- gate A: weighted, heads
@pytest.mark.parametrize("form,dtype,D", TINY_CASES, ids=[_case_id(c) for c in TINY_CASES])
def test_tiny_launch_weighted_ones_and_entry_mapping(fe, dev, form, dtype, D):
    g = _setup(fe, dev, "short_rows", form)
    assert hcspmm.own_tiny_launch(g["row_nzr"])
    _check_ones_and_powers_of_two(g, dtype, D, dev)
    _free()


@pytest.mark.parametrize("form,D", [("auto", 4), ("auto", 32), ("auto", 128), ("panel32", 128)])
def test_tiny_launch_weighted_csr_order(fe, dev, form, D):
    """check 3 of test_weighted_gpu"""
    g = _setup(fe, dev, "short_rows", form)
    gen = torch.Generator(device=dev).manual_seed(13)
    vals, X = _short(gen, (g["E"],), 8, dev), _short(gen, (g["N"], D), 12, dev)
    got = fe.forward_weighted(X, vals, *g["args"])[0]
    want, ordered = _csr_order_sum(g, X, vals, min(fe.wide_threshold(g["row_nzr"], D), 256))
    assert int(ordered.sum()) > g["N"] - 10000
    assert torch.equal(got[ordered].view(torch.int32), want[ordered].view(torch.int32))
    _free()


@pytest.mark.parametrize("dtype,D", [(F32, 3), (F32, 32), (F32, 64), (F16, 7), (F16, 30), (F16, 64)], ids=lambda v: _NAME.get(v, str(v)))
def test_tiny_launch_weighted_fma_bound(fe, dev, dtype, D):
    g = _setup(fe, dev, "short_rows")
    gen = torch.Generator(device=dev).manual_seed(14)
    vals = torch.randn(g["E"], device=dev, generator=gen)
    X = torch.randn((g["N"], D), device=dev, generator=gen).to(dtype)
    _check_fma_bound(g, X, vals, fe.forward_weighted(X, vals, *g["args"])[0])
    _free()


def _check_heads(g, heads, dh, dev, csr_limit=None):
    """test_heads_gpu: every head's columns are forward_weighted(X, V[h]) at full width, ones give forward, and per-head
    powers of two map every entry and head; csr_limit: the sequential sum of the rows at or below it as well"""
    fe, D = g["fe"], heads * dh
    gen = torch.Generator(device=dev).manual_seed(21 + D)
    X = torch.randn((g["N"], D), device=dev, generator=gen)
    V = torch.randn((heads, g["E"]), device=dev, generator=gen)
    got = fe.forward_weighted_heads(X, V, *g["args"])[0]
    assert got.shape == (g["N"], D)
    for h in range(heads):
        want = fe.forward_weighted(X, V[h].contiguous(), *g["args"])[0]
        assert torch.equal(got[:, h * dh:(h + 1) * dh], want[:, h * dh:(h + 1) * dh]), (heads, dh, h)
    got1 = fe.forward_weighted_heads(X, torch.ones((heads, g["E"]), device=dev), *g["args"])[0]
    assert torch.equal(got1, fe.forward(X, *g["args"])[0])
    X, V, sa, sb = _power_of_two_inputs(g, F32, D, 22 + D, dev, heads)
    got = fe.forward_weighted_heads(X, V, *g["args"])[0]
    for h in range(heads):
        want = sa[h] * fe.forward(sb[h] * X, *g["args"])[0]
        sl = slice(h * dh, (h + 1) * dh)
        assert torch.equal(got[:, sl], want[:, sl]), (heads, dh, h)
    if csr_limit is not None:
        Xs = torch.ldexp(torch.round(torch.ldexp(X, torch.tensor(10, device=dev))), torch.tensor(-10, device=dev))
        got = fe.forward_weighted_heads(Xs, V, *g["args"])[0]
        want, ordered = _csr_order_sum(g, Xs, V, csr_limit)
        assert torch.equal(got[ordered].view(torch.int32), want[ordered].view(torch.int32)), (heads, dh)


@pytest.mark.parametrize("form,heads,dh", HEAD_CASES, ids=["%s-%dx%d" % c for c in HEAD_CASES])
def test_tiny_launch_weighted_heads(fe, dev, form, heads, dh):
    g = _setup(fe, dev, "short_rows", form)
    assert hcspmm.own_tiny_launch(g["row_nzr"])
    _check_heads(g, heads, dh, dev, csr_limit=min(fe.wide_threshold(g["row_nzr"], heads * dh), 256))
    _free()


def test_tiny_launch_weighted_replays_in_a_hip_graph(fe, dev):
    """hybrid launch, tiny launch and fix-up pass inside one capture"""
    g = _setup(fe, dev, "short_rows")
    X = torch.randn(g["N"], 64, device=dev)
    vals = torch.rand(g["E"], device=dev)
    ref = fe.forward_weighted(X, vals, *g["args"])[0]  # warm-up: plan registry and fingerprint checks happen here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fe.forward_weighted(X, vals, *g["args"])[0]
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    vals.copy_(torch.rand(g["E"], device=dev))
    X.copy_(torch.randn(g["N"], 64, device=dev))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fe.forward_weighted(X, vals, *g["args"])[0])
    del graph, out, ref, X, vals
    _free()


# ------------------------------------------------------------------------------------------- gate B (with C and D)
def _csr_limit(g, D):
    """the rows test_weighted_gpu restricts its CSR-order check to -- deg <= min(wide_threshold, 256) -- less, on a sliced
    plan, the rows cut into column slices"""
    h = _header(g)
    lim = min(g["fe"].wide_threshold(g["row_nzr"], D), 256)
    return min(lim, h.slice_threshold) if h.n_slices else lim


@pytest.mark.parametrize("D", WIDE_WIDTHS)
@pytest.mark.parametrize("form", ["no_slices", "auto"])
def test_long_rows_on_one_lane_group_weighted(fe, dev, form, D):
    g = _setup(fe, dev, "power_law", form)
    _check_ones_and_powers_of_two(g, F32, D, dev)
    gen = torch.Generator(device=dev).manual_seed(13 + D)
    vals, X = _short(gen, (g["E"],), 8, dev), _short(gen, (g["N"], D), 12, dev)
    got = fe.forward_weighted(X, vals, *g["args"])[0]
    limit = _csr_limit(g, D)
    want, ordered = _csr_order_sum(g, X, vals, limit)
    if form == "no_slices":
        assert limit == {16: 16, 32: 32, 64: 64, 128: 128, 256: 256}[D]  # (the coverage test's thresholds, one per width)
    assert int(ordered.sum()) >= int((g["deg"] <= 16).sum())
    assert torch.equal(got[ordered].view(torch.int32), want[ordered].view(torch.int32)), (form, D, limit)
    del got, want
    vals = torch.randn(g["E"], device=dev, generator=gen)
    X = torch.randn((g["N"], D), device=dev, generator=gen)
    _check_fma_bound(g, X, vals, fe.forward_weighted(X, vals, *g["args"])[0])
    _free()


@pytest.mark.parametrize("D", WIDE_WIDTHS)
@pytest.mark.parametrize("form", ["no_slices", "auto"])
def test_long_rows_on_one_lane_group_heads(fe, dev, form, D):
    g = _setup(fe, dev, "power_law", form)
    _check_heads(g, 4, D // 4, dev, csr_limit=_csr_limit(g, D))
    _free()


def _tie_features(gen, rows, D, dev):
    """test_extremum_gpu._tie_features: small integers (many ties), half of the zeros negative, 2 % NaN, 2 % +-inf"""
    X = torch.randint(-3, 4, (rows, D), device=dev, generator=gen).float()
    X[(X == 0) & (torch.rand((rows, D), device=dev, generator=gen) < 0.5)] = -0.0
    u = torch.rand((rows, D), device=dev, generator=gen)
    X[u < 0.02] = float("nan")
    X[(u >= 0.02) & (u < 0.03)] = float("inf")
    X[(u >= 0.03) & (u < 0.04)] = float("-inf")
    return X


def _extremum_reference(g, X, reduce, chunk=16):
    """test_extremum_gpu.reference on the device: NaN first, then the largest (smallest) value, ties to the lowest entry"""
    N, E, D = g["N"], g["E"], X.shape[1]
    Z = torch.zeros((N, D), dtype=torch.float32, device=X.device)
    arg = torch.full((N, D), -1, dtype=torch.int32, device=X.device)
    epos = torch.arange(E, device=X.device)[:, None]
    for c0 in range(0, D, chunk):
        V = X[:, c0:c0 + chunk][g["cols"]]
        c = V.size(1)
        idx = g["rows"][:, None].expand(E, c).contiguous()
        key = V if reduce == "max" else -V
        isn = torch.isnan(key)
        anyn = torch.zeros((N, c), dtype=torch.int32, device=X.device).scatter_add_(0, idx, isn.int()) > 0
        kf = torch.where(isn, torch.full_like(key, float("-inf")), key)
        m = torch.full((N, c), float("-inf"), device=X.device).scatter_reduce_(0, idx, kf, "amax")
        cand = torch.where(anyn[g["rows"]], isn, ~isn & (kf == m[g["rows"]]))
        win = torch.full((N, c), E, dtype=torch.int64, device=X.device).scatter_reduce_(0, idx, torch.where(cand, epos, E), "amin")
        ok = win < E
        Z[:, c0:c0 + c] = torch.where(ok, V.gather(0, win.clamp(max=E - 1)), torch.zeros((), device=X.device))
        arg[:, c0:c0 + c] = torch.where(ok, win, -1).int()
    return Z, arg


@pytest.mark.parametrize("D", WIDE_WIDTHS)
@pytest.mark.parametrize("form", ["no_slices", "auto"])
def test_long_rows_on_one_lane_group_extremum(fe, dev, form, D):
    """the bits and tie rules of test_extremum_gpu for EVERY row, forward and backward"""
    g = _setup(fe, dev, "power_law", form)
    perm = fe.transpose_permutation(g["rp_d"], g["col_d"]).to(torch.int32)
    gen = torch.Generator(device=dev).manual_seed(31 + D)
    X = _tie_features(gen, g["N"], D, dev)
    G = torch.randint(-8, 9, (g["N"], D), device=dev, generator=gen).float()
    for reduce in ("max", "min"):
        Z, arg = (fe.forward_max if reduce == "max" else fe.forward_min)(X, *g["args"])
        wz, wa = _extremum_reference(g, X, reduce)
        assert torch.equal(arg, wa), (form, D, reduce)
        assert torch.equal(Z.view(torch.int32), wz.view(torch.int32)), (form, D, reduce)
        Z1 = (fe.forward_max if reduce == "max" else fe.forward_min)(X, *g["args"], return_arg=False)
        assert len(Z1) == 1 and torch.equal(Z1[0].view(torch.int32), wz.view(torch.int32))
        del Z1, wz, Z
        got = fe.forward_extremum_backward(G, arg, perm, *g["args"])
        i, d = torch.nonzero(wa >= 0, as_tuple=True)  # integer-valued G: exact in any order
        want = torch.zeros((g["N"], D), device=dev).index_put_((g["cols"][wa[i, d].long()], d), G[i, d], accumulate=True)
        del i, d
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (form, D, reduce)
        again = fe.forward_extremum_backward(G, arg, perm, *g["args"])
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        del got, want, again, arg, wa
    _free()


# ------------------------------------------------------------------------------------------- gate E
def _gatv2_features(dev, n, D, seed, sign=1.0):
    """test_gatv2_gpu._features"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    mag = 10.0 ** (torch.rand((n, D), device=dev, generator=gen) * (np.log10(30.0) + 3.0) - 3.0)
    x = mag * torch.where(torch.rand((n, D), device=dev, generator=gen) < 0.5, -1.0, 1.0)
    x[:, ::5] = 0.5 * sign
    return x.float()


def _gatv2_graph(dev):
    key = ("gatv2", "short_rows_symmetric")
    if key not in _CACHE:
        rp, col = _graph("short_rows_symmetric")
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        lens = torch.from_numpy(np.diff(rp)).to(dev)
        _CACHE[key] = dict(rp_d=rp_d, col_d=col_d, cols=col_d.long(), lens=lens,
                           rows=torch.repeat_interleave(torch.arange(len(rp) - 1, device=dev), lens.long()),
                           perm=frontends.get("ctypes").transpose_permutation(rp_d, col_d))
    return _CACHE[key]


@pytest.mark.parametrize("heads,dh", GATV2_SHAPES)
def test_gatv2_backward_walks_several_tiles_per_workgroup(dev, heads, dh):
    """the three bounds of test_gatv2_gpu (fp64 reference a column chunk at a time), two calls the same bits, both front-ends
    the same bits"""
    fe = frontends.get("ctypes")
    rp, col = _graph("short_rows_symmetric")
    N, E, D = len(rp) - 1, len(col), heads * dh
    g = _gatv2_graph(dev)
    rows, cols = g["rows"], g["cols"]
    hd, hs = _gatv2_features(dev, N, D, 41 * heads + dh), _gatv2_features(dev, N, D, 43 * heads + dh, sign=-1.0)
    gen = torch.Generator(device=dev).manual_seed(47)
    att = (torch.rand((heads, dh), device=dev, generator=gen) * 2 - 1).float()
    gl = torch.randn((heads, E), device=dev, generator=gen)
    got = fe.gatv2_scores_backward(gl, hd, hs, att, g["rp_d"], g["col_d"], g["perm"], SLOPE)
    gd, gs, ga = got
    assert gd.shape == (N, D) and gs.shape == (N, D) and ga.shape == (heads, dh)
    n = g["lens"].double()[:, None]
    want_att = torch.zeros(D, dtype=torch.float64, device=dev)
    mag_att = torch.zeros(D, dtype=torch.float64, device=dev)
    worst = [0.0, 0.0, 0.0]
    for c0 in range(0, D, 16):
        sl = slice(c0, min(c0 + 16, D))
        a, b = hd[:, sl], hs[:, sl]
        z32 = a[rows] + b[cols]  # one rounded fp32 add, as the kernel's: it decides the branch
        z64 = a.double()[rows] + b.double()[cols]
        pos = z32 > 0
        assert bool((pos == (z64 > 0)).all())
        l64 = torch.where(pos, z64, z64 * SLOPE64)
        term = gl[torch.arange(sl.start, sl.stop, device=dev) // dh].double().t()  # [E, c]: g[h(j)][e]
        gll = term * l64
        want_att[sl], mag_att[sl] = gll.sum(0), gll.abs().sum(0)
        del gll, l64, z32
        term = term * torch.where(pos, torch.ones_like(z64), torch.full_like(z64, SLOPE64))
        del z64, pos
        a64 = att.double().reshape(1, -1)[:, sl]
        for k, (x, idx) in enumerate(((gd, rows), (gs, cols))):
            zero = torch.zeros((N, a64.size(1)), dtype=torch.float64, device=dev)
            want = a64 * zero.clone().index_add_(0, idx, term)
            mag = a64.abs() * zero.index_add_(0, idx, term.abs())
            err, bound = (x[:, sl].double() - want).abs(), (n + 3) * U * mag + TINY
            worst[k] = max(worst[k], float((err / bound).max()))
            assert bool((err <= bound).all()), (heads, dh, c0, worst)
        del term
    err, bound = (ga.double().reshape(-1) - want_att).abs(), (E + 4) * U * mag_att + TINY
    worst[2] = float((err / bound).max())
    print("gatv2 backward at %d rows heads=%d Dh=%d: worst error / bound dst %.3f src %.3f att %.5f" % ((N, heads, dh) + tuple(worst)))
    assert bool((err <= bound).all()), (heads, dh, worst)
    assert bool((gd[g["lens"] == 0] == 0).all()) and bool((gs[g["lens"] == 0] == 0).all())
    again = fe.gatv2_scores_backward(gl, hd, hs, att, g["rp_d"], g["col_d"], g["perm"].int(), SLOPE)
    other = frontends.get("extension").gatv2_scores_backward(gl, hd, hs, att, g["rp_d"], g["col_d"], g["perm"], SLOPE)
    for x, y, z in zip(got, again, other):
        assert torch.equal(x, y) and torch.equal(x, z)
    del got, again, other, gd, gs, hd, hs, gl
    _free()


@pytest.mark.parametrize("heads,dh", GATV2_SHAPES)
def test_gatv2_backward_exact_sums_across_tiles(fe, dev, heads, dh):
    """At E = 3.7 M the (E + 4) u bound of grad_att is 22 % of sum |g l|: a tile left out or an accumulator reset between two
    tiles of a workgroup stays inside it.  So, as with integer-valued X elsewhere: inputs whose every term is a multiple of
    2^-4 -- H in {-1/2, 1/4, 1/2}, slope 1/4, g in {0, 1} -- and whose absolute sum per column stays below 2^24 such units.
    Then every partial sum in every order is exact, and so are the three gradients: grad_att bit for bit the fp64 sum,
    grad_H the one rounding of att times an exact row sum."""
    rp, col = _graph("short_rows_symmetric")
    N, E, D = len(rp) - 1, len(col), heads * dh
    g = _gatv2_graph(dev)
    rows, cols = g["rows"], g["cols"]
    gen = torch.Generator(device=dev).manual_seed(53 + D)
    levels = torch.tensor([-0.5, 0.25, 0.5], device=dev)
    hd = levels[torch.randint(0, 3, (N, D), device=dev, generator=gen)]
    hs = levels[torch.randint(0, 3, (N, D), device=dev, generator=gen)]
    att = torch.randint(-8, 9, (heads, dh), device=dev, generator=gen).float() / 8
    gl = (torch.rand((heads, E), device=dev, generator=gen) < 0.125).float()
    gd, gs, ga = fe.gatv2_scores_backward(gl, hd, hs, att, g["rp_d"], g["col_d"], g["perm"], 0.25)
    want_att = torch.empty(D, dtype=torch.float64, device=dev)
    for c0 in range(0, D, 16):
        sl = slice(c0, min(c0 + 16, D))
        z = hd[:, sl].double()[rows] + hs[:, sl].double()[cols]
        ge = gl[torch.arange(sl.start, sl.stop, device=dev) // dh].double().t()
        gll = ge * torch.where(z > 0, z, z * 0.25)
        assert float(gll.abs().sum(0).max()) * 16 < 2 ** 24  # every partial sum is a multiple of 2^-4 below 2^20: exact
        want_att[sl] = gll.sum(0)
        term = ge * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.25))
        del z, gll, ge
        a64 = att.double().reshape(1, -1)[:, sl]
        for x, idx in ((gd, rows), (gs, cols)):
            acc = torch.zeros((N, a64.size(1)), dtype=torch.float64, device=dev).index_add_(0, idx, term)
            assert torch.equal(x[:, sl], (a64 * acc).float()), (heads, dh, c0)
        del term
    assert float(want_att.abs().min()) > 1.0 and torch.equal(ga.double().reshape(-1), want_att), (heads, dh)
    del gd, gs, hd, hs, gl
    _free()


# ------------------------------------------------------------------------------------------- gate F
def test_edge_norm_beyond_one_round_of_its_grid(fe, dev):
    """17 M entries: the grid-stride loop's second round.  Compared exactly as test_edge_norm_on_the_device_matches_numpy does
    (numpy's correctly rounded fp32 sqrt and division on the host)."""
    N = 1000000
    deg_d = 15 + torch.arange(N, device=dev) % 5
    rp_d = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(deg_d, 0)]).int()
    E = int(rp_d[-1])
    assert E > 65536 * 256
    col_d = torch.randint(0, N, (E,), device=dev, generator=torch.Generator(device=dev).manual_seed(8)).int()
    sym = fe.edge_norm(rp_d, col_d, "sym").cpu().numpy()
    mean = fe.edge_norm(rp_d, col_d, "mean").cpu().numpy()
    deg = deg_d.cpu().numpy().astype(np.float64)
    rows = np.repeat(np.arange(N), deg_d.cpu().numpy())
    col = col_d.cpu().numpy()
    assert np.array_equal(sym, (np.float32(1) / np.sqrt((deg[rows] * deg[col]).astype(np.float32))).astype(np.float32))
    assert np.array_equal(mean, (np.float32(1) / deg[rows].astype(np.float32)))
    del rp_d, col_d, deg_d
    _free()
