"""8-bit (e4m3fn) feature storage on an MI355X, through both Python front-ends: the quantiser (hcspmm_quantize_fp8), the
products that read its codes (hcspmm_forward_fp8: binary, with values, with per-row scales) and the layers built on them.

The contract (include/hcspmm.h): codes are OCP e4m3fn, widened exactly; entry e of column c weighs w = values[e] * scale[c],
one fp32 multiplication; every step is acc = fmaf(w, x, acc) in fp32, in the order hcspmm_forward_weighted adds that row on
that sub-path.  The launch layout depends on the element size, so what is compared bit for bit are sums that are exact in
fp32 whatever the order:
  1. the quantiser's codes and scales against torch on the CPU, byte for byte;
  2. binary A and codes on a 2^-6 grid below 16: any sum of up to 2^14 of them is exact -> the fp64 product's bits;
  3. the same with values in {1, 2} keyed by row and scales in {0.5, 1} keyed by column (12-bit products on a 2^-7 grid);
  4. general data within gamma_n * sum |w x| of the fp64 product of the dequantised codes (the fp32 accumulation bound);
  5. strides, taller operands, empty and one-row graphs, NaN-filled outputs;  6. the size-gated launch paths;  7. the layers.
"""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

import frontends
import hcspmm
from hcspmm import capi, graphs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hc-spmm_amd")
F8 = torch.float8_e4m3fn
U = 2.0 ** -24


@pytest.fixture(scope="module", params=["ctypes", "extension"])
def fe(request):
    return frontends.get(request.param)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------- graphs and plans
def _graph(kind):  # the graph kinds of test_weighted_gpu.py
    if kind == "powerlaw":  # hubs: wide tasks, split rows
        return graphs.powerlaw_graph(3000, 60000, seed=3, max_degree_frac=0.3)
    if kind == "planted":  # dense-tile windows of every record kind
        return graphs.planted_dense_graph(2400, seed=4)
    if kind == "community":
        return graphs.community_graph(2500, 20000, seed=5)[:2]
    if kind == "molecule":  # short rows: tiny tasks
        return graphs.molecule_graph(3000, seed=6)
    if kind == "uniform":
        return graphs.uniform_graph(2000, 16000, seed=7)
    if kind == "short_rows_hubs":  # test 6: >= 524 288 rows of at most two entries, and hubs that hold 5 % of the entries
        N = 640000
        rng = np.random.default_rng(9)
        deg = rng.choice([0, 1, 2, 3, 7], size=N, p=[0.35, 0.3, 0.2, 0.1, 0.05])
        hubs = rng.choice(N, 150, replace=False)
        deg[hubs] = rng.integers(300, 700, hubs.size)
        rows = np.repeat(np.arange(N, dtype=np.int64), deg)
        return graphs._to_csr(rows, rng.integers(0, N, rows.shape[0]), N)
    raise KeyError(kind)


PLANS = {  # the nine plan forms of test_weighted_gpu.py, set by explicit plan parameters (never the environment)
    "default": {},
    "no_slices": dict(slice_threshold=-1),
    "slices": dict(slice_threshold=16, n_slices=8),
    "sparse": dict(force=0),
    "dense": dict(force=1),
    "tiny_segments": dict(split_threshold=9, segment_len=7),
    "panel32": dict(panel_cols=32),
    "panel64": dict(panel_cols=64),
    "plan_free": dict(plan=False),
}
KINDS = ["powerlaw", "planted", "community", "molecule", "uniform"]
WIDTHS = [4, 8, 12, 16, 20, 36, 64, 128, 132, 256, 520]
_CACHE, _REF = {}, {}


def _setup(fe, dev, kind, form):
    key = (fe.name, kind, form)
    if key in _CACHE:
        return _CACHE[key]
    rp, col = _graph(kind)
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    bp, e2c, e2r, ht, row_nzr, col_nzr = fe.preprocess(col_d, rp_d, N, E, (N + 15) // 16, rule=3)
    p = dict(PLANS[form])
    force = p.pop("force", None)
    plan = p.pop("plan", True)
    if force is not None:
        ht = torch.full_like(ht, force)
    if not plan:
        row_nzr = torch.zeros(1, dtype=torch.int32, device=dev)
    elif force is not None or p:
        row_nzr = fe.build_plan(rp_d, col_d, bp, e2c, ht, **p)
    deg = np.diff(rp)
    g = dict(kind=kind, rp=rp, col=col, N=N, E=E, deg=deg, args=(rp_d, col_d, bp, e2c, e2r, ht, row_nzr, col_nzr), plan=plan,
             row_nzr=row_nzr, cols=col_d.long(),
             rows=torch.repeat_interleave(torch.arange(N, device=dev), torch.from_numpy(deg).to(dev).long()))
    _CACHE[key] = g
    return g


def _fp64_product(g, X, w=None, absolute=False):
    """sum over a row's entries of w_e * X[col_e] in fp64 (index_add over the entries, 64 columns at a time)"""
    N, D = g["N"], X.shape[1]
    out = torch.zeros((N, D), dtype=torch.float64, device=X.device)
    for c0 in range(0, D, 64):
        t = X[:, c0:c0 + 64].double()[g["cols"]]
        if w is not None:
            t = t * w.double()[:, None]
        out[:, c0:c0 + 64].index_add_(0, g["rows"], t.abs() if absolute else t)
    return out


# ------------------------------------------------------------------------------------------- exact data (tests 2, 3, 6)
def _grid_codes(dev):
    """the 114 e4m3fn codes with |x| < 16 that are zero or at least 0.125: all of them multiples of 2^-6"""
    v = torch.arange(256, dtype=torch.uint8).view(F8).float()
    ok = torch.isfinite(v) & (v.abs() < 16) & ((v == 0) | (v.abs() >= 0.125))
    codes = torch.arange(256, dtype=torch.uint8)[ok]
    assert codes.numel() == 114 and bool((v[ok] * 64 == (v[ok] * 64).round()).all())
    return codes.to(dev)


def _exact_case(dev, kind, N, D):
    """codes [N, D] drawn uniformly from the grid codes, their fp32 values; one draw per (graph kind, width), shared"""
    key = ("codes", kind, D)
    if key not in _REF:
        gen = torch.Generator(device=dev).manual_seed(1000 + D)
        grid = _grid_codes(dev)
        Xq = grid[torch.randint(0, grid.numel(), (N, D), device=dev, generator=gen)].contiguous()
        _REF[key] = (Xq, Xq.view(F8).float())
    return _REF[key]


def _row_values(N, dev):  # {1, 2}, keyed by the row
    return 1.0 + ((torch.arange(N, device=dev) * 2654435761 >> 7) & 1).float()


def _col_scales(N, dev):  # {0.5, 1}, keyed by the column
    return 0.5 + 0.5 * ((torch.arange(N, device=dev) * 40503 >> 5) & 1).float()


def _exact_reference(dev, g, D, mode):
    """fp64 product converted to fp32 for the exact data: mode in binary / values / scale / both; shared by plan forms and
    front-ends"""
    key = ("ref", g["kind"], D, mode)
    if key not in _REF:
        _, Xv = _exact_case(dev, g["kind"], g["N"], D)
        w = None
        if mode != "binary":
            w = torch.ones(g["E"], device=dev)
            if mode in ("values", "both"):
                w = w * _row_values(g["N"], dev)[g["rows"]]
            if mode in ("scale", "both"):
                w = w * _col_scales(g["N"], dev)[g["cols"]]
        Z64 = _fp64_product(g, Xv, w)
        Z = Z64.float()
        assert torch.equal(Z.double(), Z64)  # exact in fp32: what makes the order irrelevant
        _REF[key] = Z
    return _REF[key]


# ------------------------------------------------------------------------------------------- 1. the quantiser
def _quantiser_input(D, seed):
    rng = np.random.default_rng(seed)
    rows = 1000
    X = rng.standard_normal((rows, D)).astype(np.float32) * np.ldexp(np.float32(1), rng.integers(-20, 21, rows))[:, None].astype(np.float32)
    special = rng.random((rows, D)) < 0.02
    X[special] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(special.sum()))
    X[5] = 0.0
    X[6] = -0.0
    X[7] = 0.0
    X[7, D // 2] = 3.0  # rows with one entry
    X[8] = 0.0
    X[8, 0] = -1e-37  # amax / 448 is not a normal number
    X[9] = np.nan   # no finite entry
    X[10] = np.inf
    X[11, 1:] = np.nan  # one finite entry
    return X


def _reference_scales(X):
    a = np.abs(X)
    a[~np.isfinite(X)] = 0.0
    amax = a.max(axis=1).astype(np.float32)
    s = (amax / np.float32(448.0)).astype(np.float32)
    s[amax == 0] = np.float32(1.0)
    s[(amax > 0) & (s < np.float32(2.0 ** -126))] = np.float32(2.0 ** -126)
    return s


def _reference_codes(X, s):
    Xt, st = torch.from_numpy(X), torch.from_numpy(s)
    return torch.clamp(Xt / st[:, None], -448, 448).to(F8).view(torch.uint8)


@pytest.mark.parametrize("D", WIDTHS + [1028, 1100])
def test_quantiser_matches_torch_byte_for_byte(fe, dev, D):
    X = _quantiser_input(D, 100 + D)
    s = _reference_scales(X)
    assert s[9] == 1 and s[10] == 1 and s[5] == 1 and s[8] == np.float32(2.0 ** -126)
    Xq, scale = fe.quantize_fp8(torch.from_numpy(X).to(dev))
    assert Xq.dtype == F8 and Xq.shape == (1000, D) and scale.dtype == torch.float32 and scale.shape == (1000,)
    assert np.array_equal(scale.cpu().numpy().view(np.int32), s.view(np.int32))
    want = _reference_codes(X, s)
    got = Xq.view(torch.uint8).cpu()
    assert torch.equal(got, want), (D, int((got != want).sum()))
    nan = torch.from_numpy(np.isnan(X))
    assert bool(((got[nan] & 0x7f) == 0x7f).all()) and bool(((got[~nan] & 0x7f) != 0x7f).all())
    # a supplied scale half the row's own: the clamp does real work
    half = (s * np.float32(0.5)).astype(np.float32)
    half[s <= np.float32(2.0 ** -125)] = s[s <= np.float32(2.0 ** -125)]
    Xq2, scale2 = fe.quantize_fp8(torch.from_numpy(X).to(dev), torch.from_numpy(half).to(dev))
    assert np.array_equal(scale2.cpu().numpy().view(np.int32), half.view(np.int32))
    got2 = Xq2.view(torch.uint8).cpu()
    assert torch.equal(got2, _reference_codes(X, half))
    sat = got2.view(F8).float().abs() == 448
    finite = torch.from_numpy(np.isfinite(X) & (np.abs(X) > 0.6 * (448 * s)[:, None]))
    assert int(sat.sum()) > 500 and bool(sat[finite & torch.from_numpy(half < s)[:, None]].all())


def test_quantiser_refuses_bad_operands(fe, dev):
    with pytest.raises(RuntimeError, match="multiples of 4"):
        fe.quantize_fp8(torch.zeros(8, 6, device=dev))
    with pytest.raises(RuntimeError, match="input must be a CUDA tensor"):
        fe.quantize_fp8(torch.zeros(8, 8))
    with pytest.raises(RuntimeError, match="float32"):
        fe.quantize_fp8(torch.zeros(8, 8, device=dev, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="scale must hold one float32 per row"):
        fe.quantize_fp8(torch.zeros(8, 8, device=dev), torch.ones(7, device=dev))


# ------------------------------------------------------------------------------------------- 2, 3. exact sums
@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_exact_sums_any_order(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    assert int(g["deg"].max()) <= 2 ** 14  # |x| < 16 on a 2^-6 grid: 2^14 terms stay within 24 bits
    for D in WIDTHS:
        Xq, _ = _exact_case(dev, kind, g["N"], D)
        want = _exact_reference(dev, g, D, "binary")
        got = fe.forward_fp8(Xq.view(F8), None, *g["args"])[0]
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32)), (kind, form, D)
    got = fe.forward_fp8(_exact_case(dev, kind, g["N"], 36)[0], None, *g["args"])[0]  # uint8 codes are taken as they are
    assert torch.equal(got, _exact_reference(dev, g, 36, "binary"))


@pytest.mark.parametrize("mode", ["values", "scale", "both"])
@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_exact_sums_with_weights_and_scales(fe, dev, kind, form, mode):
    g = _setup(fe, dev, kind, form)
    # products below 2^5 on a 2^-7 grid: 12 bits; a row of n of them needs 12 + ceil(log2 n) bits
    assert 12 + math.ceil(math.log2(max(int(g["deg"].max()), 1))) <= 24
    values = _row_values(g["N"], dev)[g["rows"]].contiguous()
    scale = _col_scales(g["N"], dev)
    assert set(values.unique().tolist()) <= {1.0, 2.0} and set(scale.unique().tolist()) == {0.5, 1.0}
    for D in WIDTHS:
        Xq = _exact_case(dev, kind, g["N"], D)[0].view(F8)
        want = _exact_reference(dev, g, D, mode)
        if mode == "values":
            got = fe.forward_weighted_fp8(Xq, None, values, *g["args"])[0]
        elif mode == "scale":
            got = fe.forward_fp8(Xq, scale, *g["args"])[0]
        else:
            got = fe.forward_weighted_fp8(Xq, scale, values, *g["args"])[0]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (kind, form, mode, D)


# ------------------------------------------------------------------------------------------- 4. general data
@pytest.mark.parametrize("form", list(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_general_data_within_the_fma_bound(fe, dev, kind, form):
    g = _setup(fe, dev, kind, form)
    values = fe.edge_norm(g["args"][0], g["args"][1], "sym")
    deg = torch.from_numpy(g["deg"]).to(dev).double()
    gamma = (deg * U / (1 - deg * U))[:, None]
    for D in (4, 20, 64, 132, 256):
        X = torch.randn((g["N"], D), device=dev, generator=torch.Generator(device=dev).manual_seed(D))
        Xq, scale = fe.quantize_fp8(X)
        got = fe.forward_weighted_fp8(Xq, scale, values, *g["args"])[0]
        w = values * scale[g["cols"]]  # ONE fp32 multiplication per entry: the contract's w_e
        Xv = Xq.float()
        exact = _fp64_product(g, Xv, w)
        absum = _fp64_product(g, Xv, w, absolute=True)
        # "sym" values are 1 / sqrt(deg(row) * deg(col)): an entry whose column is a node without entries of its own (the planted
        # graph has three) weighs inf, and its row's sums are inf or NaN in fp64 and fp32 alike -- the bound speaks about the rest
        ok = torch.isfinite(absum)
        assert bool((torch.isfinite(got) == ok).all()) and bool((torch.isfinite(exact) == ok).all()), (kind, form, D)
        assert int((~ok).any(1).sum()) <= int((~torch.isfinite(values)).sum()) and bool(ok.any(1).sum() >= g["N"] - 8)
        err = torch.where(ok, (got.double() - exact).abs(), torch.zeros_like(exact))
        bound = torch.where(ok, gamma * absum, torch.zeros_like(exact))
        assert bool((err <= bound).all()), (kind, form, D, float((err / (bound + 1e-300)).max()))


# ------------------------------------------------------------------------------------------- 5. strides and buffers
def _dptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _forward_fp8_capi(g, Xq, ldx, scale, values, Z, ldz, D):
    h = hcspmm.plan_header(g["row_nzr"]) if g["plan"] else None
    ws_bytes = capi.lib().hcspmm_workspace_bytes(ctypes.byref(h), D) if h is not None else 0
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=Z.device)
    rp_d, col_d, bp, e2c, e2r, ht, row_nzr, _ = g["args"]
    rc = capi.lib().hcspmm_forward_fp8(_dptr(Xq), Xq.size(0), ldx, 0, _dptr(scale), _dptr(values), _dptr(Z), ldz, _dptr(rp_d),
                                       _dptr(col_d), _dptr(bp), _dptr(e2c), _dptr(e2r), _dptr(ht),
                                       _dptr(row_nzr) if h is not None else ctypes.c_void_p(0),
                                       ctypes.byref(h) if h is not None else None, g["N"], g["E"], D, _dptr(ws), ws_bytes,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, ws


@pytest.mark.parametrize("form", ["default", "dense", "tiny_segments", "panel32", "plan_free"])
@pytest.mark.parametrize("kind", ["powerlaw", "planted", "molecule"])
def test_strided_operands_and_taller_x(dev, kind, form):
    g = _setup(frontends.get("ctypes"), dev, kind, form)
    N = g["N"]
    values = _row_values(N, dev)[g["rows"]].contiguous()
    for D, ldx, ldz, off in ((4, 8, 12, 4), (36, 64, 40, 1), (128, 256, 132, 3), (132, 136, 140, 5)):
        codes = _exact_case(dev, kind, N, D)[0]
        Xbig = torch.full((N + 7, ldx), 0x7f, dtype=torch.uint8, device=dev)  # NaN codes around the operand: nothing else is read
        Xbig[:N, :D] = codes
        scale = torch.full((N + 7,), float("nan"), device=dev)
        scale[:N] = _col_scales(N, dev)
        Zbig = torch.full((N, ldz + off), float("nan"), device=dev)
        Zv = Zbig[:, off:]  # element-aligned fp32 rows ldz + off apart
        rc, _ = _forward_fp8_capi(g, Xbig, ldx, scale, values, Zv, ldz + off, D)
        assert rc == 0
        assert torch.equal(Zv[:, :D].contiguous().view(torch.int32), _exact_reference(dev, g, D, "both").view(torch.int32)), (D,)
        assert bool(torch.isnan(Zbig[:, :off]).all()) and bool(torch.isnan(Zv[:, D:]).all())  # and nothing else written
        rc, _ = _forward_fp8_capi(g, Xbig, ldx, None, None, Zv, ldz + off, D)  # the binary launch, same views
        assert rc == 0
        assert torch.equal(Zv[:, :D].contiguous().view(torch.int32), _exact_reference(dev, g, D, "binary").view(torch.int32)), (D,)
        assert bool(torch.isnan(Zbig[:, :off]).all()) and bool(torch.isnan(Zv[:, D:]).all())


def test_device_side_argument_errors(dev):
    g = _setup(frontends.get("ctypes"), dev, "powerlaw", "default")
    N, D = g["N"], 64
    Xq = torch.zeros((N, D), dtype=torch.uint8, device=dev)
    Z = torch.zeros((N, D), device=dev)
    h = hcspmm.plan_header(g["row_nzr"])
    need = capi.lib().hcspmm_workspace_bytes(ctypes.byref(h), D)
    assert need > 0
    rp_d, col_d, bp, e2c, e2r, ht, row_nzr, _ = g["args"]

    def call(x_rows=N, ws_bytes=need, n=N, xq=Xq):
        ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
        return capi.lib().hcspmm_forward_fp8(_dptr(xq), x_rows, D, 0, None, None, _dptr(Z), D, _dptr(rp_d), _dptr(col_d), _dptr(bp),
                                             _dptr(e2c), _dptr(e2r), _dptr(ht), _dptr(row_nzr), ctypes.byref(h), n, g["E"], D,
                                             _dptr(ws), ws_bytes, None)
    assert call() == 0
    assert call(ws_bytes=need - 4) == capi.EWORKSPACE
    assert call(n=N - 1) == capi.EPLAN
    assert call(x_rows=h.num_columns - 1) == capi.EINVAL
    assert call(xq=Xq.view(-1)[2:]) == capi.EINVAL  # a code base off the dword grid
    torch.cuda.synchronize()


def test_empty_and_one_row_graphs(fe, dev):
    for rp, col in ((np.array([0, 0], np.int32), np.zeros(0, np.int32)),          # one row, E = 0
                    (np.array([0, 1], np.int32), np.array([0], np.int32)),        # one row, a self loop
                    (np.zeros(41, np.int32), np.zeros(0, np.int32)),              # 40 rows, E = 0
                    (np.arange(34, dtype=np.int32), ((np.arange(33) + 1) % 33).astype(np.int32))):  # a ring: one entry per row
        N, E = len(rp) - 1, len(col)
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        graph = fe.preprocess(col_d, rp_d, N, E, (N + 15) // 16, rule=3)
        for plan in (True, False):
            args = (rp_d, col_d) + tuple(graph[:4]) + ((graph[4] if plan else torch.zeros(1, dtype=torch.int32, device=dev)), graph[5])
            for D in (4, 36, 128):
                Xq, Xv = _exact_case(dev, "tiny%d" % N, N, D)
                values = torch.full((E,), 2.0, device=dev)
                scale = torch.full((N,), 0.5, device=dev)
                want = torch.zeros((N, D), device=dev)
                if E:
                    want[torch.repeat_interleave(torch.arange(N, device=dev), torch.from_numpy(np.diff(rp)).to(dev).long())] = Xv[col_d.long()]
                assert torch.equal(fe.forward_fp8(Xq.view(F8), None, *args)[0], want), (N, E, plan, D)
                assert torch.equal(fe.forward_weighted_fp8(Xq.view(F8), scale, values, *args)[0], want), (N, E, plan, D)


def test_bad_operands_are_refused(fe, dev):
    g = _setup(fe, dev, "uniform", "default")
    N, E = g["N"], g["E"]
    Xq = torch.zeros((N, 16), dtype=torch.uint8, device=dev).view(F8)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        fe.forward_fp8(torch.zeros((N, 16), device=dev), None, *g["args"])
    with pytest.raises(RuntimeError, match="multiples of 4"):
        fe.forward_fp8(torch.zeros((N, 6), dtype=torch.uint8, device=dev), None, *g["args"])
    with pytest.raises(RuntimeError, match="scale must hold one float32 per row"):
        fe.forward_fp8(Xq, torch.ones(N - 1, device=dev), *g["args"])
    with pytest.raises(RuntimeError, match="values must hold one float32 per stored entry"):
        fe.forward_weighted_fp8(Xq, None, torch.ones(E - 1, device=dev), *g["args"])
    with pytest.raises(RuntimeError, match="values must be a float32 tensor"):
        fe.forward_weighted_fp8(Xq, None, torch.ones(E, dtype=torch.float64, device=dev), *g["args"])
    with pytest.raises(RuntimeError, match="rows but the graph has"):
        fe.forward_fp8(Xq[:-1], None, *g["args"])


# ------------------------------------------------------------------------------------------- 6. size-gated paths
OVERRIDES = ("HCSPMM_TINY_KERNEL_MIN_TASKS", "HCSPMM_PANEL_COLS", "HCSPMM_SLICE_THRESHOLD", "HCSPMM_SLICES")


def _assert_defaults():
    found = [k for k in OVERRIDES if k in os.environ]
    assert not found, "unset %s: these tests pin the launch decisions the library takes by default" % ", ".join(found)


@pytest.mark.parametrize("D", [4, 36, 128, 264])  # L = 4 (4 codes per lane), 8, 16 and 64 (8 codes per lane)
def test_gates_own_tiny_launch_and_automatic_slices(fe, dev, D):
    """the smallest graph that opens both gates: 640 000 rows (544 000 of at most two entries -> n_tiny >= 524 288: the tiny
    tasks' own launch, tiny_kernel / tiny_w_kernel<F8>) whose 150 hubs of 300 ... 700 entries hold 5 % of the entries of an X
    of more than 250 000 rows (-> XCD-affine column slices without being asked)"""
    _assert_defaults()
    g = _setup(fe, dev, "short_rows_hubs", "default")
    h = fe.header(g["row_nzr"])
    assert h.n_tiny >= 524288 and capi.lib().hcspmm_own_tiny_launch(ctypes.byref(hcspmm.plan_header(g["row_nzr"])), 0) == 1
    assert h.n_slices > 0 and h.n_slice_tasks > 0 and h.slice_threshold == 256
    assert fe.wide_threshold_fp8(g["row_nzr"], D) in (16, 32, 64, 128, 256, 2 ** 31 - 1)
    assert int(g["deg"].max()) <= 2 ** 12
    Xq = _exact_case(dev, "short_rows_hubs", g["N"], D)[0].view(F8)
    got = fe.forward_fp8(Xq, None, *g["args"])[0]
    assert torch.equal(got.view(torch.int32), _exact_reference(dev, g, D, "binary").view(torch.int32))
    values = _row_values(g["N"], dev)[g["rows"]].contiguous()
    got = fe.forward_weighted_fp8(Xq, _col_scales(g["N"], dev), values, *g["args"])[0]
    assert torch.equal(got.view(torch.int32), _exact_reference(dev, g, D, "both").view(torch.int32))
    del got
    for k in [k for k in _REF if k[1] == "short_rows_hubs" and k[2] == D]:
        del _REF[k]
    torch.cuda.empty_cache()


def test_gate_automatic_panels(fe, dev):
    """capi.hip panel_choice, one-byte elements: a cache line is 128 columns, so from 256 columns up a graph whose tasks hold
    eight entries or more on average is walked panel-major -- the 3000-row power-law graph already is (tests 2 and 3 at
    D = 256 and 520 ran through it); below 256 columns, or with short rows, one pass"""
    _assert_defaults()
    g = _setup(fe, dev, "powerlaw", "default")
    h = fe.header(g["row_nzr"])
    assert h.panel_cols == 0 and h.nnz_sparse / (h.n_tasks + h.n_slice_tasks) >= 8.0
    # the wide threshold is taken for the lane-group count of ONE panel (128 columns: L = 16) from 256 columns up ...
    t128, t256, t520 = (fe.wide_threshold_fp8(g["row_nzr"], D) for D in (128, 256, 520))
    assert t256 != 2 ** 31 - 1 and t520 != 2 ** 31 - 1
    # ... where a single pass over 520 columns would leave one lane group per wave and no wide task at all
    gm = _setup(fe, dev, "molecule", "default")
    hm = fe.header(gm["row_nzr"])
    assert hm.nnz_sparse / max(hm.n_tasks + hm.n_slice_tasks, 1) < 8.0 and fe.wide_threshold_fp8(gm["row_nzr"], 520) == 2 ** 31 - 1
    assert t128 in (16, 32, 64, 128, 256)


# ------------------------------------------------------------------------------------------- 7. layers and driver
def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


@pytest.mark.parametrize("norm", ["sym", "mean"])
@pytest.mark.parametrize("model", ["gcn", "gin"])
def test_layers_quantised_forward_exact_backward(dev, model, norm):
    _pkg_imports()
    import GNN_model
    import HCSPMM
    rp, col = graphs.powerlaw_graph(1500, 20000, seed=21, max_degree_frac=0.2)
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    args = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16, -1))
    ew = HCSPMM.edge_norm(rp_d, col_d, norm)
    conv = (GNN_model.GCNConv if model == "gcn" else GNN_model.GINConv)(24, 16, 0).to(dev)
    assert conv.feature_storage == "fp32"
    X0 = torch.randn(N, 24, device=dev)
    G = torch.randn(N, 16, device=dev)
    out = {}
    for storage in ("fp32", "fp8"):
        conv.feature_storage = storage
        conv.weights.grad = None
        X = X0.clone().requires_grad_(True)
        Y = conv(X, *args, None, edge_weight=ew)
        (Y * G).sum().backward()
        out[storage] = (Y.detach(), X.grad.clone(), conv.weights.grad.clone())
    W = conv.weights.detach()
    with torch.no_grad():
        if model == "gin":  # aggregate, then update
            Xq, s = HCSPMM.quantize_fp8(X0)
            want = GNN_model._mm(HCSPMM.forward_weighted_fp8(Xq, s, ew, *args)[0], W)  # the layers' update
        else:
            Xq, s = HCSPMM.quantize_fp8(GNN_model._mm(X0, W))
            want = HCSPMM.forward_weighted_fp8(Xq, s, ew, *args)[0]
    assert torch.equal(out["fp8"][0], want)
    assert not torch.equal(out["fp8"][0], out["fp32"][0])  # (the forward really is quantised)
    assert torch.equal(out["fp8"][1], out["fp32"][1]), "dX differs from the fp32 layer's"
    assert torch.equal(out["fp8"][2], out["fp32"][2]), "dW differs from the fp32 layer's"
    conv.feature_storage = "fp8"
    with pytest.raises(ValueError, match="edge_weight"):
        conv(X0, *args, None)
    conv.feature_storage = "bf16"
    with pytest.raises(ValueError, match="feature_storage"):
        conv(X0, *args, None, edge_weight=ew)


def test_aggregate_fp8_directed_and_refusals(dev):
    _pkg_imports()
    import GNN_model
    import HCSPMM
    rp, col = graphs.uniform_graph(600, 5000, seed=3)  # not pattern-symmetric
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    args = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16, -1))
    ew = torch.rand(E, device=dev)
    G = torch.randn(N, 12, device=dev)
    grads = []
    for fn in (GNN_model.weighted_aggregate, GNN_model.aggregate_fp8):
        X = torch.randn(N, 12, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).requires_grad_(True)
        (fn(X, ew, args, directed=True) * G).sum().backward()
        grads.append(X.grad)
    assert torch.equal(grads[0], grads[1])
    with pytest.raises(ValueError, match="multiples of 4"):
        GNN_model.aggregate_fp8(torch.randn(N, 6, device=dev), ew, args, directed=True)
    with pytest.raises(NotImplementedError, match="SDDMM"):
        GNN_model.aggregate_fp8(torch.randn(N, 8, device=dev), ew.clone().requires_grad_(True), args, directed=True)


@pytest.mark.parametrize("model", ["gcn", "gin"])
def test_driver_trains_and_evaluates_with_fp8(model, capsys, monkeypatch):
    _pkg_imports()
    monkeypatch.chdir(PKG)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_fp8", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    net = mod.main(["--dataset", "example", "--dim", "16", "--num_layers", "3", "--hidden", "32", "--classes", "20",
                    "--epochs", "20", "--model", model, "--norm", "sym", "--fp8"])
    out = capsys.readouterr().out
    assert "Train (ms/epoch):" in out
    line = [l for l in out.splitlines() if l.startswith("FP8 eval:")]
    assert len(line) == 1
    agree = float(line[0].split("argmax agreement")[1].split()[0])
    diff = float(line[0].split("max |log-prob diff|")[1].split()[0])
    assert 0.0 <= agree <= 1.0 and math.isfinite(diff) and diff > 0.0
    for name, prm in net.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    for argv in (["--model", "gcn", "--fp8"], ["--model", "gat", "--norm", "none", "--fp8"],
                 ["--model", "gcn", "--norm", "sym", "--classes", "22", "--fp8"]):
        with pytest.raises(SystemExit):
            mod.parse_args(argv)
