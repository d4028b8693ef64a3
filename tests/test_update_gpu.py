"""The update GEMM (hcspmm_dense_update: out = X W) and the weight gradient (hcspmm_weight_grad: dW = A^T B) against
the fp64 product, across the whole dispatch of hc-spmm_amd/csrc/update_kernels.hip.

launch_dense_update picks one of four kernels by the alignment of `in` (and `out`), D, H and the LDS the staged weights
need; each streaming kernel is instantiated for T = ceil(H/16) output tiles.  _route() below mirrors those predicates, and
test_update_table_reaches_every_route_and_tile asserts that the case table reaches every (route, T) cell, so that a
change to the dispatch cannot silently leave the table behind.  launch_weight_grad has one instantiation per
(ceil(D/16), ceil(H/16)) in its supported range; the weight-gradient table reaches all 25.

Checks of every case:
  * random-normal operands: |got - fp64 product| <= 1e-5 * (|X| |W|) componentwise (the suite's bar for A*X);
  * integer operands in [-2, 2]: EXACTLY the fp64 product (every partial sum is an integer below 2^24), which catches
    a dropped, duplicated or misplaced k-term or column whatever its magnitude;
  * a second call gives the same bits, and the two front-ends (ctypes `hcspmm`, extension `HCSPMM`) agree bit for bit;
  * through the C ABI: nothing outside the output is written (dense update into a sentinel-filled buffer at an offset of
    one float), and the weight gradient is right with a workspace full of NaN (trailing groups with no rows must write
    zero partials).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import hcspmm
from hcspmm import capi

pytestmark = pytest.mark.gpu

EXT_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hc-spmm_amd", "hybrid_kernel")

LDS_BYTES = 64 * 1024  # the streaming kernels' staged weights
WG_CAP = 512           # weight_grad_groups: at most 512 groups of at least 64 rows


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: no HIP device visible")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    if EXT_DIR not in sys.path:
        sys.path.insert(0, EXT_DIR)
    import HCSPMM
    return HCSPMM


def _cdiv(a, b):
    return (a + b - 1) // b


def _route(in_addr, out_addr, D, H):
    """(route, T) launch_dense_update takes; for the any-shape kernel T is the number of passes of its h0 loop (128 columns
    each)."""
    Tp = _cdiv(H, 16)
    if (in_addr | out_addr) % 16 == 0 and D % 16 == 0 and H % 16 == 0 and H <= 64 and D * (H + 4) * 4 <= LDS_BYTES:
        return "exact", H // 16
    if in_addr % 16 == 0 and D % 16 == 0 and 0 < H <= 128 and D * (16 * Tp + 4) * 4 <= LDS_BYTES:
        return "padded", Tp
    if in_addr % 8 == 0 and D % 2 == 0 and D >= 2 and H <= 64 and 16 * _cdiv(D, 16) * (16 * Tp + 4) * 4 <= LDS_BYTES:
        return "dpad", Tp
    return "any", _cdiv(H, 128)


ALL_CELLS = ({("exact", t) for t in range(1, 5)} | {("padded", t) for t in range(1, 9)} | {("dpad", t) for t in range(1, 5)}
             | {("any", t) for t in range(1, 4)})

# (N, D, H, offset of `in` in floats, layout of W); the allocator's blocks are 16-byte aligned, so offsets 1 and 2 make `in`
# only 4- and 8-byte aligned, 0 and 4 are the aligned controls.  W: "c" contiguous, "t" a transposed view, "s" big[::2, ::3].
UPDATE_TABLE = [
    # exact: T = 1 .. 4, the LDS edges (240, 64) and (304, 48) on the streaming side, the grid-stride loop at 70 001 rows
    (4097, 32, 16, 0, "c"), (17, 64, 32, 4, "t"), (70001, 48, 48, 0, "s"), (15, 304, 48, 0, "c"), (1, 16, 48, 4, "t"),
    (16, 240, 64, 0, "t"), (70001, 96, 64, 4, "c"), (4097, 32, 32, 0, "s"),
    # padded: H off the 16-column grid, T = 1 .. 8, the LDS edge (112, 128)
    (4097, 32, 1, 0, "c"), (70001, 96, 22, 0, "t"), (17, 64, 40, 4, "s"), (16, 32, 60, 0, "c"), (4097, 48, 65, 0, "t"),
    (70001, 32, 80, 0, "s"), (15, 16, 96, 4, "c"), (4097, 64, 97, 0, "t"), (1, 32, 112, 0, "s"), (17, 112, 128, 0, "c"),
    (70001, 16, 128, 4, "t"), (16, 16, 113, 0, "s"),
    # dpad: an even D off the 16-column grid, or a 16-multiple D whose rows are only 8-byte aligned
    (4097, 22, 16, 0, "c"), (70001, 22, 32, 2, "t"), (17, 30, 48, 0, "s"), (16, 64, 64, 2, "c"), (15, 2, 40, 2, "t"),
    (4097, 32, 48, 2, "s"), (1, 96, 1, 2, "c"),
    # the any-shape kernel: odd D, a 4-byte aligned `in`, H > 128 (second and third pass of the h0 loop), the far side of
    # each LDS edge: (256, 64), (320, 48), (128, 128)
    (70001, 7, 5, 0, "c"), (4097, 32, 32, 1, "t"), (17, 64, 48, 1, "s"), (16, 256, 64, 0, "c"), (15, 320, 48, 4, "t"),
    (17, 128, 128, 0, "s"), (4097, 33, 129, 0, "c"), (16, 64, 200, 4, "t"), (1, 15, 257, 1, "s"), (4097, 300, 257, 2, "c"),
    (70001, 16, 129, 0, "t"), (15, 1, 200, 1, "c"), (17, 17, 80, 1, "t"), (16, 96, 16, 1, "s"),
]

SENTINEL = -3.0e38


def _dptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _make_x(N, D, off, dev):
    buf = torch.empty(off + N * D + 3, device=dev)
    return buf[off:off + N * D].view(N, D)


def _make_w(D, H, layout, dev):
    if layout == "c":
        return torch.empty(D, H, device=dev)
    if layout == "t":
        return torch.empty(H, D, device=dev).t()
    return torch.empty(2 * D, 3 * H, device=dev)[::2, ::3]


def _within(got, want, scale):
    """componentwise |got - want| <= 1e-5 * scale; the largest ratio for the message."""
    err = (got.double() - want).abs()
    ok = bool((err <= 1e-5 * scale + 1e-30).all())
    return ok, float((err / (1e-5 * scale + 1e-30)).max()) if err.numel() else 0.0


def _check_update(X, W, ext, tag):
    N, D = X.shape
    H = W.shape[1]
    dev = X.device
    gen = torch.Generator(device=dev).manual_seed(N * 7919 + D * 131 + H)
    # random-normal operands: the 1e-5 bar, determinism, both front-ends the same bits
    X.copy_(torch.randn(N, D, device=dev, generator=gen))
    W.copy_(torch.randn(D, H, device=dev, generator=gen))
    got = hcspmm.update(X, W)
    assert got is not None and got.shape == (N, H), tag
    want = X.double() @ W.double()
    scale = X.double().abs() @ W.double().abs()
    ok, ratio = _within(got, want, scale)
    assert ok, "%s: off by %.3g x the 1e-5 bar" % (tag, ratio)
    assert torch.equal(got, hcspmm.update(X, W)), tag + ": two calls differ"
    assert torch.equal(got, ext.update(X, W)), tag + ": hcspmm.update and HCSPMM.update differ"
    # the C ABI into a sentinel-filled buffer, output at an offset of one float (only 4-byte aligned)
    buf = torch.full((N * H + 65,), SENTINEL, device=dev)
    out = buf[1:1 + N * H].view(N, H)
    rc = capi.lib().hcspmm_dense_update(_dptr(X), _dptr(W), W.stride(0), W.stride(1), _dptr(out), N, D, H, _stream(dev))
    assert rc == capi.OK, "%s: hcspmm_dense_update returned %d" % (tag, rc)
    torch.cuda.synchronize(dev)
    assert bool((buf[:1] == SENTINEL).all()) and bool((buf[1 + N * H:] == SENTINEL).all()), tag + ": wrote outside out"
    ok, ratio = _within(out, want, scale)
    assert ok, "%s (ABI, out + 1 float): off by %.3g x the 1e-5 bar" % (tag, ratio)
    # small-integer operands: exactly the fp64 product
    X.copy_(torch.randint(-2, 3, (N, D), device=dev, generator=gen).float())
    W.copy_(torch.randint(-2, 3, (D, H), device=dev, generator=gen).float())
    want = X.double() @ W.double()
    got = hcspmm.update(X, W)
    assert torch.equal(got.double(), want), "%s: integer product not exact (%d wrong)" % (tag, int((got.double() != want).sum()))
    assert torch.equal(got, ext.update(X, W)), tag + ": front-ends differ (integer operands)"
    buf.fill_(SENTINEL)
    rc = capi.lib().hcspmm_dense_update(_dptr(X), _dptr(W), W.stride(0), W.stride(1), _dptr(out), N, D, H, _stream(dev))
    assert rc == capi.OK
    torch.cuda.synchronize(dev)
    assert torch.equal(out.double(), want), tag + " (ABI, out + 1 float): integer product not exact"
    assert bool((buf[:1] == SENTINEL).all()) and bool((buf[1 + N * H:] == SENTINEL).all()), tag + ": wrote outside out"


def _update_case(N, D, H, off, layout, dev, ext):
    X, W = _make_x(N, D, off, dev), _make_w(D, H, layout, dev)
    r = _route(X.data_ptr(), 0, D, H)  # (out: a fresh allocation, 16-byte aligned)
    assert r == _route(4 * off, 0, D, H), "the allocator's block is not 16-byte aligned: the table's routes do not hold"
    _check_update(X, W, ext, "N=%d D=%d H=%d in+%d W=%s -> %s T=%d" % (N, D, H, off, layout, r[0], r[1]))


def test_update_table_reaches_every_route_and_tile():
    """The case table runs every (route, T) cell of launch_dense_update at least once, and every shape the issue names."""
    hit = {_route(4 * off, 0, D, H) for N, D, H, off, _ in UPDATE_TABLE}
    assert hit == ALL_CELLS, "not reached: %s" % sorted(ALL_CELLS - hit)
    assert {1, 15, 16, 17, 4097, 70001} <= {c[0] for c in UPDATE_TABLE}
    assert {1, 48, 65, 80, 97, 128, 129, 200, 257} <= {c[2] for c in UPDATE_TABLE}
    assert {0, 1, 2, 4} == {c[3] for c in UPDATE_TABLE} and {"c", "t", "s"} == {c[4] for c in UPDATE_TABLE}
    shapes = {(c[1], c[2]) for c in UPDATE_TABLE}
    for streams, falls in (((240, 64), (256, 64)), ((304, 48), (320, 48)), ((112, 128), (128, 128))):
        assert streams in shapes and falls in shapes
        assert _route(0, 0, *streams)[0] != "any" and _route(0, 0, *falls)[0] == "any"
    assert any(c[1] % 2 for c in UPDATE_TABLE) and any(c[1] % 2 == 0 and c[1] % 16 for c in UPDATE_TABLE)
    # an output that is only 4-byte aligned (the ABI checks) moves every exact shape onto the padded kernel, same T
    for _, D, H, off, _ in UPDATE_TABLE:
        r = _route(4 * off, 0, D, H)
        assert _route(4 * off, 4, D, H) == (("padded", r[1]) if r[0] == "exact" else r)


@pytest.mark.parametrize("N,D,H,off,layout", UPDATE_TABLE)
def test_dense_update_dispatch_table(dev, ext, N, D, H, off, layout):
    _update_case(N, D, H, off, layout, dev, ext)


def _sweep_cases(seed, n):
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n):
        N = int(np.exp(rng.uniform(0, np.log(20000)))) if rng.random() < 0.8 else int(rng.integers(1, 20001))
        D = int(rng.integers(1, 301)) if rng.random() < 0.5 else 16 * int(rng.integers(1, 19))
        H = int(rng.integers(1, 261)) if rng.random() < 0.5 else int(rng.integers(1, 129))
        cases.append((N, D, H, int(rng.choice([0, 1, 2, 4])), str(rng.choice(["c", "t", "s"]))))
    return cases


@pytest.mark.parametrize("seed", range(8))
def test_dense_update_random_sweep(dev, ext, seed):
    """25 seeded random shapes per seed (200 in all), offsets and W layouts: combinations the table does not list."""
    for N, D, H, off, layout in _sweep_cases(1000 + seed, 25):
        _update_case(N, D, H, off, layout, dev, ext)


def test_dense_update_declines(dev, ext):
    """Operands the kernel does not take: None (caller: torch.mm) from both front-ends, never an error."""
    X, W = torch.zeros(5, 0, device=dev), torch.zeros(0, 4, device=dev)  # D == 0 (the ABI refuses D <= 0)
    assert hcspmm.update(X, W) is None and ext.update(X, W) is None
    X, W = torch.zeros(5, 8, device=dev), torch.zeros(8, 4, device=dev)
    for fe in (hcspmm, ext):
        assert fe.update(X[:, ::2], W[::2]) is None and fe.update(X.double(), W.double()) is None
        assert fe.update(X.cpu(), W.cpu()) is None and fe.update(X[:0], W) is None and fe.update(X, W[:, :0]) is None


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
WG_TILES = [(dt, ht) for ht in range(1, 5) for dt in range(1, 9) if dt * ht <= 16]
WG_N = [1, 37, 32767, 32785, 100003]


def _wg_groups(N):
    return max(1, min(WG_CAP, _cdiv(N, 64)))


def _wg_supported(D, H):
    dt, ht = _cdiv(D, 16), _cdiv(H, 16)
    return D > 0 and H > 0 and dt <= 8 and ht <= 4 and dt * ht <= 16


def _ragged(t, salt):
    return 16 * t - 1 - (7 * t + 3 * salt) % 15  # 16 t - r, r in 1 .. 15


def _wg_shapes(dt, ht):
    return [(D, H) for D in (16 * dt, _ragged(dt, ht)) for H in (16 * ht, _ragged(ht, dt))]


def test_weight_grad_table_reaches_every_instantiation():
    assert len(WG_TILES) == 25
    hit = {(_cdiv(D, 16), _cdiv(H, 16)) for dt, ht in WG_TILES for D, H in _wg_shapes(dt, ht)}
    assert hit == set(WG_TILES) and all(_wg_supported(D, H) for dt, ht in WG_TILES for D, H in _wg_shapes(dt, ht))
    assert not _wg_supported(129, 16) and not _wg_supported(16, 65) and not _wg_supported(80, 64)
    # the row split: 32 767 -> 512 groups of 64 rows, the last one short; 32 785 -> 512 groups of 80 rows, the trailing
    # ones empty (they must write zero partials)
    for N in (32767, 32785):
        G = _wg_groups(N)
        rows = _cdiv(_cdiv(N, G), 16) * 16
        assert G == WG_CAP and (rows, N % rows) == ((64, 63) if N == 32767 else (80, 65))
        assert N == 32767 or G * rows - N >= rows


def _check_weight_grad(N, D, H, dev, ext):
    tag = "N=%d D=%d H=%d" % (N, D, H)
    gen = torch.Generator(device=dev).manual_seed(N * 31 + D * 7 + H)
    bigA, bigB = torch.empty(N, D + 5, device=dev), torch.empty(N, H + 3, device=dev)
    A, B = bigA[:, 2:2 + D], bigB[:, 1:1 + H]  # lda > D, ldb > H
    ws_bytes = int(capi.lib().hcspmm_weight_grad_workspace(N, D, H))
    assert ws_bytes == _wg_groups(N) * D * H * 4, tag
    ws = torch.empty(ws_bytes // 4, device=dev)
    out = torch.empty(D, H, device=dev)

    def abi():
        ws.fill_(float("nan"))  # every group writes its whole partial, empty groups included
        out.fill_(float("nan"))
        rc = capi.lib().hcspmm_weight_grad(_dptr(A), A.stride(0), _dptr(B), B.stride(0), _dptr(out), N, D, H, _dptr(ws),
                                           ws_bytes, _stream(dev))
        assert rc == capi.OK, "%s: hcspmm_weight_grad returned %d" % (tag, rc)
        return out.clone()

    A.copy_(torch.randn(N, D, device=dev, generator=gen))
    B.copy_(torch.randn(N, H, device=dev, generator=gen))
    got = hcspmm.weight_grad(A, B)
    assert got is not None and got.shape == (D, H), tag
    want = A.double().t() @ B.double()
    scale = A.double().abs().t() @ B.double().abs()
    ok, ratio = _within(got, want, scale)
    assert ok, "%s: off by %.3g x the 1e-5 bar" % (tag, ratio)
    assert torch.equal(got, hcspmm.weight_grad(A, B)), tag + ": two calls differ"
    assert torch.equal(got, ext.weight_grad(A, B)), tag + ": hcspmm.weight_grad and HCSPMM.weight_grad differ"
    assert torch.equal(got, abi()), tag + ": differs with a NaN-filled workspace"
    A.copy_(torch.randint(-2, 3, (N, D), device=dev, generator=gen).float())
    B.copy_(torch.randint(-2, 3, (N, H), device=dev, generator=gen).float())
    want = A.double().t() @ B.double()
    got = hcspmm.weight_grad(A, B)
    assert torch.equal(got.double(), want), "%s: integer product not exact (%d wrong)" % (tag, int((got.double() != want).sum()))
    assert torch.equal(got, ext.weight_grad(A, B)) and torch.equal(got, abi()), tag + ": integer operands, entry points differ"


@pytest.mark.parametrize("dt,ht", WG_TILES)
def test_weight_grad_every_instantiation(dev, ext, dt, ht):
    """dW = A^T B for D = 16 DT and 16 DT - r, H = 16 HT and 16 HT - r, over row counts that leave the last group short
    (32 767), trailing groups empty (32 785) or fill the grid (100 003); A and B column slices of wider matrices."""
    for D, H in _wg_shapes(dt, ht):
        for N in WG_N:
            _check_weight_grad(N, D, H, dev, ext)


def test_weight_grad_declines_and_abi_errors(dev, ext):
    for D, H in ((129, 16), (16, 65), (80, 64), (128, 48)):  # outside the instantiated range
        A, B = torch.zeros(50, D, device=dev), torch.zeros(50, H, device=dev)
        assert hcspmm.weight_grad(A, B) is None and ext.weight_grad(A, B) is None, (D, H)
    # rows that overlap (lda < D): declined, not an error
    row = torch.randn(24, device=dev)
    A, B = row.expand(300, 24), torch.randn(300, 16, device=dev)
    assert A.stride() == (0, 1)
    assert hcspmm.weight_grad(A, B) is None and ext.weight_grad(A, B) is None
    Bx = torch.randn(16, device=dev).expand(300, 16)
    assert hcspmm.weight_grad(B, Bx) is None and ext.weight_grad(B, Bx) is None
    # the C ABI: a short workspace, lda < D
    N, D, H = 300, 24, 16
    A = torch.randn(N, D, device=dev)
    ws_bytes = int(capi.lib().hcspmm_weight_grad_workspace(N, D, H))
    ws, out = torch.zeros(ws_bytes // 4, device=dev), torch.zeros(D, H, device=dev)
    call = capi.lib().hcspmm_weight_grad
    assert call(_dptr(A), D, _dptr(B), H, _dptr(out), N, D, H, _dptr(ws), ws_bytes - 4, _stream(dev)) == capi.EWORKSPACE
    assert call(_dptr(A), D - 1, _dptr(B), H, _dptr(out), N, D, H, _dptr(ws), ws_bytes, _stream(dev)) == capi.EINVAL
    assert call(_dptr(A), D, _dptr(B), H, _dptr(out), N, D, H, _dptr(ws), ws_bytes, _stream(dev)) == capi.OK
    torch.cuda.synchronize(dev)
    assert bool(((out.double() - A.double().t() @ B.double()).abs() <= 1e-5 * (A.double().abs().t() @ B.double().abs())).all())
