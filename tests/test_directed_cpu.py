"""Directed graphs without a GPU: the host transpose (hcspmm_transpose_graph) against scipy, its symmetric special case
(hcspmm_transpose_permutation), its refusals, the argument checks the three new device entry points make before they touch
HIP, and the register budgets of the indexed-values translation unit (cross-compiled for gfx950)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hcspmm import capi, graphs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hc-spmm_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else ctypes.c_void_p(0)


GUARD = 7  # words behind every output, checked to be untouched


def _transpose_graph(rp, col, num_cols=None):
    rp, col = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(col, np.int32)
    N, E = len(rp) - 1, len(col)
    M = N if num_cols is None else num_cols
    rp_t = np.full(M + 1 + GUARD, -77, np.int32)
    col_t = np.full(E + GUARD, -77, np.int32)
    eid_t = np.full(E + GUARD, -77, np.int32)
    rc = capi.lib().hcspmm_transpose_graph(_ptr(rp), _ptr(col), N, M, E, _ptr(rp_t), _ptr(col_t), _ptr(eid_t))
    for a, n in ((rp_t, M + 1), (col_t, E), (eid_t, E)):
        assert (a[n:] == -77).all(), "written out of bounds"
    return rc, rp_t[:M + 1], col_t[:E], eid_t[:E]


def _asymmetric(kind):
    if kind == "uniform":
        return graphs.uniform_graph(500, 3000, seed=6)
    if kind == "powerlaw":
        return graphs.powerlaw_graph(3000, 40000, seed=3, symmetric=False)
    if kind == "powerlaw_hubs":
        return graphs.powerlaw_graph(3000, 60000, seed=4, symmetric=False, max_degree_frac=0.9)
    return graphs.planted_dense_graph(1200, seed=8)


ASYMMETRIC = {"uniform": (500, 3000), "powerlaw": (3000, 40000), "powerlaw_hubs": (3000, 60000), "planted": (1200, 10779)}


def _check_against_scipy(rp, col, n_cols):
    sp = pytest.importorskip("scipy.sparse")
    N, E = len(rp) - 1, len(col)
    vals = np.random.default_rng(5).standard_normal(E)
    rc, rp_t, col_t, eid_t = _transpose_graph(rp, col, n_cols)
    assert rc == 0
    At = sp.csr_matrix((vals, col, rp), shape=(N, n_cols)).T.tocsr()
    At.sort_indices()
    assert np.array_equal(At.indptr, rp_t) and np.array_equal(At.indices, col_t)
    assert np.array_equal(At.data, vals[eid_t])
    assert np.array_equal(np.sort(eid_t), np.arange(E))


@pytest.mark.parametrize("kind", list(ASYMMETRIC))
def test_transpose_graph_matches_scipy(kind):
    sp = pytest.importorskip("scipy.sparse")
    rp, col = _asymmetric(kind)
    N, E = len(rp) - 1, len(col)
    assert (N, E) == ASYMMETRIC[kind]
    rows = np.repeat(np.arange(N), np.diff(rp))
    assert all((np.diff(col[rp[r]:rp[r + 1]]) > 0).all() for r in range(N)), "the generator left the input contract"
    A = sp.csr_matrix((np.ones(E), col, rp), shape=(N, N))
    assert A.multiply(A.T).nnz < E, "the pattern is symmetric: the case would not tell A from A^T"
    if kind == "powerlaw_hubs":
        assert np.bincount(col, minlength=N).max() == 1277  # the maximum in-degree the case was chosen for
    assert len(rows) == E
    _check_against_scipy(rp, col, N)


def test_transpose_graph_of_a_rectangular_block():
    rp, col = graphs.powerlaw_block(700, 2500, 9000, seed=2)
    assert len(rp) == 701 and len(col) == 9000
    _check_against_scipy(rp, col, 2500)
    rc = _transpose_graph(rp, col, int(col.max()))[0]  # one column too few
    assert rc == capi.EINVAL


def _symmetric(kind):
    sp = pytest.importorskip("scipy.sparse")
    if kind == "community":
        rp, col = graphs.community_graph(3000, 30000, seed=3)[:2]
        A = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(len(rp) - 1,) * 2)
        A = ((A + A.T) > 0).astype(np.float64).tocsr()
    else:
        rp, col = graphs.powerlaw_graph(4000, 50000, seed=4)
        if kind == "powerlaw":
            return rp, col
        A = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(len(rp) - 1,) * 2) + sp.identity(len(rp) - 1)
        A = (A > 0).astype(np.float64).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32)


@pytest.mark.parametrize("kind", ["powerlaw", "community", "powerlaw_self_loops"])
def test_symmetric_pattern_gives_the_transpose_permutation(kind):
    """the graphs of test_weighted_cpu.py::test_transpose_permutation_matches_scipy: the outputs are (rp, col, perm)"""
    rp, col = _symmetric(kind)
    E = len(col)
    perm = np.full(E, -1, np.int32)
    assert capi.lib().hcspmm_transpose_permutation(_ptr(rp), _ptr(col), len(rp) - 1, E, _ptr(perm)) == 0
    rc, rp_t, col_t, eid_t = _transpose_graph(rp, col)
    assert rc == 0
    assert np.array_equal(rp_t, rp) and np.array_equal(col_t, col) and np.array_equal(eid_t, perm)


@pytest.mark.parametrize("case", ["unsorted", "duplicate", "column_too_large", "negative_column"])
def test_transpose_graph_refuses_bad_rows(case):
    rp = np.array([0, 3, 5], np.int32)
    col = {"unsorted": [0, 2, 1, 0, 1], "duplicate": [0, 1, 1, 0, 1], "column_too_large": [0, 1, 3, 0, 1],
           "negative_column": [-1, 1, 2, 0, 1]}[case]
    rc, rp_t, col_t, eid_t = _transpose_graph(rp, np.array(col, np.int32), 3)
    assert rc == capi.EINVAL
    assert (rp_t == -77).all() and (col_t == -77).all() and (eid_t == -77).all()  # refused before anything is written
    assert _transpose_graph(rp, np.array([0, 1, 2, 0, 1], np.int32), 3)[0] == 0


def test_transpose_graph_refuses_null_outputs_and_negative_sizes():
    L = capi.lib()
    rp, col = np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32)
    out = [np.zeros(3, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)]
    null = ctypes.c_void_p(0)
    for k in range(3):
        ptrs = [_ptr(o) for o in out]
        ptrs[k] = null
        assert L.hcspmm_transpose_graph(_ptr(rp), _ptr(col), 2, 2, 2, *ptrs) == capi.EINVAL
    ptrs = [_ptr(o) for o in out]
    assert L.hcspmm_transpose_graph(null, _ptr(col), 2, 2, 2, *ptrs) == capi.EINVAL
    assert L.hcspmm_transpose_graph(_ptr(rp), null, 2, 2, 2, *ptrs) == capi.EINVAL
    for n, m, e in ((-1, 2, 2), (2, -1, 2), (2, 2, -1)):
        assert L.hcspmm_transpose_graph(_ptr(rp), _ptr(col), n, m, e, *ptrs) == capi.EINVAL
    assert L.hcspmm_transpose_graph(_ptr(rp), _ptr(col), 2, 2, 1, *ptrs) == capi.EINVAL  # row_pointers[N] != E
    assert L.hcspmm_transpose_graph(_ptr(rp), _ptr(col), 2, 2, 2, *ptrs) == 0


def test_transpose_graph_of_nothing():
    rc, rp_t, col_t, eid_t = _transpose_graph(np.zeros(6, np.int32), np.zeros(0, np.int32), 4)  # E = 0
    assert rc == 0 and np.array_equal(rp_t, np.zeros(5, np.int32))
    rc, rp_t, _, _ = _transpose_graph(np.zeros(1, np.int32), np.zeros(0, np.int32))  # N = 0
    assert rc == 0 and list(rp_t) == [0]
    rc, rp_t, _, _ = _transpose_graph(np.zeros(1, np.int32), np.zeros(0, np.int32), 3)  # no rows, three columns
    assert rc == 0 and list(rp_t) == [0, 0, 0, 0]


# ---------------------------------------------------------------- argument checks before any HIP call
def _vp(v):
    return ctypes.c_void_p(0x1000 if v else 0)  # never dereferenced: every case fails before HIP is touched


def _fwi(X=1, Z=1, dtype=0, rp=1, col=1, N=64, E=100, D=32, ldx=None, ldz=None, values=1, heads=4, vindex=1, num_values=100):
    return capi.lib().hcspmm_forward_weighted_indexed(_vp(X), N, ldx or D, _vp(Z), ldz or D, dtype, _vp(rp), _vp(col), _vp(1),
                                                      _vp(1), _vp(1), _vp(1), ctypes.c_void_p(0), None, N, E, D,
                                                      ctypes.c_void_p(0), 0, ctypes.c_void_p(0), _vp(values), heads, _vp(vindex),
                                                      num_values)


@pytest.mark.parametrize("case", [dict(vindex=0), dict(values=0), dict(num_values=-1), dict(num_values=0), dict(dtype=1),
                                  dict(dtype=2), dict(D=24, heads=4), dict(D=12, heads=2), dict(D=30, heads=4), dict(heads=0),
                                  dict(heads=-1), dict(X=0), dict(Z=0), dict(rp=0), dict(col=0), dict(D=0), dict(N=-1),
                                  dict(E=-1), dict(ldx=16), dict(dtype=7), dict(heads=1, D=6, dtype=1)])
def test_forward_weighted_indexed_argument_checks(case):
    assert _fwi(**case) == capi.EINVAL


def test_forward_weighted_indexed_of_no_rows_launches_nothing():
    assert _fwi(N=0) == 0
    assert _fwi(N=0, heads=1, D=6) == 0  # one head takes any width


def _gat_bwd(alpha=1, ga=1, s_dst=1, s_src=1, rp=1, col=1, rp_t=1, eid_t=1, src_rows=16, N=16, E=8, heads=2, out=1, gd=1,
             gs=1, slope=0.2):
    return capi.lib().hcspmm_gat_attention_backward_directed(_vp(alpha), _vp(ga), _vp(s_dst), _vp(s_src), slope, _vp(rp), _vp(col),
                                                             _vp(rp_t), _vp(eid_t), src_rows, N, E, heads, _vp(out), _vp(gd),
                                                             _vp(gs), ctypes.c_void_p(0))


@pytest.mark.parametrize("case", [dict(rp_t=0), dict(eid_t=0), dict(src_rows=-1), dict(rp=0), dict(col=0), dict(alpha=0),
                                  dict(ga=0), dict(s_dst=0), dict(s_src=0), dict(out=0), dict(gd=0), dict(gs=0), dict(heads=0),
                                  dict(N=-1), dict(E=-1), dict(slope=float("nan")), dict(src_rows=0)])
def test_gat_attention_backward_directed_argument_checks(case):
    assert _gat_bwd(**case) == capi.EINVAL


def _v2_bwd(g=1, H_dst=1, H_src=1, att=1, rp=1, col=1, rp_t=1, col_t=1, eid_t=1, src_rows=16, N=16, E=8, D=16, heads=2, ld=None,
            gd=1, gs=1, ga=1, ws=1, ws_bytes=1 << 20, slope=0.2):
    ld = ld or D
    return capi.lib().hcspmm_gatv2_scores_backward_directed(_vp(g), _vp(H_dst), ld, _vp(H_src), ld, _vp(att), slope, _vp(rp),
                                                            _vp(col), _vp(rp_t), _vp(col_t), _vp(eid_t), src_rows, N, E, D, heads,
                                                            _vp(gd), ld, _vp(gs), ld, _vp(ga), _vp(ws), ws_bytes,
                                                            ctypes.c_void_p(0))


@pytest.mark.parametrize("case", [dict(rp_t=0), dict(col_t=0), dict(eid_t=0), dict(src_rows=-1), dict(D=12, heads=2),
                                  dict(D=18, heads=4), dict(heads=0), dict(rp=0), dict(col=0), dict(g=0), dict(H_dst=0),
                                  dict(H_src=0), dict(att=0), dict(gd=0), dict(gs=0), dict(ga=0), dict(ld=8), dict(N=-1),
                                  dict(E=-1), dict(slope=float("inf")), dict(src_rows=0)])
def test_gatv2_scores_backward_directed_argument_checks(case):
    assert _v2_bwd(**case) == capi.EINVAL


def test_gatv2_scores_backward_directed_needs_its_workspace():
    assert _v2_bwd(ws_bytes=0) == capi.EWORKSPACE


def test_abi_version_is_unchanged():
    assert capi.lib().hcspmm_abi_version() == 3


# ---------------------------------------------------------------- register budgets of the indexed kernels
def _usage(src):
    cmd = [HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", os.devnull]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-2000:]
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_indexed_kernels_keep_the_heads_kernels_occupancy():
    """the occupancies pinned for the heads kernels (test_heads_cpu.py BUDGETS): 5 waves per SIMD planned, 8 tiny, 4 plan-free.
    No scratch, except the 20-byte reload of the planned L = 32 build (its weighted counterpart is allowed 36: DESIGN.md
    section 3.14).  The indexed builds are the heads kernels' templates with INDEXED = true (spmm_weighted_heads_impl.h), so they
    carry the same kernel names."""
    usage = _usage("spmm_weighted_indexed.hip")
    assert all("Lb1E" in name or "fixup_kernel" in name for name in usage), sorted(usage)  # every build is the indexed form
    floors = {"hybrid_plan_wh_kernel": 5, "tiny_wh_kernel": 8, "hybrid_window_wh_kernel": 4, "fixup_kernel": 7}
    seen = {k: 0 for k in floors}
    for name, v in usage.items():
        kernel = next((k for k in floors if k in name), None)
        assert kernel is not None, name
        seen[kernel] += 1
        assert v["occupancy"] >= floors[kernel], (name, v)
        l32 = kernel == "hybrid_plan_wh_kernel" and "ELi32ELi4E" in name
        assert v["scratch"] <= (20 if l32 else 0), (name, v)
    assert seen == {"hybrid_plan_wh_kernel": 7, "tiny_wh_kernel": 7, "hybrid_window_wh_kernel": 7, "fixup_kernel": 3}, seen
