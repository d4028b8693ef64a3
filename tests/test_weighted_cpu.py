"""Edge-weighted aggregation without a GPU: the weighted translation units' register budgets (cross-compiled for gfx950),
the host transpose permutation against scipy, and the argument checks hcspmm_forward_weighted / hcspmm_edge_norm_device make
before they touch HIP."""
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


def _resource_usage(unit):
    cmd = [HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, unit), "-o", os.devnull]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-2000:]
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


@pytest.fixture(scope="module")
def usage():
    from concurrent.futures import ThreadPoolExecutor
    units = ("spmm_weighted.hip", "spmm_weighted_h16.hip")
    with ThreadPoolExecutor(2) as ex:
        return dict(zip(units, ex.map(_resource_usage, units)))


def _plan_args(name):
    """hybrid_plan_w_kernel<E, L, VEC, UNROLL, MINW> -> (E, L, VEC, UNROLL, MINW)"""
    m = re.search(r"hybrid_plan_w_kernelINS_(\w+?)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE", name)
    return (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5))) if m else None


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_weighted_fp32_kernels_keep_their_budgets(usage):
    """fp32 planned: five waves per SIMD like the binary kernel; nothing spilled except the L = 32 build (36 bytes) and the
    8-byte-lane build of D = 2, 3 (20, the binary kernel's own reload) -- DESIGN.md section 5.  Tiny-task launch: 8 / 0."""
    u = usage["spmm_weighted.hip"]
    plan = {n: v for n, v in u.items() if _plan_args(n)}
    assert len(plan) == 7, sorted(u)
    for n, v in plan.items():
        a = _plan_args(n)
        assert v["occupancy"] >= 5 and v["vgprs"] <= 96, (a, v)
        assert v["scratch"] <= (36 if a[1] == 32 else 20), (a, v)
    tiny = {n: v for n, v in u.items() if "tiny_w_kernel" in n}
    assert len(tiny) == 7
    for n, v in tiny.items():
        assert v["occupancy"] >= 8 and v["scratch"] == 0, (n, v)
    window = {n: v for n, v in u.items() if "hybrid_window_w_kernel" in n}
    assert len(window) == 7
    for n, v in window.items():
        assert v["occupancy"] >= 4 and v["scratch"] == 0, (n, v)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_weighted_16bit_kernels_keep_their_budgets(usage):
    """16-bit planned: four waves per SIMD like the binary builds; at most the 20-byte reload, except the fp16 L = 32
    16-byte-lane build (96 bytes).  Tiny-task launch: eight waves; the fp16 16-byte-lane builds reload 76 bytes."""
    u = usage["spmm_weighted_h16.hip"]
    plan = {n: v for n, v in u.items() if _plan_args(n)}
    assert len(plan) == 30, sorted(u)
    for n, v in plan.items():
        a = _plan_args(n)
        assert v["occupancy"] >= 4, (a, v)
        assert v["scratch"] <= (96 if (a[0], a[1], a[2]) == ("3F16", 32, 8) else 20), (a, v)
    tiny = {n: v for n, v in u.items() if "tiny_w_kernel" in n}
    assert len(tiny) == 30
    for n, v in tiny.items():
        assert v["occupancy"] >= 8, (n, v)
        assert v["scratch"] <= (76 if ("3F16" in n and "ELi8EEEv" in n) else 0), (n, v)
    for n, v in u.items():
        if "hybrid_window_w_kernel" in n:
            assert v["occupancy"] >= 3 and v["scratch"] == 0, (n, v)


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else ctypes.c_void_p(0)


def _transpose_permutation(rp, col):
    rp, col = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(col, np.int32)
    perm = np.full(len(col), -1, np.int32)
    rc = capi.lib().hcspmm_transpose_permutation(_ptr(rp), _ptr(col), len(rp) - 1, len(col), _ptr(perm))
    return rc, perm


@pytest.mark.parametrize("kind", ["powerlaw", "community", "powerlaw_self_loops"])
def test_transpose_permutation_matches_scipy(kind):
    sp = pytest.importorskip("scipy.sparse")
    if kind == "community":
        rp, col = graphs.community_graph(3000, 30000, seed=3)[:2]
        A = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(len(rp) - 1,) * 2)
        A = ((A + A.T) > 0).astype(np.float64).tocsr()  # a symmetric pattern
        A.sort_indices()
        rp, col = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    else:
        rp, col = graphs.powerlaw_graph(4000, 50000, seed=4)
        if kind == "powerlaw_self_loops":
            A = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(len(rp) - 1,) * 2) + sp.identity(len(rp) - 1)
            A = (A > 0).astype(np.float64).tocsr()
            A.sort_indices()
            rp, col = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    N, E = len(rp) - 1, len(col)
    vals = np.random.default_rng(5).standard_normal(E)  # asymmetric values on a symmetric pattern
    rc, perm = _transpose_permutation(rp, col)
    assert rc == 0
    assert np.array_equal(np.sort(perm), np.arange(E))
    At = sp.csr_matrix((vals, col, rp), shape=(N, N)).T.tocsr()
    At.sort_indices()
    assert np.array_equal(At.indptr, rp) and np.array_equal(At.indices, col)
    assert np.array_equal(At.data, vals[perm])


def test_transpose_permutation_refuses_an_asymmetric_pattern():
    rp, col = graphs.uniform_graph(500, 3000, seed=6)
    rc, _ = _transpose_permutation(rp, col)
    assert rc == capi.EINVAL
    rc, _ = _transpose_permutation(np.array([0, 1, 1], np.int32), np.array([1], np.int32))  # (0, 1) without (1, 0)
    assert rc == capi.EINVAL
    rc, perm = _transpose_permutation(np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    assert rc == 0 and list(perm) == [1, 0]


def _fw(X=1, Z=1, N=16, E=8, D=4, ldx=4, ldz=4, dtype=0, values=1, rp=1, col=1, x_rows=16):
    vp = lambda v: ctypes.c_void_p(0x1000 if v else 0)  # never dereferenced: every case fails before HIP is touched
    return capi.lib().hcspmm_forward_weighted(vp(X), x_rows, ldx, vp(Z), ldz, dtype, vp(rp), vp(col), vp(1), vp(1), vp(1), vp(1),
                                              ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), 0, ctypes.c_void_p(0),
                                              vp(values))


@pytest.mark.parametrize("case", [dict(values=0), dict(values=0, N=0), dict(D=0), dict(ldx=3), dict(ldz=2), dict(N=-1),
                                  dict(E=-1), dict(dtype=3), dict(X=0), dict(Z=0), dict(rp=0), dict(col=0)])
def test_forward_weighted_argument_checks(case):
    assert _fw(**case) == capi.EINVAL


def test_edge_norm_argument_checks():
    L = capi.lib()
    one = ctypes.c_void_p(0x1000)
    assert L.hcspmm_edge_norm_device(one, one, 4, 8, 2, one, None) == capi.EINVAL  # unknown kind
    assert L.hcspmm_edge_norm_device(one, one, -1, 8, 0, one, None) == capi.EINVAL
    assert L.hcspmm_edge_norm_device(one, one, 4, 8, 1, ctypes.c_void_p(0), None) == capi.EINVAL
    assert L.hcspmm_edge_norm_device(one, one, 0, 8, 0, one, None) == capi.EINVAL  # entries without rows
