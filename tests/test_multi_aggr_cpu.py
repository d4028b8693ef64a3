"""One-pass sum / sum-of-squares / max / min aggregation without a GPU: the register budgets of spmm_multi.hip (cross-compiled
for gfx950), the argument checks hcspmm_forward_multi makes before it touches HIP, the driver's flags, and PNAConv's
post-processing (mean, std, degree scalers, delta) against a hand-written torch expression on precomputed aggregates."""
import ctypes
import importlib.util
import math
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

from hcspmm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hc-spmm_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# waves per SIMD by kernel and build: (L lanes per row, VEC floats per lane); every one without scratch
PLAN_OCC = {(4, 4): 5, (8, 4): 4, (16, 4): 5, (32, 4): 5, (64, 4): 5, (4, 2): 4, (4, 1): 7}
WINDOW_OCC = {(4, 4): 5, (8, 4): 5, (16, 4): 5, (32, 4): 5, (64, 4): 5, (4, 2): 4, (4, 1): 8}
FIXUP_OCC = {4: 5, 2: 8, 1: 8}  # multi_fixup_kernel<VEC>


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


def _expected(name):
    """(pinned occupancy, floats per lane) of a kernel of the unit"""
    m = re.search(r"multi_plan_kernelILi(\d+)ELi(\d+)ELi\d+EE", name)
    if m:
        return PLAN_OCC[(int(m.group(1)), int(m.group(2)))], int(m.group(2))
    m = re.search(r"multi_window_kernelILi(\d+)ELi(\d+)ELi\d+EE", name)
    if m:
        return WINDOW_OCC[(int(m.group(1)), int(m.group(2)))], int(m.group(2))
    m = re.search(r"multi_fixup_kernelILi(\d+)EE", name)
    if m:
        return FIXUP_OCC[int(m.group(1))], int(m.group(1))
    return None


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_multi_kernels_keep_their_budgets():
    """L = 4 ... 64 at 16-byte lanes and L = 4 at 8- / 4-byte lanes, planned and plan-free, and the three fix-up builds: no
    scratch anywhere, occupancy as pinned above and at least four waves per SIMD on every 16-byte-lane build"""
    usage = _usage("spmm_multi.hip")
    assert len(usage) == 17, sorted(usage)
    for name, v in usage.items():
        want = _expected(name)
        assert want is not None, name
        assert (v["scratch"], v["occupancy"]) == (0, want[0]), (name, v)
        if want[1] == 4:
            assert v["occupancy"] >= 4, (name, v)


def _vp(v):
    return ctypes.c_void_p(0x1000 if v else 0)  # never dereferenced: every case fails before HIP is touched


def _fm(X=1, dtype=0, zsum=1, zsumsq=1, zmax=1, zmin=1, amax=1, amin=1, rp=1, col=1, bp=1, e2c=1, e2r=1, ht=1, N=64, E=100, D=32,
        ldx=None, ldz=None, ldarg=None):
    return capi.lib().hcspmm_forward_multi(_vp(X), N, ldx or D, dtype, _vp(zsum), _vp(zsumsq), _vp(zmax), _vp(zmin), ldz or D,
                                           _vp(amax), _vp(amin), ldarg or D, _vp(rp), _vp(col), _vp(bp), _vp(e2c), _vp(e2r), _vp(ht),
                                           ctypes.c_void_p(0), None, N, E, D, ctypes.c_void_p(0), 0, ctypes.c_void_p(0))


@pytest.mark.parametrize("case", [dict(dtype=1), dict(dtype=2), dict(dtype=7), dict(dtype=-1),
                                  dict(zsum=0, zsumsq=0, zmax=0, zmin=0), dict(zsum=0, zsumsq=0, zmax=0, zmin=0, amax=0, amin=0),
                                  dict(ldx=16), dict(ldz=16), dict(ldarg=16), dict(ldarg=16, amax=0), dict(ldarg=16, amin=0),
                                  dict(X=0), dict(rp=0), dict(col=0), dict(bp=0), dict(ht=0), dict(e2c=0), dict(D=0), dict(N=-1),
                                  dict(E=-1)])
def test_forward_multi_argument_checks(case):
    assert _fm(**case) == capi.EINVAL


def test_forward_multi_nothing_to_do_and_nullable_outputs():
    assert _fm(N=0) == 0  # no rows, no launch
    assert _fm(N=0, amax=0, amin=0, ldarg=1) == 0  # both args NULL: their stride is not looked at
    for only in ("zsum", "zsumsq", "zmax", "zmin"):  # any single value output is a valid call
        assert _fm(N=0, **{k: int(k == only) for k in ("zsum", "zsumsq", "zmax", "zmin")}) == 0
    assert capi.lib().hcspmm_multi_workspace_bytes(None, 32) == 0


def test_symbols_and_abi_version():
    for name in ("hcspmm_forward_multi", "hcspmm_multi_workspace_bytes"):
        assert name in capi.SYMBOLS
        assert getattr(capi.lib(), name) is not None
    with open(os.path.join(ROOT, "include", "hcspmm.h")) as f:
        header = f.read()
    assert re.search(r"\bint hcspmm_forward_multi\(", header) and re.search(r"\bsize_t hcspmm_multi_workspace_bytes\(", header)
    assert re.search(r"#define HCSPMM_ABI_VERSION 3\b", header)
    assert capi.lib().hcspmm_abi_version() == 3
    assert len(capi.SYMBOLS["hcspmm_forward_multi"][1]) == 26


def _pkg_imports():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _driver():
    _pkg_imports()
    spec = importlib.util.spec_from_file_location("hc_spmm_main_pna", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_pna_flags():
    mod = _driver()
    args = mod.parse_args(["--model", "pna"])
    assert args.model == "pna"
    assert mod.parse_args(["--model", "pna", "--directed"]).directed
    for extra in (["--norm", "sym"], ["--norm", "mean"], ["--aggr", "max"], ["--aggr", "mean"]):
        with pytest.raises(SystemExit):
            mod.parse_args(["--model", "pna"] + extra)
    # what --model sage had stays: max by default, sum rejected
    assert mod.parse_args(["--model", "sage"]).aggr == "max"
    with pytest.raises(SystemExit):
        mod.parse_args(["--model", "sage", "--aggr", "sum"])


def _aggregates(seed, N, D):
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 9, (N,), generator=g)
    deg[::5] = 0  # rows without entries: deg clamps to 1, every aggregate is 0
    rp = torch.zeros(N + 1, dtype=torch.int32)
    rp[1:] = torch.cumsum(deg, 0)
    # aggregates of some per-row samples, so that sumsq / deg - mean^2 is a real variance (and sometimes rounds below 0)
    s, q = torch.zeros(N, D), torch.zeros(N, D)
    mx, mn = torch.zeros(N, D), torch.zeros(N, D)
    for r in range(N):
        if deg[r] > 0:
            x = torch.randn(int(deg[r]), D, generator=g) if r % 3 else torch.full((int(deg[r]), D), 0.1 * r)
            s[r], q[r], mx[r], mn[r] = x.sum(0), (x * x).sum(0), x.max(0).values, x.min(0).values
    return rp, s, q, mx, mn


@pytest.mark.parametrize("avg_log_deg", [None, 1.7])
def test_pnaconv_post_processing(avg_log_deg):
    _pkg_imports()
    import GNN_model
    N, D = 40, 5
    rp, s, q, mx, mn = _aggregates(3, N, D)
    conv = GNN_model.PNAConv(D, 3, avg_log_deg=avg_log_deg)
    assert conv.weights_root.shape == (D, 3) and conv.weights_neigh.shape == (12 * D, 3)
    got = conv.scaled_aggregates(s, q, mx, mn, rp)
    # by hand: deg = clamp(row length, 1); delta = mean log(deg + 1)
    deg = torch.tensor([max(int(rp[i + 1] - rp[i]), 1) for i in range(N)], dtype=torch.float32)[:, None]
    delta = avg_log_deg if avg_log_deg is not None else sum(math.log(float(d) + 1.0) for d in deg[:, 0]) / N
    mean = s / deg
    std = (torch.clamp(q / deg - mean ** 2, min=0.0) + 1e-5) ** 0.5
    base = torch.cat([mean, mn, mx, std], 1)
    want = torch.cat([base, base * torch.log(deg + 1) / delta, base * delta / torch.log(deg + 1)], 1)
    assert got.shape == (N, 12 * D)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6)
    empty = (rp[1:] == rp[:-1])
    assert torch.equal(got[empty][:, :3 * D], torch.zeros(int(empty.sum()), 3 * D))
    torch.testing.assert_close(got[empty][:, 3 * D:4 * D], torch.full((int(empty.sum()), D), math.sqrt(1e-5)))


def test_pnaconv_subsets_and_refusals():
    _pkg_imports()
    import GNN_model
    N, D = 24, 4
    rp, s, q, mx, mn = _aggregates(4, N, D)
    conv = GNN_model.PNAConv(D, 2, aggregators=("max", "std"), scalers=("attenuation",), avg_log_deg=2.0)
    assert conv.weights_neigh.shape == (2 * D, 2)
    deg = (rp[1:] - rp[:-1]).clamp(min=1).float()[:, None]
    std = torch.sqrt(torch.clamp(q / deg - (s / deg) ** 2, min=0.0) + 1e-5)
    torch.testing.assert_close(conv.scaled_aggregates(s, q, mx, mn, rp), torch.cat([mx, std], 1) * 2.0 / torch.log(deg + 1))
    for bad in (dict(aggregators=("median",)), dict(aggregators=("sum",)), dict(scalers=("linear",)), dict(aggregators=())):
        with pytest.raises(ValueError):
            GNN_model.PNAConv(D, 2, **bad)
