"""GATv2 attention without a GPU: the register budgets of its translation unit (cross-compiled for gfx950), the argument
checks hcspmm_gatv2_scores / hcspmm_gatv2_scores_backward make before they touch HIP, the workspace formula, the exported
symbols and the driver's flags."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest

from hcspmm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hc-spmm_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# waves per SIMD of every build.  Scores: (L lanes per entry, LH lanes per head, MULTI)
SCORES_OCCUPANCY = {(1, 1, 0): 8, (2, 1, 0): 8, (2, 2, 0): 8, (4, 1, 0): 8, (4, 2, 0): 8, (4, 4, 0): 8,
                    (8, 1, 0): 8, (8, 2, 0): 8, (8, 4, 0): 7, (8, 8, 0): 8,
                    (16, 1, 0): 8, (16, 2, 0): 8, (16, 4, 0): 7, (16, 8, 0): 7, (16, 16, 0): 7,
                    (32, 1, 0): 8, (32, 2, 0): 8, (32, 4, 0): 7, (32, 8, 0): 7, (32, 16, 0): 7, (32, 32, 0): 7,
                    (64, 1, 0): 8, (64, 2, 0): 7, (64, 4, 0): 7, (64, 8, 0): 7, (64, 16, 0): 7, (64, 32, 0): 7, (64, 64, 0): 7}
SCORES_OCCUPANCY.update({(64, 1, 1): 5, (64, 2, 1): 4, (64, 4, 1): 4, (64, 8, 1): 4, (64, 16, 1): 4, (64, 32, 1): 4, (64, 64, 1): 4})
# grad: (SIDE, L lanes per row); SIDE 0 = dst (also sums the att partials), 1 = src
GRAD_OCCUPANCY = {(0, 1): 4, (0, 2): 4, (0, 4): 4, (0, 8): 4, (0, 16): 4, (0, 32): 4, (0, 64): 5,
                  (1, 1): 5, (1, 2): 5, (1, 4): 5, (1, 8): 5, (1, 16): 5, (1, 32): 5, (1, 64): 6}


@pytest.fixture(scope="module")
def usage():
    cmd = [HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "gatv2_attention.hip"), "-o", os.devnull]
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


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_gatv2_kernels_keep_their_budgets(usage):
    """50 builds: 28 single-pass + 7 multi-pass score kernels, 2 x 7 row kernels, the fold: nothing spilled, occupancy as
    pinned above"""
    assert len(usage) == 50, sorted(usage)
    seen = set()
    for name, v in usage.items():
        assert v["scratch"] == 0, (name, v)
        m = re.search(r"gatv2_scores_kernelILi(\d+)ELi(\d+)ELb([01])E", name)
        if m:
            key = ("scores",) + tuple(int(x) for x in m.groups())
            assert v["occupancy"] == SCORES_OCCUPANCY[key[1:]], (name, v)
        elif re.search(r"gatv2_grad_kernelILi([01])ELi(\d+)E", name):
            m = re.search(r"gatv2_grad_kernelILi([01])ELi(\d+)E", name)
            key = ("grad",) + tuple(int(x) for x in m.groups())
            assert v["occupancy"] == GRAD_OCCUPANCY[key[1:]], (name, v)
        else:
            assert "gatv2_att_fold_kernel" in name, name
            key = ("fold",)
            assert v["occupancy"] == 8, (name, v)
        seen.add(key)
    assert len(seen) == 50


def _vp(v):
    return ctypes.c_void_p(0x1000 if v else 0)  # never dereferenced: every case fails before HIP is touched


def _fwd(hd=1, ld_dst=16, hs=1, src_rows=32, ld_src=16, att=1, slope=0.2, out=1, rp=1, col=1, N=16, E=8, D=16, heads=2):
    return capi.lib().hcspmm_gatv2_scores(_vp(hd), ld_dst, _vp(hs), src_rows, ld_src, _vp(att), slope, _vp(out), _vp(rp), _vp(col),
                                          N, E, D, heads, ctypes.c_void_p(0))


def _bwd(g=1, hd=1, ld_dst=16, hs=1, ld_src=16, att=1, slope=0.2, rp=1, col=1, perm=1, N=16, E=8, D=16, heads=2, gd=1, ld_gdst=16,
         gs=1, ld_gsrc=16, ga=1, ws=1, ws_bytes=1 << 20):
    return capi.lib().hcspmm_gatv2_scores_backward(_vp(g), _vp(hd), ld_dst, _vp(hs), ld_src, _vp(att), slope, _vp(rp), _vp(col),
                                                   _vp(perm), N, E, D, heads, _vp(gd), ld_gdst, _vp(gs), ld_gsrc, _vp(ga), _vp(ws),
                                                   ws_bytes, ctypes.c_void_p(0))


BAD_SLOPES = [float("nan"), float("inf"), -float("inf")]
BAD_SHAPES = [dict(heads=0), dict(heads=-3), dict(D=0), dict(D=-16), dict(heads=3), dict(D=12, heads=2), dict(D=2, heads=1)]


@pytest.mark.parametrize("case", [dict(hd=0), dict(hs=0), dict(att=0), dict(out=0), dict(rp=0), dict(col=0), dict(N=-1), dict(E=-1),
                                  dict(src_rows=-1), dict(N=0), dict(src_rows=0), dict(ld_dst=15), dict(ld_src=15)] + BAD_SHAPES +
                         [dict(slope=s) for s in BAD_SLOPES])
def test_forward_argument_checks(case):
    assert _fwd(**case) == capi.EINVAL


def test_forward_without_entries_launches_nothing():
    assert _fwd(out=0, col=0, E=0) == 0
    assert _fwd(hd=0, hs=0, out=0, col=0, N=0, E=0, src_rows=0) == 0


@pytest.mark.parametrize("case", [dict(g=0), dict(hd=0), dict(hs=0), dict(att=0), dict(rp=0), dict(col=0), dict(perm=0), dict(gd=0),
                                  dict(gs=0), dict(ga=0), dict(ws=0), dict(N=-1), dict(E=-1), dict(N=0), dict(ld_dst=15),
                                  dict(ld_src=15), dict(ld_gdst=15), dict(ld_gsrc=15)] + BAD_SHAPES +
                         [dict(slope=s) for s in BAD_SLOPES])
def test_backward_argument_checks(case):
    assert _bwd(**case) == capi.EINVAL


def test_backward_refuses_a_short_workspace():
    need = capi.lib().hcspmm_gatv2_backward_workspace_bytes(16, 8, 16, 2)
    assert need > 0
    assert _bwd(ws_bytes=need - 1) == capi.EWORKSPACE
    assert _bwd(ws_bytes=0, ws=0) == capi.EWORKSPACE
    assert _bwd(ws_bytes=need - 1, heads=0) == capi.EINVAL  # argument errors come first


def test_workspace_formula():
    """one [D] fp32 partial per workgroup of the row launches: one workgroup per tile of 4 waves x (64 / L) lane groups x 4
    rows, at most 4096 (beyond, a workgroup takes several tiles); L = the fewest power-of-two lanes whose 4 columns each
    cover D (at most 64)"""
    ws = capi.lib().hcspmm_gatv2_backward_workspace_bytes
    for N in (1, 15, 16, 17, 1000, 233000, 4859280):
        for D, heads in ((4, 1), (8, 2), (12, 1), (32, 8), (64, 4), (96, 2), (256, 4), (320, 1), (512, 8)):
            L = 1
            while L * 4 < D and L < 64:
                L *= 2
            rows = 4 * (64 // L) * 4
            assert ws(N, 10, D, heads) == min(-(-N // rows), 4096) * D * 4, (N, D, heads)
            assert ws(N, 0, D, heads) == ws(N, 10 ** 9, D, heads)  # the grid does not depend on E
    for bad in ((0, 0, 16, 2), (-1, 0, 16, 2), (16, -1, 16, 2), (16, 8, 16, 0), (16, 8, 12, 2), (16, 8, 16, 3), (16, 8, 0, 1)):
        assert ws(*bad) == 0, bad


def test_symbols_are_exported_and_declared():
    lib = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    for name in ("hcspmm_gatv2_scores", "hcspmm_gatv2_backward_workspace_bytes", "hcspmm_gatv2_scores_backward"):
        assert getattr(lib, name) is not None
        assert name in capi.SYMBOLS and re.search(r"\b%s\(" % name, header), name
    assert capi.lib().hcspmm_abi_version() == 3  # additions only
    import hcspmm
    assert "gatv2_scores" in hcspmm.__all__ and "gatv2_scores_backward" in hcspmm.__all__


def test_driver_gatv2_flags():
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_gatv2_cpu", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(["--model", "gatv2", "--heads", "4", "--gat-concat"])
    assert args.model == "gatv2" and args.heads == 4 and args.gat_concat
    for bad in (["--norm", "sym"], ["--hidden", "30"], ["--heads", "0"], ["--gat-concat", "--heads", "3"]):
        with pytest.raises(SystemExit):
            mod.parse_args(["--model", "gatv2"] + bad)
