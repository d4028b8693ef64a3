"""8-bit (e4m3fn) feature storage without a GPU: the new symbols are exported and declared, the ABI version stands, and
hcspmm_quantize_fp8 / hcspmm_forward_fp8 return every argument error before they touch HIP (include/hcspmm.h)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hcspmm
from hcspmm import capi, graphs
from hcspmm.capi import Header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hcspmm_quantize_fp8", "hcspmm_forward_fp8", "hcspmm_wide_threshold_fp8")


def test_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    declared = set(re.findall(r"\b(hcspmm_[a-z0-9_]+)\s*\(", header))
    L = capi.lib()
    for name in NEW:
        assert name in declared and name in capi.SYMBOLS, name
        assert getattr(L, name) is not None
    assert re.search(r"#define\s+HCSPMM_FP8_E4M3\s+0\b", header)
    assert L.hcspmm_abi_version() == 3  # additions only
    for name in ("quantize_fp8", "forward_fp8", "forward_weighted_fp8", "wide_threshold_fp8"):
        assert callable(getattr(hcspmm, name)), name


def test_existing_entry_points_take_no_fp8_dtype_code():
    """the 8-bit type has its own entry points: dtype 3 stays an error of the typed ones, and of their threshold query"""
    one = ctypes.c_void_p(0x1000)
    L = capi.lib()
    assert L.hcspmm_forward_typed(one, 16, 4, one, 4, 3, one, one, one, one, one, one, ctypes.c_void_p(0), None, 16, 8, 4,
                                  ctypes.c_void_p(0), 0, ctypes.c_void_p(0)) == capi.EINVAL
    assert L.hcspmm_wide_threshold_typed(None, 128, 3) == 2 ** 31 - 1


def _vp(v):
    return ctypes.c_void_p(v if v > 1 else (0x1000 if v else 0))  # never dereferenced: every case fails before HIP is touched


def _fw(Xq=1, x_rows=64, ldx=None, fmt=0, scale=1, values=1, Z=1, ldz=None, rp=1, col=1, bp=1, e2c=1, e2r=1, ht=1, plan=0,
        header=None, N=64, E=100, D=32, ws=0, ws_bytes=0):
    return capi.lib().hcspmm_forward_fp8(_vp(Xq), x_rows, D if ldx is None else ldx, fmt, _vp(scale), _vp(values), _vp(Z),
                                         D if ldz is None else ldz, _vp(rp), _vp(col), _vp(bp), _vp(e2c), _vp(e2r), _vp(ht),
                                         _vp(plan), ctypes.byref(header) if header is not None else None, N, E, D, _vp(ws),
                                         ws_bytes, ctypes.c_void_p(0))


def _q(X=1, rows=64, ldx=None, D=32, fmt=0, scale_in=0, Xq=1, ldq=None, scale_out=1):
    return capi.lib().hcspmm_quantize_fp8(_vp(X), rows, D if ldx is None else ldx, D, fmt, _vp(scale_in), _vp(Xq),
                                          D if ldq is None else ldq, _vp(scale_out), ctypes.c_void_p(0))


FORWARD_ERRORS = [
    dict(Xq=0), dict(Z=0), dict(rp=0), dict(col=0), dict(bp=0), dict(ht=0), dict(e2c=0), dict(e2r=0),  # NULL pointers
    dict(fmt=1), dict(fmt=-1), dict(fmt=2),                     # e5m2 / fnuz / anything but HCSPMM_FP8_E4M3
    dict(D=6), dict(D=16, ldx=18), dict(D=0), dict(D=-4),       # off the 4-column / 4-byte grid
    dict(D=16, ldx=12), dict(D=16, ldz=12),                     # strides shorter than a row
    dict(N=-1), dict(E=-1), dict(x_rows=-1),                    # negative sizes
    dict(Xq=0x1002),                                            # a code base off the dword grid
    dict(plan=1),                                               # a plan without its header
]


@pytest.mark.parametrize("case", FORWARD_ERRORS, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_forward_fp8_argument_checks(case):
    assert _fw(**case) == capi.EINVAL
    assert _fw(values=0, **case) == capi.EINVAL  # the same with either operand missing, and with both (the binary launch)
    assert _fw(scale=0, **case) == capi.EINVAL
    assert _fw(values=0, scale=0, **case) == capi.EINVAL


QUANTIZE_ERRORS = [
    dict(X=0), dict(Xq=0), dict(scale_out=0),                   # NULL pointers (scale_out may be NULL only next to scale_in)
    dict(fmt=1), dict(fmt=-1),
    dict(D=6), dict(D=16, ldq=18), dict(D=0),
    dict(D=16, ldx=12), dict(D=16, ldq=12),
    dict(rows=-1),
    dict(Xq=0x1001),
]


@pytest.mark.parametrize("case", QUANTIZE_ERRORS, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_quantize_fp8_argument_checks(case):
    assert _q(**case) == capi.EINVAL
    if "scale_out" not in case:
        assert _q(scale_in=1, **case) == capi.EINVAL


def test_nothing_to_do_launches_nothing():
    assert _fw(N=0, E=0) == 0
    assert _q(rows=0) == 0


@pytest.fixture(scope="module")
def hub_plan():
    """a plan with split rows (a workspace) on the host: hubs of up to 0.9 N entries"""
    rp, col = graphs.powerlaw_graph(2000, 40000, seed=2, max_degree_frac=0.9)
    N, E = len(rp) - 1, len(col)
    plan = hcspmm.preprocess(torch.from_numpy(col), torch.from_numpy(rp), N, E, (N + 15) // 16, rule=0)[4].numpy()
    return N, E, Header.from_buffer_copy(plan[:Header.WORDS].tobytes())


def test_forward_fp8_checks_the_workspace_and_the_plan(hub_plan):
    N, E, h = hub_plan
    D = 64
    need = capi.lib().hcspmm_workspace_bytes(ctypes.byref(h), D)
    assert need > 0 and h.n_split_rows > 0
    common = dict(plan=1, header=h, N=N, E=E, D=D, x_rows=N)
    assert _fw(ws=1, ws_bytes=need - 4, **common) == capi.EWORKSPACE  # short
    assert _fw(ws=0, ws_bytes=need, **common) == capi.EWORKSPACE      # absent
    assert _fw(ws=1, ws_bytes=need, **dict(common, N=N + 1)) == capi.EPLAN  # the header is another graph's
    assert _fw(ws=1, ws_bytes=need, **dict(common, E=E - 1)) == capi.EPLAN
    assert _fw(ws=1, ws_bytes=need, **dict(common, x_rows=h.num_columns - 1)) == capi.EINVAL  # the plan gathers rows Xq lacks
    assert _fw(ws=1, ws_bytes=need, plan=0, header=h, N=N, E=E, D=D, x_rows=N) == capi.EINVAL  # a header without its plan
    keep = h.magic
    h.magic = 0
    assert _fw(ws=1, ws_bytes=need, **common) == capi.EPLAN
    h.magic = keep


def test_wide_threshold_fp8(hub_plan):
    N, E, h = hub_plan
    L = capi.lib()
    assert L.hcspmm_wide_threshold_fp8(None, 128) == 64          # plan-free: the fixed threshold
    assert L.hcspmm_wide_threshold_fp8(None, 520) == 2 ** 31 - 1  # one lane group per wave: no wide rows
    for D in (0, -4, 6, 130):
        assert L.hcspmm_wide_threshold_fp8(ctypes.byref(h), D) == 2 ** 31 - 1
    for D in (4, 32, 128, 256):
        t = L.hcspmm_wide_threshold_fp8(ctypes.byref(h), D)
        assert t in (16, 32, 64, 128, 256, 2 ** 31 - 1), (D, t)
    assert hcspmm.wide_threshold_fp8(None, 128) == 64
