"""The 16-bit GATv2 attention without a GPU: the two typed symbols, their argument checks before they touch HIP, the resource report
of gatv2_attention16.hip (cross-compiled for gfx950 with the build's flags), and GATv2Conv's activation_dtype surface."""
import ctypes
import os
import re

import pytest
import torch

from hcspmm import capi
from test_edge16_cpu import _resource_report
from test_gated_cpu import HIPCC, ROOT, _pkg_imports, _vp

F16, BF16 = 1, 2
FWD, BWD = "hcspmm_gatv2_scores_typed", "hcspmm_gatv2_scores_backward_typed"


def _fwd(dtype=BF16, hd=0x1000, hs=0x2000, att=1, out=1, rp=1, col=1, N=64, E=100, D=32, heads=4, src_rows=64, ld_dst=None, ld_src=None,
         slope=0.2):
    return getattr(capi.lib(), FWD)(ctypes.c_void_p(hd), ld_dst or D, ctypes.c_void_p(hs), src_rows, ld_src or D, dtype, _vp(att), slope,
                                    _vp(out), _vp(rp), _vp(col), N, E, D, heads, ctypes.c_void_p(0))


def _bwd(dtype=BF16, grad_dtype=None, g=1, hd=0x1000, hs=0x2000, att=1, rp=1, col=1, rp_t=1, col_t=1, perm=1, gd=0x3000, gs=0x4000, ga=1,
         ws=1, ws_bytes=1 << 30, N=64, E=100, D=32, heads=4, ld_dst=None, ld_src=None, ld_gdst=None, ld_gsrc=None, slope=0.2):
    return getattr(capi.lib(), BWD)(_vp(g), ctypes.c_void_p(hd), ld_dst or D, ctypes.c_void_p(hs), ld_src or D, dtype, _vp(att), slope,
                                    _vp(rp), _vp(col), _vp(rp_t), _vp(col_t), _vp(perm), N, N, E, D, heads, ctypes.c_void_p(gd),
                                    ld_gdst or D, ctypes.c_void_p(gs), ld_gsrc or D, dtype if grad_dtype is None else grad_dtype, _vp(ga),
                                    _vp(ws), ws_bytes, ctypes.c_void_p(0))


# both calls: odd strides, bases off the dword grid, Dh % 4 != 0, D > 512 (256 at Dh % 8 != 0), and the fp32 calls' own refusals
SHARED = (dict(ld_dst=33), dict(ld_src=35), dict(hd=0x1002), dict(hs=0x2002), dict(D=24, heads=4), dict(D=520, heads=1),
          dict(D=264, heads=22), dict(heads=0), dict(heads=5), dict(ld_dst=16), dict(att=0), dict(rp=0), dict(col=0), dict(hd=0),
          dict(slope=float("nan")), dict(slope=float("inf")))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("call,case", [(_fwd, c) for c in SHARED + (dict(out=0), dict(src_rows=0), dict(N=-1))]
                         + [(_bwd, c) for c in SHARED + (dict(ld_gdst=33), dict(ld_gsrc=35), dict(gd=0x3002), dict(gs=0x4002), dict(g=0),
                                                         dict(grad_dtype=3), dict(perm=0), dict(rp_t=0), dict(col_t=0), dict(ga=0),
                                                         dict(ws=0), dict(ld_gdst=16))])
def test_sixteen_bit_refusals_come_before_hip(dtype, call, case):
    assert call(dtype, **case) == capi.EINVAL


def test_symbols_forwarding_workspace_and_nothing_to_do():
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    assert re.search(r"#define HCSPMM_ABI_VERSION 3\b", header) and capi.lib().hcspmm_abi_version() == 3
    for name, n_args in ((FWD, 16), (BWD, 27)):  # declared, listed, exported
        assert re.search(r"\bint %s\(" % name, header) and len(capi.SYMBOLS[name][1]) == n_args and getattr(capi.lib(), name)
    assert _bwd(BF16, grad_dtype=F16) == capi.EINVAL and _bwd(F16, grad_dtype=BF16) == capi.EINVAL and _bwd(0, grad_dtype=BF16) == capi.EINVAL
    # fp32 forwards: the fp32 calls' codes for the same defects; odd strides are none there
    for call in (_fwd, _bwd):
        assert call(-1) == capi.EINVAL and call(3) == capi.EINVAL  # a foreign dtype
        assert call(0, D=24, heads=4) == capi.EINVAL and call(0, ld_dst=16) == capi.EINVAL and call(0, slope=float("nan")) == capi.EINVAL
    assert _fwd(0, ld_dst=33, E=0) == 0 and _fwd(0, hd=0x1004, D=520, heads=1, E=0) == 0
    assert _bwd(0, ws_bytes=0) == capi.EWORKSPACE and _bwd(0, ld_gdst=33, ws_bytes=0) == capi.EWORKSPACE
    need = capi.lib().hcspmm_gatv2_backward_workspace_bytes(64, 100, 32, 4)
    for dtype in (F16, BF16):
        assert need > 0 and _bwd(dtype, ws_bytes=need - 1) == capi.EWORKSPACE and _bwd(dtype, grad_dtype=0, ws_bytes=0) == capi.EWORKSPACE
        assert _bwd(dtype, grad_dtype=0, ld_gdst=33, ws_bytes=0) == capi.EWORKSPACE  # an fp32 gradient may have an odd stride
    for dtype in (0, F16, BF16):  # nothing to do: no launch
        assert _fwd(dtype, out=0, col=0, E=0) == 0 and _fwd(dtype, hd=0, hs=0, out=0, col=0, N=0, E=0, src_rows=0) == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_kernels_keep_their_budgets():
    """2 types x 7 lane counts x VEC 8 / 4, no scratch: scores at 4 waves per SIMD or more, the gradients at the fp32 unit's (dst 4, src 5)"""
    report = _resource_report("gatv2_attention16")
    seen = set()
    for name, (scratch, occ) in report.items():
        assert scratch == 0, (name, scratch)
        m = re.search(r"gatv2_scores16_kernelINS_(3F16|4BF16)ELi(\d+)ELi(\d+)EE", name)
        g = re.search(r"gatv2_grad16_kernelINS_(3F16|4BF16)ELi([01])ELi(\d+)ELi(\d+)EE", name)
        if m or g:
            kind = "scores" if m else ("dst" if g.group(2) == "0" else "src")
            assert occ >= (5 if kind == "src" else 4), (name, occ)
            seen.add((kind,) + ((m.group(1), int(m.group(2)), int(m.group(3))) if m else (g.group(1), int(g.group(3)), int(g.group(4)))))
    assert seen == {(k, e, L, v) for k in ("scores", "dst", "src") for e in ("3F16", "4BF16") for L in (1, 2, 4, 8, 16, 32, 64)
                    for v in (8, 4)}
    assert len(report) == len(seen) + 1 and any("gatv2_att16_fold_kernel" in n for n in report)


def test_gatv2conv_activation_dtype():
    _pkg_imports()
    import GNN_model
    conv = GNN_model.GATv2Conv(16, 8, heads=4, concat=True, activation_dtype=torch.bfloat16)
    assert conv.activation_dtype is torch.bfloat16 and GNN_model.GATv2Conv(16, 8, heads=4).activation_dtype is None
    assert {n: tuple(p.shape) for n, p in conv.named_parameters()} == {"weights": (16, 64), "att": (4, 8)}
    assert all(p.dtype == torch.float32 for p in conv.parameters()) and GNN_model.GATv2Scores16 and GNN_model.GATv2ScoresDirected16
    GNN_model.GATv2Conv(16, 8, heads=4).load_state_dict(conv.state_dict())
    GNN_model.GATv2Conv(16, 512, heads=1, activation_dtype=torch.float16), GNN_model.GATv2Conv(16, 4, heads=64, activation_dtype=torch.float16)
    for bad in (dict(input_dim=15), dict(activation_dtype=torch.float64), dict(output_dim=8, heads=65), dict(output_dim=12, heads=22)):
        with pytest.raises(ValueError, match="activation_dtype"):
            GNN_model.GATv2Conv(**dict(dict(input_dim=16, output_dim=8, heads=4, activation_dtype=torch.float16), **bad))
    with pytest.raises(ValueError, match="activation_dtype"):
        GNN_model.gatv2_attention(None, None, None, (None, None), activation_dtype=torch.float64)
