"""Edge-feature messages without a GPU: the argument errors of hcspmm_forward_edge_messages / hcspmm_edge_messages_grad (all
reported before any device call), the exported names, the compiler's resource report of the two new translation units by
the method of test_register_budget_fp8.py, and the GINEConv parameters."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hc-spmm_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
sys.path.insert(0, PKG)

from hcspmm import capi  # noqa: E402

EINVAL = -1
P = ctypes.c_void_p(4096)  # a non-null pointer nobody dereferences: every case below fails before any device call
MUL, ADD_RELU, COPY = 0, 1, 2


def _forward(X=P, x_rows=10, ldx=8, F=P, f_rows=20, ldf=8, index=None, op=ADD_RELU, Z=P, ldz=8, N=10, E=20, D=8, rowptr=P, col=P):
    return capi.lib().hcspmm_forward_edge_messages(X, x_rows, ldx, F, f_rows, ldf, index, op, Z, ldz, rowptr, col, P, P, P, P, None,
                                                   None, N, E, D, None, 0, None)


def _grad(gZ=P, ldg=8, X=P, x_rows=10, ldx=8, F=P, ldf=8, gF=P, ldgf=8, op=ADD_RELU, rowptr=P, col=P, N=10, E=20, D=8):
    return capi.lib().hcspmm_edge_messages_grad(gZ, ldg, X, x_rows, ldx, F, ldf, gF, ldgf, op, rowptr, col, N, E, D, None)


def test_forward_argument_errors_are_einval():
    assert _forward(op=3) == EINVAL and _forward(op=-1) == EINVAL  # a bad op
    assert _forward(F=None) == EINVAL  # NULL F with E > 0
    assert _forward(X=None, op=MUL) == EINVAL and _forward(X=None, op=ADD_RELU) == EINVAL  # NULL X for the ops that read it
    assert _forward(ldx=7) == EINVAL and _forward(ldf=7) == EINVAL and _forward(ldz=7) == EINVAL  # short strides
    assert _forward(f_rows=19) == EINVAL  # f_rows < E without an index
    assert _forward(f_rows=0, index=P) == EINVAL and _forward(f_rows=0) == EINVAL  # f_rows == 0 with E > 0
    assert _forward(f_rows=-1, index=P) == EINVAL
    # alongside those of hcspmm_forward_weighted
    assert _forward(D=0) == EINVAL and _forward(N=-1) == EINVAL and _forward(E=-1) == EINVAL
    assert _forward(Z=None) == EINVAL and _forward(rowptr=None) == EINVAL and _forward(col=None) == EINVAL
    L = capi.lib()
    assert L.hcspmm_forward_edge_messages(P, 10, 8, P, 20, 8, None, ADD_RELU, P, 8, P, P, P, P, P, P, P, None, 10, 20, 8, None, 0,
                                          None) == EINVAL  # a plan without its header
    assert L.hcspmm_forward_edge_messages(P, 10, 8, P, 20, 8, None, ADD_RELU, P, 8, P, P, None, P, P, P, None, None, 10, 20, 8, None,
                                          0, None) == EINVAL  # plan-free without blockPartition
    # what is NOT an error: N = 0 returns at once (copy without X and a short ldx included)
    assert _forward(N=0, E=0, F=None, f_rows=0) == 0
    assert _forward(N=0, E=0, F=None, f_rows=0, X=None, ldx=0, op=COPY) == 0


def test_grad_argument_errors_are_einval():
    assert _grad(op=3) == EINVAL
    assert _grad(gZ=None) == EINVAL and _grad(gF=None) == EINVAL and _grad(col=None) == EINVAL and _grad(rowptr=None) == EINVAL
    assert _grad(X=None, op=MUL) == EINVAL and _grad(X=None, op=ADD_RELU) == EINVAL and _grad(F=None, op=ADD_RELU) == EINVAL
    assert _grad(ldg=7) == EINVAL and _grad(ldgf=7) == EINVAL and _grad(ldx=7) == EINVAL and _grad(ldf=7) == EINVAL
    assert _grad(D=0) == EINVAL and _grad(N=-1) == EINVAL and _grad(E=-1) == EINVAL and _grad(N=0) == EINVAL
    # the operands an op does not read may be NULL, their strides anything; E = 0 launches nothing
    assert _grad(E=0, gZ=None, gF=None, col=None) == 0
    assert _grad(E=0, X=None, F=None, ldx=0, ldf=0, op=COPY) == 0


def test_symbols_constants_and_abi_version():
    lib = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "hcspmm.h")).read()
    for name in ("hcspmm_forward_edge_messages", "hcspmm_edge_messages_grad"):
        assert getattr(lib, name) is not None
        assert name in capi.SYMBOLS and re.search(r"\b%s\(" % name, header), name
    assert capi.lib().hcspmm_abi_version() == 3  # additions only
    assert re.search(r"#define HCSPMM_ABI_VERSION 3\b", header)
    import hcspmm
    assert "forward_edge_messages" in hcspmm.__all__ and "edge_messages_grad" in hcspmm.__all__
    for name, code in hcspmm.EDGE_OPS.items():
        m = re.search(r"#define HCSPMM_EDGE_OP_%s (\d+)" % name.upper(), header)
        assert m and int(m.group(1)) == code, name
    assert sorted(hcspmm.EDGE_OPS.values()) == [0, 1, 2]


# ------------------------------------------------------------------------------------------- resource report
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


UNITS = ("spmm_edge_messages.hip", "edge_messages_grad.hip", "spmm_extremum.hip")


@pytest.fixture(scope="module")
def usage():
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(3) as ex:
        return dict(zip(UNITS, ex.map(_resource_usage, UNITS)))


def _ints_of(name, kernel):
    """kernel<...integer template arguments...> -> their tuple, from the mangled name"""
    m = re.search(r"\d+%sI((?:L[ib]\d+E)+)E" % kernel, name)
    return tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1))) if m else None


BUILDS = {(L, 4) for L in (4, 8, 16, 32, 64)} | {(4, 2), (4, 1)}  # (lanes per task, elements per lane)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_forward_builds_spill_nothing_and_keep_the_extremum_occupancy(usage):
    u, x = usage["spmm_edge_messages.hip"], usage["spmm_extremum.hip"]
    for n, v in u.items():
        assert v["scratch"] == 0, (n, v)
    # the corresponding extremum builds: same lanes per task and vector width, forward and backward; the bar is the better of the two
    for mine, theirs in (("edge_messages_plan_kernel", "extremum_plan_kernel"), ("edge_messages_window_kernel", "extremum_window_kernel")):
        bar = {}
        for n, v in x.items():
            a = _ints_of(n, theirs)
            if a:
                bar[a[:2]] = max(bar.get(a[:2], 0), v["occupancy"])
        assert set(bar) == BUILDS, sorted(bar)
        seen = set()
        for n, v in u.items():
            a = _ints_of(n, mine)
            if a:
                op, lv = a[0], a[1:3]
                seen.add((op, lv))
                print(mine, "op", op, "L, VEC", lv, v, "extremum occupancy", bar[lv])
                assert v["occupancy"] >= bar[lv], (n, v, bar[lv])
        assert seen == {(op, lv) for op in (0, 1, 2) for lv in BUILDS}, sorted(seen)
    fixups = {n: v for n, v in u.items() if _ints_of(n, "edge_messages_fixup_kernel")}
    assert len(fixups) == 3
    xfix = min(v["occupancy"] for n, v in x.items() if re.search(r"\d+fixup_kernel", n))  # the binary pass the backward there uses
    for n, v in fixups.items():
        assert v["occupancy"] >= xfix, (n, v)
    # the unit contains only the new kernels
    assert len(u) == 2 * 3 * len(BUILDS) + 3, sorted(u)
    for n in u:
        assert re.search(r"edge_messages_(plan|window|fixup)_kernel", n), n


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_gradient_builds_spill_nothing(usage):
    u = usage["edge_messages_grad.hip"]
    builds = {_ints_of(n, "edge_messages_grad_kernel") for n in u}
    lv = {(L, 4) for L in (1, 2, 4, 8, 16, 32, 64)} | {(1, 2), (2, 2), (1, 1)}
    assert builds == {(op,) + a for op in (0, 1, 2) for a in lv}, sorted(u)  # only the new kernel
    for n, v in u.items():
        assert v["scratch"] == 0 and v["occupancy"] >= 4, (n, v)


def test_new_builds_stay_out_of_the_pinned_units():
    """the register-budget and kernel-count tests pin the instantiations of the existing units"""
    for unit in os.listdir(CSRC):
        if unit.endswith((".hip", "_impl.h")) and unit not in ("spmm_edge_messages.hip", "edge_messages_grad.hip", "capi.hip"):
            text = open(os.path.join(CSRC, unit)).read()
            assert "EdgeMsg" not in text and "edge_messages" not in text, unit


# ------------------------------------------------------------------------------------------- layer
def test_gineconv_parameters_and_reset():
    import torch
    if os.path.join(PKG, "hybrid_kernel") not in sys.path:
        sys.path.insert(0, os.path.join(PKG, "hybrid_kernel"))  # GNN_model imports the extension; nothing is launched here
    import GNN_model
    conv = GNN_model.GINEConv(24, 16, 5, eps=0.5)
    assert conv.weights.shape == (24, 16) and conv.weights_edge.shape == (5, 24)
    assert {n for n, _ in conv.named_parameters()} == {"weights", "weights_edge"}
    assert float(conv.eps) == 0.5 and not conv.eps.requires_grad and "eps" in dict(conv.named_buffers())
    assert conv.weights.abs().max() <= 1 / 4 and conv.weights_edge.abs().max() <= 1 / 24 ** 0.5
    trained = GNN_model.GINEConv(24, 16, 5, eps=0.5, train_eps=True, fixed=1, directed=True)
    assert {n for n, _ in trained.named_parameters()} == {"weights", "weights_edge", "eps"} and trained.eps.requires_grad
    assert trained.fixed == 1 and trained.directed
    with torch.no_grad():
        trained.eps.fill_(3.0)
        trained.weights.fill_(9.0)
    trained.reset_parameters()
    assert float(trained.eps.detach()) == 0.5 and trained.weights.abs().max() <= 1 / 4
    with pytest.raises(ValueError, match="edge_attr"):
        conv(torch.zeros(4, 24), *([None] * 8), None, None)


def test_driver_gine_flags():
    import importlib.util
    for p in (PKG, os.path.join(PKG, "hybrid_kernel")):
        if p not in sys.path:
            sys.path.insert(0, p)
    spec = importlib.util.spec_from_file_location("hc_spmm_main_gine_cpu", os.path.join(PKG, "HC-SpMM_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(["--model", "gine", "--edge-dim", "5", "--directed"])
    assert args.model == "gine" and args.edge_dim == 5 and args.directed
    assert mod.parse_args(["--model", "gine"]).edge_dim == 8
    for bad in (["--edge-dim", "0"], ["--norm", "sym"], ["--fp8"]):
        with pytest.raises(SystemExit):
            mod.parse_args(["--model", "gine"] + bad)
