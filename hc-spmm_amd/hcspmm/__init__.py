"""hcspmm -- Python host glue over the C ABI of libhcspmm.so (include/hcspmm.h).

Mirrors the operator surface of the reference's `HCSPMM` extension module
(/root/reference/hybrid_kernel/hybrid_all.cpp:500-525): `preprocess`, `forward`,
`forward_more`, `forward_fixed32`, `forward_fixed64`, the fused variants and the `backward*`
aliases, with the same positional arguments and return lists, so code written against the
reference calls it unchanged.  Tensors are plumbing only (device memory + streams); all work
happens behind the C ABI.  There is NO CPU fallback: if libhcspmm.so is missing, or a feature
tensor is not on the GPU, the call raises.
"""
import collections
import ctypes
import os
import threading
import weakref

import torch

from .capi import (EPLAN, Header, PlanParams, RULE_AS_SHIPPED, RULE_INTENDED, RULE_INTENDED_GUARD, RULE_MI355X,
                   RULE_MI355X_WIDE, check, lib)

__all__ = [
    "preprocess", "forward", "forward_more", "forward_fixed32", "forward_fixed64", "forward_fixed32_fused",
    "forward_fixed64_fused", "forward_final_fused", "forward_final_fused_64", "forward_GIN_final_fused", "backward",
    "backward_fixed32", "backward_fixed32_fused", "backward_final_fused", "backward_fixed64",
    "backward_fixed64_fused", "backward_final_fused_64", "backward_GIN_final_fused", "loi_reorder",
    "apply_permutation", "weight_grad", "update", "plan_header", "forward_rect", "forward_into", "sddmm", "edge_softmax", "edge_softmax_backward",
    "gat_attention", "gat_attention_backward", "forward_weighted_heads", "sddmm_heads",
    "gatv2_scores", "gatv2_scores_backward",
    "transpose_graph", "transpose_graph_device", "sample_row_pointers", "sample_neighbors", "plan_free_graph",
    "SAMPLE_WAVE_ROW_MAX", "forward_weighted_indexed", "gat_attention_backward_directed", "gatv2_scores_backward_directed",
    "forward_max", "forward_min", "forward_extremum_backward", "forward_multi",
    "forward_softmax", "softmax_backward", "forward_gated",
    "forward_edge_messages", "edge_messages_grad", "EDGE_OPS",
    "quantize_fp8", "forward_fp8", "forward_weighted_fp8", "wide_threshold_fp8",
    "wide_threshold", "workspace_bytes", "fused_in_launch", "own_tiny_launch", "build_plan", "set_default_rule", "default_rule", "RULE_INTENDED", "RULE_INTENDED_GUARD",
    "RULE_AS_SHIPPED", "RULE_MI355X", "RULE_MI355X_WIDE", "mi355x_rule", "tune_plan",
]

# The window classifier preprocess() uses when the caller names none.  The reference's coefficients (rule 0) were fitted on an
# RTX 3090 and its paper says they hold only "while the GPU architecture ... remain[s] unchanged" (p.7): the default here is the
# refit made on MI355X with the reference's own procedure -- the NARROW one (RULE_MI355X), because preprocess is not told the
# embedding width and that set is never slower than rule 0 at any width (profiles/r04/ab_classifier_rules.log: -1 ... +25 %),
# while the wide set loses up to 15 % below 64 columns.  preprocess(rule="mi355x", dim=D) picks the set for a known width;
# HCSPMM_RULE=0 / set_default_rule(RULE_INTENDED) / rule=0 give the reference's hybrid_type bit for bit.
_DEFAULT_RULE = int(os.environ.get("HCSPMM_RULE", RULE_MI355X))
_PLAN_PARAMS = PlanParams(int(os.environ.get("HCSPMM_SPLIT_THRESHOLD", 0)), int(os.environ.get("HCSPMM_SEGMENT_LEN", 0)),
                          int(os.environ.get("HCSPMM_FUSE_IN_LAUNCH", 0)))


def set_default_rule(rule):
    """Classifier rule used by preprocess(): RULE_MI355X (default: the width-agnostic MI355X refit), RULE_MI355X_WIDE
    (mi355x_rule(D) picks between the two), or the reference's RULE_INTENDED, _GUARD, _AS_SHIPPED."""
    global _DEFAULT_RULE
    _DEFAULT_RULE = int(rule)


def default_rule():
    return _DEFAULT_RULE


def mi355x_rule(embedding_dim):
    """The MI355X refit of the window classifier for this embedding width (hcspmm.h: the boundary between
    the two sub-paths moves with D, and preprocess -- like the reference's -- is not told D)."""
    return RULE_MI355X if int(embedding_dim) < 64 else RULE_MI355X_WIDE


# ---------------------------------------------------------------------------------------------
# plan registry: data_ptr of a plan tensor -> host copy of its header.  The registry does NOT keep the
# tensor alive (a caller that preprocesses many graphs must be able to free their plans): an entry holds a
# weak reference and is valid only while that tensor lives -- while it does, its memory cannot be handed to
# another tensor, so the address is an unambiguous key; a dead entry is dropped and the header re-read (one
# 256-byte device read).  Each entry also remembers which (row_pointers, column_index) tensors the plan has
# been checked against: preprocess / build_plan register the pair the plan was built from; any other pair is
# fingerprinted on the device once (hcspmm_graph_fingerprint_device) and refused unless it matches the header.
# ---------------------------------------------------------------------------------------------
class _Entry:
    __slots__ = ("ref", "header", "graphs", "checked")

    def __init__(self, plan_t, header):
        self.ref = weakref.ref(plan_t)
        self.header = header
        self.graphs = collections.OrderedDict()  # (rowptr ptr, col ptr) -> (weakref, weakref)
        self.checked = None                      # (N, E, numel) hcspmm_plan_check has passed for


_REG = collections.OrderedDict()
_REG_LOCK = threading.Lock()
_REG_MAX = 256
_GRAPHS_MAX = 8


def _purge_locked():
    for k in [k for k, e in _REG.items() if e.ref() is None]:
        del _REG[k]
    while len(_REG) >= _REG_MAX:  # least recently used first
        _REG.popitem(last=False)


def _register(plan_t, header, row_pointers=None, column_index=None):
    e = _Entry(plan_t, header)
    if row_pointers is not None and column_index is not None and row_pointers.is_cuda:
        e.graphs[(row_pointers.data_ptr(), column_index.data_ptr())] = (weakref.ref(row_pointers), weakref.ref(column_index))
    with _REG_LOCK:
        _purge_locked()
        _REG[plan_t.data_ptr()] = e
    return e


def _entry(row_nzr, num_nodes=None, num_edges=None):
    if row_nzr is None or row_nzr.numel() < Header.WORDS or row_nzr.dtype != torch.int32:
        return None
    key = row_nzr.data_ptr()
    with _REG_LOCK:
        e = _REG.get(key)
        if e is not None:
            if e.ref() is not None:
                _REG.move_to_end(key)
                return e
            del _REG[key]
    host = row_nzr[:Header.WORDS].cpu().contiguous()
    h = Header.from_buffer_copy(host.numpy().tobytes())
    if h.magic != Header.MAGIC:
        return None
    if num_nodes is not None and check(lib().hcspmm_plan_check(ctypes.byref(h), num_nodes, num_edges, row_nzr.numel()),
                                       soft=True) != 0:
        return None
    return _register(row_nzr, h)


def plan_header(row_nzr, num_nodes=None, num_edges=None):
    """Host copy of the plan header carried by `row_nzr`, or None for the reference's [0]
    placeholder.  A plan tensor first seen here (e.g. a clone) costs one small device read."""
    e = _entry(row_nzr, num_nodes, num_edges)
    return e.header if e is not None else None


def _verify_graph(e, row_pointers, column_index):
    """The plan of entry `e` was built for ONE graph; N and E alone do not identify it (a LOI reorder keeps both)."""
    key = (row_pointers.data_ptr(), column_index.data_ptr())
    hit = e.graphs.get(key)
    if hit is not None and hit[0]() is not None and hit[1]() is not None:
        return
    L = lib()
    out = torch.empty(1, dtype=torch.int64, device=row_pointers.device)
    stream = torch.cuda.current_stream(row_pointers.device)
    with torch.cuda.device(row_pointers.device):
        check(L.hcspmm_graph_fingerprint_device(_ptr(row_pointers), _ptr(column_index), row_pointers.numel() - 1,
                                                column_index.numel(), _ptr(out), ctypes.c_void_p(stream.cuda_stream)))
    got = int(out.item()) & 0xFFFFFFFFFFFFFFFF
    if got != e.header.fingerprint:
        raise RuntimeError("hcspmm: plan does not match this graph (row_pointers / column_index differ from the ones "
                           "the plan was built from) [code %d]" % EPLAN)
    while len(e.graphs) >= _GRAPHS_MAX:
        e.graphs.popitem(last=False)
    e.graphs[key] = (weakref.ref(row_pointers), weakref.ref(column_index))


def wide_threshold(row_nzr, embedding_dim, dtype=torch.float32):
    """Rows of the sparse path with more entries than this are summed by a whole wave (shuffle-tree
    combine) instead of one lane group in CSR order; see hcspmm_wide_threshold in include/hcspmm.h."""
    h = plan_header(row_nzr)
    return int(lib().hcspmm_wide_threshold_typed(ctypes.byref(h) if h is not None else None, int(embedding_dim),
                                                 _DTYPES[dtype]))


def wide_threshold_fp8(row_nzr, embedding_dim):
    """wide_threshold for forward_fp8 / forward_weighted_fp8 (hcspmm_wide_threshold_fp8, include/hcspmm.h)."""
    h = plan_header(row_nzr)
    return int(lib().hcspmm_wide_threshold_fp8(ctypes.byref(h) if h is not None else None, int(embedding_dim)))


def workspace_bytes(row_nzr, embedding_dim):
    """Bytes of fp32 workspace a forward with this plan and width needs (partial sums of split rows); 0 without a plan."""
    h = plan_header(row_nzr)
    return int(lib().hcspmm_workspace_bytes(ctypes.byref(h), int(embedding_dim))) if h is not None else 0


def fused_in_launch(row_nzr, embedding_dim, hidden_dim):
    """Form forward_*_fused takes with this plan and shape (hcspmm_fused_in_launch, include/hcspmm.h): 0 = two launches,
    1 = dense-tile windows update inside the hybrid launch, 2 = the sparse-row path as well (row-tile form)."""
    h = plan_header(row_nzr)
    return int(lib().hcspmm_fused_in_launch(ctypes.byref(h), int(embedding_dim), int(hidden_dim))) if h is not None else 0


def own_tiny_launch(row_nzr, fused=False):
    """True when the tiny tasks of this plan run as a launch of their own (tiny_kernel, tiny_w_kernel, tiny_wh_kernel) rather
    than as a region of the hybrid launch (hcspmm_own_tiny_launch, include/hcspmm.h); fused: ask about forward_*_fused."""
    h = plan_header(row_nzr)
    return bool(lib().hcspmm_own_tiny_launch(ctypes.byref(h), int(bool(fused)))) if h is not None else False


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else 0)


class _on_device:
    """`with torch.cuda.device(d)` only when d is not already current (the context manager costs a few microseconds,
    which is the whole kernel time on a Cora-scale graph)."""
    __slots__ = ("ctx",)

    def __init__(self, device):
        self.ctx = None if device.index is None or device.index == torch.cuda.current_device() else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _i32_host(t):
    t = t.detach()
    if t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() > (1 << 16):
        # large device arrays come back through a pinned buffer: a pageable D2H copy runs at ~1.4 GB/s
        # (first-touch page faults inside the copy), a pinned one at PCIe rate
        host = torch.empty(t.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(t, non_blocking=True)
        torch.cuda.current_stream(t.device).synchronize()
        return host
    return t.to(device="cpu", dtype=torch.int32).contiguous()


def preprocess(column_index, row_pointers, num_nodes, num_edges, num_row_windows, rule=None, dim=None, num_columns=None):
    """HCSPMM.preprocess (hybrid_all.cpp:13-17,501; hybrid_all_kernel.cu:339-408).

    Argument order as the reference: column_index FIRST (HC-SpMM_main.py:52).  `num_edges` is
    ignored in favour of column_index.size(0).  Runs on the host (north_star),
    returns [blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr] on the device
    of `column_index`; `row_nzr` carries the MI355X launch plan, `col_nzr` stays the [0] placeholder.
    `rule` (not in the reference): a HCSPMM_RULE_* number, or "mi355x" together with `dim` = the embedding
    width the graph will be multiplied at (picks the narrow or the wide MI355X refit).
    `num_columns` (not in the reference, whose graphs are square): rows of the matrix the column ids index, for
    a row block of a sharded graph.  Column ids outside [0, num_columns) raise -- on the GPU they would be
    out-of-bounds gathers.
    """
    L = lib()
    dev = column_index.device
    col_h = _i32_host(column_index)
    rp_h = _i32_host(row_pointers)
    N = int(rp_h.numel()) - 1
    E = int(col_h.numel())
    if int(num_nodes) != N:
        raise RuntimeError("preprocess: num_nodes (%d) != row_pointers.size(0)-1 (%d)" % (num_nodes, N))
    W = (N + 15) // 16
    if int(num_row_windows) != W:
        raise RuntimeError("preprocess: num_row_windows (%d) != ceil(N/16) (%d)" % (num_row_windows, W))
    on_gpu = dev.type == "cuda"
    # host outputs in pinned memory when they are headed for the GPU (torch's caching host allocator recycles the blocks
    # from call to call): the uploads run at PCIe rate and asynchronously instead of through a pageable staging copy
    bp = torch.empty(W, dtype=torch.int32, pin_memory=on_gpu)
    ht = torch.empty(W, dtype=torch.int32, pin_memory=on_gpu)
    e2c = torch.empty(E, dtype=torch.int32, pin_memory=on_gpu)
    # edgeToRow is the plain CSR row expansion: made on the device when the graph lives there -- fill_edgeToRow
    # (K.cu:314-337) as one small HIP kernel of the library, enqueued now so that it runs under the host passes below
    e2r = None
    if on_gpu:
        e2r = torch.empty(E, dtype=torch.int32, device=dev)
        rp_dev = row_pointers.to(device=dev, dtype=torch.int32).contiguous()  # (no copy when it already is)
        with torch.cuda.device(dev):
            check(L.hcspmm_edge_to_row_device(_ptr(rp_dev), N, E, _ptr(e2r),
                                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    e2r_h = None if on_gpu else torch.empty(E, dtype=torch.int32)
    if rule == "mi355x":
        if dim is None:
            raise RuntimeError('preprocess: rule="mi355x" needs dim= (the embedding width)')
        rule = mi355x_rule(dim)
    r = _DEFAULT_RULE if rule is None else int(rule)
    M = N if num_columns is None else int(num_columns)
    check(L.hcspmm_preprocess_host(_ptr(rp_h), _ptr(col_h), N, E, M, r, 0, _ptr(bp), _ptr(e2c), _ptr(e2r_h), _ptr(ht)))
    if not on_gpu:
        e2r = e2r_h
    # the window products go up while the host builds the plan from them (pinned memory: asynchronous PCIe-rate copies)
    up = [t.to(dev, non_blocking=True) for t in (bp, e2c, e2r, ht)]  # .to() is a no-op for the device-made e2r
    words = ctypes.c_int64(0)
    check(L.hcspmm_plan_words(_ptr(rp_h), N, E, _ptr(bp), _ptr(ht), ctypes.byref(_PLAN_PARAMS), ctypes.byref(words)))
    plan = torch.empty(max(int(words.value), Header.WORDS), dtype=torch.int32, pin_memory=on_gpu)
    check(L.hcspmm_plan_build(_ptr(rp_h), _ptr(col_h), N, E, M, _ptr(bp), _ptr(e2c), _ptr(ht),
                              ctypes.byref(_PLAN_PARAMS), _ptr(plan), plan.numel()))
    h = Header.from_buffer_copy(plan[:Header.WORDS].numpy().tobytes())
    plan = plan[:h.total_words]  # hcspmm_plan_words sizes for the larger of the two layouts (column slices or none)
    outs = up + [plan.to(dev, non_blocking=True)]
    _register(outs[4], h, row_pointers, column_index)
    col_nzr = torch.zeros(1, dtype=torch.int32, device=dev)
    return [outs[0], outs[1], outs[2], outs[3], outs[4], col_nzr]


def build_plan(row_pointers, column_index, blockPartition, edgeToColumn, hybrid_type, device=None,
               split_threshold=0, segment_len=0, num_columns=None, fuse_in_launch=False, slice_threshold=0, n_slices=0,
               panel_cols=0):
    """Launch plan for an arbitrary window classification (e.g. every window forced onto one sub-path,
    or a classifier of the caller's own): -> plan tensor to pass as `row_nzr`.  fuse_in_launch: 1 (or True) = the fused
    operators update this plan's dense-tile windows inside the hybrid launch, 2 = the sparse-row path as well (row-tile
    form; include/hcspmm.h hcspmm_forward_fused).
    slice_threshold / n_slices: XCD-affine column slices (hcspmm_plan_params; 0 = automatic, < 0 = off).
    panel_cols: feature columns per pass of the sparse-row path (0 = chosen at launch, < 0 = one pass; see tune_plan)."""
    L = lib()
    rp_h, col_h = _i32_host(row_pointers), _i32_host(column_index)
    bp_h, e2c_h, ht_h = _i32_host(blockPartition), _i32_host(edgeToColumn), _i32_host(hybrid_type)
    N, E = rp_h.numel() - 1, col_h.numel()
    params = PlanParams(int(split_threshold), int(segment_len), int(fuse_in_launch), int(slice_threshold), int(n_slices),
                        int(panel_cols)) \
        if (split_threshold or segment_len or fuse_in_launch or slice_threshold or n_slices or panel_cols) else _PLAN_PARAMS
    words = ctypes.c_int64(0)
    check(L.hcspmm_plan_words(_ptr(rp_h), N, E, _ptr(bp_h), _ptr(ht_h), ctypes.byref(params), ctypes.byref(words)))
    plan = torch.empty(max(int(words.value), Header.WORDS), dtype=torch.int32)
    check(L.hcspmm_plan_build(_ptr(rp_h), _ptr(col_h), N, E, N if num_columns is None else int(num_columns), _ptr(bp_h),
                              _ptr(e2c_h), _ptr(ht_h), ctypes.byref(params), _ptr(plan), plan.numel()))
    h = Header.from_buffer_copy(plan[:Header.WORDS].numpy().tobytes())
    plan = plan[:h.total_words]
    dev = torch.device(device) if device is not None else row_pointers.device
    plan_d = plan.to(dev)
    _register(plan_d, h, row_pointers, column_index)
    return plan_d


def tune_plan(row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, embedding_dim,
              dtype=torch.float32, num_columns=None, candidates=None, steps=20, fuse_in_launch=False):
    """Measure, on this GPU and THIS graph, the plan variants whose best choice no size rule predicts -- column slices on /
    off and the panel width of the sparse-row path -- and return (best plan tensor, report).  The automatic choices are tuned
    on power-law graphs from 10 K to 16 M nodes; between them (e.g. 66 K-130 K nodes) another panel width can be 5-17 %
    faster (profiles/r03/ab_panel_midsize.log, ab_slices_midsize.log).  Costs a handful of plan builds and
    len(candidates) * (3 + steps) launches: worth it for a graph that will be multiplied thousands of times (training).
    candidates: list of dicts of build_plan keywords (slice_threshold, n_slices, panel_cols, ...); default = slices
    {automatic, off, 256 x 8} x panels {automatic, 32, 64, one pass} (panels only for embedding_dim >= 64).  The results of
    all variants agree within the 1e-5 bar; rows short enough to be summed in CSR order by every variant agree bit for bit."""
    dev = row_pointers.device
    if not row_pointers.is_cuda:
        raise RuntimeError("tune_plan measures on the GPU: graph tensors must be CUDA tensors")
    D = int(embedding_dim)
    N = row_pointers.size(0) - 1
    M = N if num_columns is None else int(num_columns)
    if candidates is None:
        panels = [0, 32, 64, -1] if D >= 64 else [0]  # (fp32 columns: 16-bit features take twice as many per pass)
        candidates = [dict(slice_threshold=s, panel_cols=p) for s in (0, -1, 256) for p in panels]
    X = torch.randn(M, D, device=dev).to(dtype)
    Z = torch.empty(N, D, dtype=dtype, device=dev)
    col_nzr = torch.zeros(1, dtype=torch.int32, device=dev)
    report, best, seen = [], None, set()
    for kw in candidates:
        plan = build_plan(row_pointers, column_index, blockPartition, edgeToColumn, hybrid_type, num_columns=M,
                          fuse_in_launch=fuse_in_launch, **kw)
        h = plan_header(plan)
        key = (h.n_slices, h.slice_threshold, h.panel_cols, h.n_slice_tasks)
        if key in seen:  # e.g. "slices off" on a graph the automatic rule leaves unsliced anyway
            continue
        seen.add(key)
        ws = torch.empty(max(workspace_bytes(plan, D) // 4, 1), dtype=torch.float32, device=dev)
        a = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, plan, col_nzr)
        for _ in range(3):
            forward_into(X, Z, *a, workspace=ws)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(steps):
            forward_into(X, Z, *a, workspace=ws)
        e.record()
        e.synchronize()
        ms = s.elapsed_time(e) / steps
        report.append(dict(kw, ms=ms, n_slices=h.n_slices))
        if best is None or ms < best[0]:
            best = (ms, plan)
    return best[1], sorted(report, key=lambda r: r["ms"])


def _check_input(t, name):
    # hybrid_all.cpp:185-187 CHECK_CUDA / CHECK_CONTIGUOUS, same messages
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


# feature element types of hcspmm_forward_typed (include/hcspmm.h HCSPMM_DTYPE_*)
_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


_GRAPH_NAMES = ("nodePointer", "edgeList", "blockPartition", "edgeToColumn", "edgeToRow")


def _check_graph(*arrays, input_error=None):
    """CHECK_INPUT of the graph arrays in the reference's order -- (row_pointers, column_index) or all five -- then the int32
    contract of the CSR pair: the kernels read both as int32, so any other dtype would be an out-of-bounds read.
    input_error: the message of a contiguous input that fails its dtype contract, which the extension reports between the
    two (None: the input is sound, or the entry point checks it elsewhere)."""
    for t, n in zip(arrays, _GRAPH_NAMES):
        _check_input(t, n)
    if input_error is not None:
        raise RuntimeError(input_error)
    if arrays[0].dtype != torch.int32 or arrays[1].dtype != torch.int32:
        raise RuntimeError("nodePointer / edgeList must be int32")


def _graph_args(X, graph, row_nzr, rect=False, dtypes=(torch.float32,)):
    """The checks of an entry point that gathers the rows of a contiguous X -> its _planned_call"""
    _check_input(X, "input")
    _check_graph(*graph[:5], input_error=None if X.dtype in dtypes and X.dim() == 2 else
                 "input must be a 2-D %s tensor" % " / ".join(str(d).replace("torch.", "") for d in dtypes))
    N = graph[0].size(0) - 1
    if X.size(0) != N and not rect:
        raise RuntimeError("input has %d rows but the graph has %d nodes" % (X.size(0), N))
    return _planned_call(graph, row_nzr, X.size(1), X.size(0), X.device)


def _checked_header(row_nzr, row_pointers, column_index, N, E, x_rows):
    """Header of the plan in `row_nzr` (None: the reference's placeholder -> plan-free kernel), after checking
    that the plan belongs to THIS graph and that X has every row the plan gathers."""
    e = _entry(row_nzr, N, E) if (row_nzr is not None and row_nzr.is_cuda) else None
    if e is None:
        return None
    if e.checked != (N, E, row_nzr.numel()):
        check(lib().hcspmm_plan_check(ctypes.byref(e.header), N, E, row_nzr.numel()))
        e.checked = (N, E, row_nzr.numel())
    if x_rows < e.header.num_columns:
        raise RuntimeError("input has %d rows but the plan gathers from %d" % (x_rows, e.header.num_columns))
    _verify_graph(e, row_pointers, column_index)
    return e.header


def _ws_bytes(h, D):
    return int(lib().hcspmm_workspace_bytes(ctypes.byref(h), D))


def _ws_bytes_extremum(h, D):
    return int(lib().hcspmm_extremum_workspace_bytes(ctypes.byref(h), D))


class _planned_call(_on_device):
    """One launch on a graph with or without a plan.  `graph`: the tensors whose pointers open the C ABI's graph arguments -- the
    six of the SpMM entry points, or (row_pointers, column_index) for the SDDMM.  Runs _checked_header (the plan in `row_nzr`
    belongs to this graph, and the gathered operand has src_rows >= the rows the plan gathers), then takes the caller's
    `workspace` if it is large enough or allocates what ws_fn(header, D) -- _ws_bytes, _ws_bytes_extremum; None for an entry
    point without a workspace -- asks for.  Supplies, spelled here and nowhere else:
      graph  the run (graph pointers..., plan, header, N, E, D) of every planned entry point
      ws     the run (workspace, workspace_bytes, stream) that closes it
    and is the call's _on_device context.  Flat on purpose (slots, no closures): the kernel of a Cora-scale call is shorter
    than this constructor."""
    __slots__ = ("N", "E", "D", "graph", "ws", "stream", "buf")

    def __init__(self, graph, row_nzr, D, src_rows, device, workspace=None, ws_fn=_ws_bytes):
        _on_device.__init__(self, device)
        self.N, self.E, self.D = N, E, D = graph[0].size(0) - 1, graph[1].size(0), D
        h = _checked_header(row_nzr, graph[0], graph[1], N, E, src_rows)
        buf, ws_bytes = None, 0
        if h is not None and ws_fn is not None:
            ws_bytes = ws_fn(h, D)
            if ws_bytes:
                if workspace is not None and workspace.numel() * workspace.element_size() >= ws_bytes:
                    buf = workspace  # a caller-kept buffer: nothing is allocated in the step (hcspmm.sharded)
                else:
                    buf = torch.empty(ws_bytes // 4, dtype=torch.float32, device=device)
        self.buf = buf  # (alive until the launch is enqueued)
        self.stream = stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        if h is not None:
            self.graph = (*map(_ptr, graph), _ptr(row_nzr), ctypes.byref(h), N, E, D)
        else:
            self.graph = (*map(_ptr, graph), ctypes.c_void_p(0), None, N, E, D)
        self.ws = (_ptr(buf), ws_bytes, stream)


def _spmm(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
          Z=None, rect=False):
    c = _graph_args(X, (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type),
                       row_nzr, rect, dtypes=tuple(_DTYPES))
    D = c.D
    if Z is None:
        Z = torch.empty((c.N, D), dtype=X.dtype, device=X.device)
    with c:
        check(lib().hcspmm_forward_typed(_ptr(X), X.size(0), D, _ptr(Z), D, _DTYPES[X.dtype], *c.graph, *c.ws))
    return Z


def forward(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr):
    """HCSPMM.forward -> [A*X]  (hybrid_all.cpp:194-221; any embedding_dim).  X may also be float16 / bfloat16
    (the paper's half-precision variants, Table VII): rows are gathered as stored, summed in fp32 in the fp32
    path's order and rounded once -- Z has X's dtype."""
    return [_spmm(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr)]


def forward_rect(X_full, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                 col_nzr):
    """Row-block form used by the multi-GPU shard (hcspmm.sharded): A is n_local x M with column ids
    indexing the rows of X_full (M x D, the all-gathered embedding matrix) -> [Z_local (n_local x D)]."""
    return [_spmm(X_full, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                  col_nzr, rect=True)]


def forward_into(X, Z, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                 col_nzr, workspace=None):
    """Strided form: Z[:, :] = A @ X where X and Z may be column slices of wider matrices (unit inner
    stride, any row stride) and X may have any number of rows (column ids index them).  Used by the
    multi-GPU shard to multiply one gathered column panel at a time straight into its slice of Z.
    `workspace`: optional caller-kept fp32 buffer of at least workspace_bytes(row_nzr, D) bytes."""
    _check_graph(row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
    for t, n in ((X, "input"), (Z, "output")):
        if not t.is_cuda:
            raise RuntimeError("%s must be a CUDA tensor" % n)
        if t.dtype not in _DTYPES or t.dtype != X.dtype or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.size(1):
            raise RuntimeError("%s must be a 2-D float32 / float16 / bfloat16 view with unit inner stride" % n)
    N, D = row_pointers.size(0) - 1, X.size(1)
    if Z.size(0) != N or Z.size(1) != D:
        raise RuntimeError("output must be [num_nodes, embedding_dim]")
    c = _planned_call((row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type),
                      row_nzr, D, X.size(0), X.device, workspace)
    with c:
        check(lib().hcspmm_forward_typed(_ptr(X), X.size(0), X.stride(0), _ptr(Z), Z.stride(0), _DTYPES[X.dtype], *c.graph,
                                         *c.ws))
    return Z


def _check_values(values, E, device):
    # the reference-style CHECK_INPUT messages (hybrid_all.cpp:185-187), then the weighted operand's own contract
    _check_input(values, "values")
    if values.dtype != torch.float32:
        raise RuntimeError("values must be a float32 tensor")
    if values.dim() != 1 or values.numel() != E:
        raise RuntimeError("values must hold one float32 per stored entry: %d, got %s" % (E, tuple(values.shape)))
    if values.device != device:
        raise RuntimeError("values must be on the device of the input")


def forward_weighted(X, values, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                     col_nzr):
    """Edge-weighted aggregation -> [A_w * X]: values[e] (float32, one per entry of column_index) weights entry e.  Same
    plan, registry, fingerprint check and workspace handling as forward; X may be float32 / float16 / bfloat16 (Z has its
    dtype, values stay float32).  values == 1 gives forward's bits.  The values are read on every call (hcspmm.h
    hcspmm_forward_weighted)."""
    c = _graph_args(X, (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type),
                       row_nzr, dtypes=tuple(_DTYPES))
    N, E, D = c.N, c.E, c.D
    _check_values(values, E, X.device)
    Z = torch.empty((N, D), dtype=X.dtype, device=X.device)
    with c:
        check(lib().hcspmm_forward_weighted(_ptr(X), X.size(0), D, _ptr(Z), D, _DTYPES[X.dtype], *c.graph, *c.ws,
                                            _ptr(values if E else torch.zeros(1, device=X.device))))  # (NULL values: EINVAL)
    return [Z]


_FP8_E4M3 = 0  # HCSPMM_FP8_E4M3


def _check_row_scale(scale, X):
    _check_input(scale, "scale")
    if scale.dtype != torch.float32 or scale.dim() != 1 or scale.numel() != X.size(0) or scale.device != X.device:
        raise RuntimeError("scale must hold one float32 per row of the input, on its device")


def quantize_fp8(X, scale=None):
    """Per-row quantiser -> (Xq, scale): Xq torch.float8_e4m3fn [rows, D], scale float32 [rows] with
    Xq[r] = rne_e4m3(clamp(X[r] / scale[r], -448, 448)) and scale[r] = amax_r / 448 over the row's finite entries (1 for a row
    without any, or all zeros).  A caller's `scale` (float32 [rows]) replaces the computed one.  D % 4 == 0
    (hcspmm.h hcspmm_quantize_fp8)."""
    _check_input(X, "input")
    if X.dtype != torch.float32 or X.dim() != 2:
        raise RuntimeError("input must be a 2-D float32 tensor")
    rows, D = X.size(0), X.size(1)
    if D == 0 or D % 4 != 0:
        raise RuntimeError("the 8-bit kernels take embedding widths that are multiples of 4, got %d" % D)
    if scale is not None:
        _check_row_scale(scale, X)
    Xq = torch.empty((rows, D), dtype=torch.uint8, device=X.device)
    out = torch.empty(rows, dtype=torch.float32, device=X.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(X.device).cuda_stream)
    with _on_device(X.device):
        check(lib().hcspmm_quantize_fp8(_ptr(X), rows, D, D, _FP8_E4M3, _ptr(scale), _ptr(Xq), D, _ptr(out), stream))
    return Xq.view(torch.float8_e4m3fn), out


def _spmm_fp8(Xq, scale, values, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr):
    _check_input(Xq, "input")
    _check_graph(row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow,
                 input_error=None if Xq.dtype in (torch.float8_e4m3fn, torch.uint8) and Xq.dim() == 2 else
                 "input must be a 2-D float8_e4m3fn (or uint8) tensor")
    N, E, D = row_pointers.size(0) - 1, column_index.size(0), Xq.size(1)
    if Xq.size(0) != N:
        raise RuntimeError("input has %d rows but the graph has %d nodes" % (Xq.size(0), N))
    if D == 0 or D % 4 != 0:
        raise RuntimeError("the 8-bit kernels take embedding widths that are multiples of 4, got %d" % D)
    if scale is not None:
        _check_row_scale(scale, Xq)
    if values is not None:
        _check_values(values, E, Xq.device)
    c = _planned_call((row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type),
                      row_nzr, D, Xq.size(0), Xq.device)
    Z = torch.empty((N, D), dtype=torch.float32, device=Xq.device)
    with c:
        check(lib().hcspmm_forward_fp8(_ptr(Xq), Xq.size(0), D, _FP8_E4M3, _ptr(scale), _ptr(values), _ptr(Z), D, *c.graph,
                                       *c.ws))
    return Z


def forward_fp8(Xq, scale, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr):
    """Aggregation of 8-bit features -> [A * (scale[:, None] * Xq)], float32: Xq float8_e4m3fn (or uint8 codes) [N, D] as
    quantize_fp8 gives it, scale float32 [N] or None (= 1).  Codes are gathered as stored, widened exactly and accumulated in
    fp32 (hcspmm.h hcspmm_forward_fp8)."""
    return [_spmm_fp8(Xq, scale, None, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr)]


def forward_weighted_fp8(Xq, scale, values, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type,
                         row_nzr, col_nzr):
    """forward_fp8 with edge values -> [A_w * (scale[:, None] * Xq)]: entry e of column c weighs values[e] * scale[c] (one fp32
    multiplication), every step an fp32 fma in forward_weighted's order (hcspmm.h hcspmm_forward_fp8)."""
    if values is None:
        raise RuntimeError("values must be a CUDA tensor")
    return [_spmm_fp8(Xq, scale, values, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr)]


def _check_heads_width(D, heads, dtype):
    # the multi-head kernels' limits (hcspmm.h hcspmm_forward_weighted_heads / hcspmm_sddmm_heads)
    if dtype != torch.float32:
        raise RuntimeError("the multi-head kernels take float32 features only, got %s" % (dtype,))
    if heads < 1 or D % heads != 0 or (D // heads) % 4 != 0:
        raise RuntimeError("the multi-head kernels need heads >= 1 and D = heads * Dh with Dh a multiple of 4: D = %d, heads = %d"
                           % (D, heads))


def forward_weighted_heads(X, values, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type,
                           row_nzr, col_nzr):
    """Multi-head edge-weighted aggregation -> [Z]: values [heads, E] (float32, head-major), X [rows, D] float32 with
    D = heads * Dh, Dh % 4 == 0; Z[:, h*Dh:(h+1)*Dh] = A_{values[h]} X[:, h*Dh:(h+1)*Dh], all heads in one launch.  Each
    head's columns are bit for bit forward_weighted(X, values[h]) at full width (hcspmm.h hcspmm_forward_weighted_heads)."""
    c = _graph_args(X, (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type),
                       row_nzr, dtypes=tuple(_DTYPES))
    N, E, D = c.N, c.E, c.D
    _check_input(values, "values")
    if values.dtype != torch.float32:
        raise RuntimeError("values must be a float32 tensor")
    if values.dim() != 2 or values.size(1) != E or values.size(0) < 1:
        raise RuntimeError("values must be [heads, E] with E = %d, got %s" % (E, tuple(values.shape)))
    if values.device != X.device:
        raise RuntimeError("values must be on the device of the input")
    heads = values.size(0)
    _check_heads_width(D, heads, X.dtype)
    Z = torch.empty((N, D), dtype=X.dtype, device=X.device)
    with c:
        check(lib().hcspmm_forward_weighted_heads(_ptr(X), X.size(0), D, _ptr(Z), D, _DTYPES[X.dtype], *c.graph, *c.ws,
                                                  _ptr(values if E else torch.zeros(1, device=X.device)), heads))
    return [Z]


def forward_weighted_indexed(X, values, value_index, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow,
                             hybrid_type, row_nzr, col_nzr):
    """forward_weighted_heads whose weight for entry e is values[h, value_index[e]] -> [Z]: values [heads, V] (or [V]: one
    head, any D forward_weighted takes), value_index int32 [E] with every index in [0, V).  Bit for bit
    forward_weighted_heads(X, values[:, value_index]) without the gathered copy (hcspmm.h hcspmm_forward_weighted_indexed)."""
    c = _graph_args(X, (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type),
                       row_nzr, dtypes=tuple(_DTYPES))
    N, E, D = c.N, c.E, c.D
    _check_input(values, "values")
    _check_input(value_index, "value_index")
    if values.dtype != torch.float32:
        raise RuntimeError("values must be a float32 tensor")
    if values.dim() not in (1, 2) or (values.dim() == 2 and values.size(0) < 1):
        raise RuntimeError("values must be [heads, V] or [V], got %s" % (tuple(values.shape),))
    if value_index.dtype != torch.int32 or value_index.dim() != 1 or value_index.numel() != E:
        raise RuntimeError("value_index must be an int32 [E] tensor with E = %d, got %s %s"
                           % (E, value_index.dtype, tuple(value_index.shape)))
    if values.device != X.device or value_index.device != X.device:
        raise RuntimeError("values and value_index must be on the device of the input")
    heads, V = (1, values.size(0)) if values.dim() == 1 else tuple(values.shape)
    if X.dtype != torch.float32:
        raise RuntimeError("the indexed kernels take float32 features only, got %s" % X.dtype)
    if heads > 1:
        _check_heads_width(D, heads, X.dtype)
    Z = torch.empty((N, D), dtype=X.dtype, device=X.device)
    with c:
        check(lib().hcspmm_forward_weighted_indexed(_ptr(X), X.size(0), D, _ptr(Z), D, _DTYPES[X.dtype], *c.graph, *c.ws,
                                                    _ptr(values if V else torch.zeros(1, device=X.device)), heads,
                                                    _ptr(value_index), V))
    return [Z]


def _extremum(X, graph, reduce, return_arg):
    row_nzr = graph[6]
    _check_graph(*graph[:5])
    if not X.is_cuda:
        raise RuntimeError("input must be a CUDA tensor")
    if X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or X.stride(0) < X.size(1):
        raise RuntimeError("input must be a 2-D float32 view with unit inner stride (max / min aggregation is float32 only)")
    N, D = graph[0].size(0) - 1, X.size(1)
    c = _planned_call(graph[:6], row_nzr, D, X.size(0), X.device, ws_fn=_ws_bytes_extremum)
    Z = torch.empty((N, D), dtype=torch.float32, device=X.device)
    arg = torch.empty((N, D), dtype=torch.int32, device=X.device) if return_arg else None
    with c:
        check(lib().hcspmm_forward_extremum(_ptr(X), X.size(0), X.stride(0), _ptr(Z), D, 0, *c.graph, *c.ws, reduce,
                                            _ptr(arg) if arg is not None else ctypes.c_void_p(0), D))
    return [Z, arg] if return_arg else [Z]


def forward_max(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
                return_arg=True):
    """Max over each row's neighbours -> [Z, arg] ([Z] with return_arg=False): Z[r][d] = max of X[col(e)][d] over the
    entries e of row r, arg[r][d] = the winning e (int32).  Ties go to the lowest e, NaN wins, rows without entries give 0
    and -1 (hcspmm.h hcspmm_forward_extremum).  X: float32 [rows, D] view with unit inner stride (rows >= the columns the
    graph refers to)."""
    return _extremum(X, (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr),
                     0, return_arg)


def forward_min(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
                return_arg=True):
    """Min over each row's neighbours: forward_max's contract with min (NaN still wins)."""
    return _extremum(X, (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr),
                     1, return_arg)


def forward_extremum_backward(grad_Z, arg, perm, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow,
                              hybrid_type, row_nzr, col_nzr):
    """Backward of forward_max / forward_min on a square, pattern-symmetric graph -> grad_X [N, D]:
    grad_X[j][d] = sum of grad_Z[i][d] over the entries e = (i, j) with arg[i][d] == e.  perm: the int32 transpose
    permutation (transpose_permutation(...).int()).  Deterministic, no atomics (hcspmm.h hcspmm_forward_extremum_backward)."""
    _check_graph(row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
    for t, n in ((grad_Z, "grad_Z"), (arg, "arg"), (perm, "perm")):
        _check_input(t, n)
    N, E = row_pointers.size(0) - 1, column_index.size(0)
    if grad_Z.dtype != torch.float32 or grad_Z.dim() != 2 or grad_Z.size(0) != N:
        raise RuntimeError("grad_Z must be a float32 [num_nodes, D] tensor")
    D = grad_Z.size(1)
    if arg.dtype != torch.int32 or tuple(arg.shape) != (N, D):
        raise RuntimeError("arg must be the int32 [num_nodes, D] argmax of the forward")
    if perm.dtype != torch.int32 or perm.dim() != 1 or perm.numel() != E:
        raise RuntimeError("perm must be an int32 [E] tensor with E = %d, got %s %s" % (E, perm.dtype, tuple(perm.shape)))
    for t, n in ((arg, "arg"), (perm, "perm")):
        if t.device != grad_Z.device:
            raise RuntimeError("%s must be on the device of grad_Z" % n)
    c = _planned_call((row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type),
                      row_nzr, D, N, grad_Z.device)
    grad_X = torch.empty((N, D), dtype=torch.float32, device=grad_Z.device)
    with c:
        check(lib().hcspmm_forward_extremum_backward(_ptr(grad_Z), D, _ptr(arg), D, _ptr(grad_X), D, *c.graph, _ptr(perm),
                                                     *c.ws))
    return grad_X


def _ws_bytes_multi(h, D):
    return int(lib().hcspmm_multi_workspace_bytes(ctypes.byref(h), D))


MULTI_AGGREGATES = ("sum", "sumsq", "max", "min")


def _multi_wanted(aggregates):
    """which of MULTI_AGGREGATES a forward_multi call asks for, in that order"""
    aggregates = (aggregates,) if isinstance(aggregates, str) else tuple(aggregates)
    for a in aggregates:
        if a not in MULTI_AGGREGATES:
            raise ValueError("aggregates must be among %s, got %r" % (", ".join(repr(k) for k in MULTI_AGGREGATES), a))
    if not aggregates:
        raise ValueError("aggregates must name at least one of %s" % ", ".join(repr(k) for k in MULTI_AGGREGATES))
    return [a in aggregates for a in MULTI_AGGREGATES]


def forward_multi(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
                  aggregates=MULTI_AGGREGATES, return_arg=True):
    """Sum, sum of squares, max and min over each row's neighbours in one gather pass -> [Z_sum, Z_sumsq, Z_max, Z_min, arg_max,
    arg_min] (hcspmm.h hcspmm_forward_multi): contiguous [N, D] tensors, float32 values and int32 args.  An aggregate that
    `aggregates` does not name is None, and so is the arg of an extremum that was not asked for; both args are None with
    return_arg=False.  max / min / args follow forward_max's contract bit for bit.  X: as for forward_max."""
    want = _multi_wanted(aggregates)
    _check_graph(row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
    if not X.is_cuda:
        raise RuntimeError("input must be a CUDA tensor")
    if X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or X.stride(0) < X.size(1):
        raise RuntimeError("input must be a 2-D float32 view with unit inner stride (multi aggregation is float32 only)")
    N, D = row_pointers.size(0) - 1, X.size(1)
    c = _planned_call((row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type), row_nzr, D, X.size(0),
                      X.device, ws_fn=_ws_bytes_multi)
    Z = [torch.empty((N, D), dtype=torch.float32, device=X.device) if w else None for w in want]
    args = [torch.empty((N, D), dtype=torch.int32, device=X.device) if (w and return_arg) else None for w in want[2:]]
    if N == 0:
        return Z + args
    null = ctypes.c_void_p(0)
    with c:
        check(lib().hcspmm_forward_multi(_ptr(X), X.size(0), X.stride(0), 0, *(_ptr(z) if z is not None else null for z in Z), D,
                                         *(_ptr(a) if a is not None else null for a in args), D, *c.graph, *c.ws))
    return Z + args


def _ws_bytes_softmax(h, D):
    return int(lib().hcspmm_softmax_workspace_bytes(ctypes.byref(h), D))


def _beta_vector(beta, D, device):
    """beta of the softmax aggregation as a float32 [D] device vector: a Python number, or a float32 tensor of 1 or D elements
    on the input's device, broadcast there (no host synchronisation: the call captures into a HIP graph)"""
    if isinstance(beta, torch.Tensor):
        if beta.dtype != torch.float32 or beta.numel() not in (1, D) or beta.device != device:
            raise RuntimeError("beta must be a Python float or a float32 tensor with 1 or D = %d elements on the device of the "
                               "input, got %s %s on %s" % (D, beta.dtype, tuple(beta.shape), beta.device))
        return beta.detach().reshape(-1).expand(D).contiguous()
    return torch.full((D,), float(beta), dtype=torch.float32, device=device)


def forward_softmax(X, beta, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
                    return_stats=True):
    """Per-channel softmax aggregation of each row's neighbours in one gather pass -> (Z, M, L, Q) (hcspmm.h
    hcspmm_forward_softmax): Z[r][d] = sum_e p_e x_e with p_e = softmax over the row's entries of beta[d] * x_e, and the
    statistics of its backward, M = max_e fl(beta x_e), L = sum_e exp(beta x_e - M), Q = sum_e p_e x_e^2 -- contiguous float32
    [N, D].  return_stats: True for all three, False for none ((Z, None, None, None)), or an iterable naming some of "M", "L",
    "Q"; a statistic not asked for is None.  beta: a Python float or a float32 tensor of 1 or D elements.  Rows without
    entries give Z = Q = 0, M = -inf, L = 0.  X: as for forward_max."""
    if isinstance(return_stats, (str, bytes)):
        return_stats = (return_stats,)
    if not hasattr(return_stats, "__iter__"):  # a bool, or anything else with a truth value (0 / 1, numpy.bool_)
        want = [bool(return_stats)] * 3
    else:
        names = tuple(return_stats)
        for n in names:
            if n not in ("M", "L", "Q"):
                raise ValueError("return_stats must be a bool or name some of 'M', 'L', 'Q', got %r" % (n,))
        want = [n in names for n in ("M", "L", "Q")]
    _check_graph(row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
    if not X.is_cuda:
        raise RuntimeError("input must be a CUDA tensor")
    if X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or X.stride(0) < X.size(1):
        raise RuntimeError("input must be a 2-D float32 view with unit inner stride (softmax aggregation is float32 only)")
    N, D = row_pointers.size(0) - 1, X.size(1)
    if D == 0:
        raise RuntimeError("input must have at least one column")
    b = _beta_vector(beta, D, X.device)
    c = _planned_call((row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type), row_nzr, D, X.size(0),
                      X.device, ws_fn=_ws_bytes_softmax)
    Z = torch.empty((N, D), dtype=torch.float32, device=X.device)
    stats = [torch.empty((N, D), dtype=torch.float32, device=X.device) if w else None for w in want]
    if N == 0:
        return (Z, *stats)
    null = ctypes.c_void_p(0)
    with c:
        check(lib().hcspmm_forward_softmax(_ptr(X), X.size(0), X.stride(0), 0, _ptr(b), _ptr(Z),
                                           *(_ptr(t) if t is not None else null for t in stats), D, *c.graph, *c.ws))
    return (Z, *stats)


def softmax_backward(grad_Z, Z, M, L, X, beta, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type,
                     row_nzr, col_nzr):
    """Gradient of forward_softmax with respect to X -> float32 [n, D], on the graph the backward WALKS (A^T's eight tensors, or
    A's own for a symmetric pattern; n rows): dX[j] = sum over the entries (j, i) of row j of exp(beta x_j - M[i]) / L[i] * grad_Z[i]
    * (1 + beta (x_j - Z[i])).  grad_Z, Z, M, L: contiguous float32 [rows, D] of the forward (rows >= the walked graph's column
    ids); X: the float32 [n, D] view the forward gathered; beta as for forward_softmax.  Deterministic, no atomics (hcspmm.h
    hcspmm_softmax_backward).  The gradient with respect to beta is (grad_Z * (Q - Z * Z)).sum(0)."""
    _check_graph(row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
    for t, n in ((grad_Z, "grad_Z"), (Z, "Z"), (M, "M"), (L, "L")):
        _check_input(t, n)
    if not X.is_cuda:
        raise RuntimeError("input must be a CUDA tensor")
    if X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or X.stride(0) < X.size(1):
        raise RuntimeError("input must be a 2-D float32 view with unit inner stride (softmax aggregation is float32 only)")
    n, D = row_pointers.size(0) - 1, X.size(1)
    if X.size(0) != n:
        raise RuntimeError("input has %d rows but the walked graph has %d nodes" % (X.size(0), n))
    if grad_Z.dtype != torch.float32 or grad_Z.dim() != 2 or grad_Z.size(1) != D or D == 0:
        raise RuntimeError("grad_Z must be a float32 [rows, D] tensor with D = %d > 0, got %s %s" % (D, grad_Z.dtype, tuple(grad_Z.shape)))
    for t, name in ((Z, "Z"), (M, "M"), (L, "L")):
        if t.dtype != torch.float32 or t.shape != grad_Z.shape or t.device != X.device:
            raise RuntimeError("%s must be a float32 tensor of grad_Z's shape on the device of the input" % name)
    if grad_Z.device != X.device:
        raise RuntimeError("grad_Z must be on the device of the input")
    b = _beta_vector(beta, D, X.device)
    c = _planned_call((row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type), row_nzr, D,
                      grad_Z.size(0), X.device)
    if c.E > 0 and grad_Z.size(0) == 0:
        raise RuntimeError("grad_Z has no rows but the walked graph has %d entries" % c.E)
    grad_X = torch.empty((n, D), dtype=torch.float32, device=X.device)
    if n == 0:
        return grad_X
    with c:
        check(lib().hcspmm_softmax_backward(_ptr(grad_Z), _ptr(Z), _ptr(M), _ptr(L), D, grad_Z.size(0), _ptr(X), X.stride(0),
                                            _ptr(b), _ptr(grad_X), D, *c.graph, *c.ws))
    return grad_X


def _ws_bytes_gated(h, D):
    return int(lib().hcspmm_gated_workspace_bytes(ctypes.byref(h), D))


GATED_OUTPUTS = ("gate", "dgate")


def forward_gated(P, Q, V, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
                  outputs=("gate",)):
    """Gated neighbour aggregation in one gather pass -> (Z_gate, Z_dgate) (hcspmm.h hcspmm_forward_gated): with
    z = P[i] + Q[j] over the entries (i, j) of row i, Z_gate[i] = sum_j sigmoid(z) * V[j] and Z_dgate[i] = sum_j sigmoid'(z) * V[j],
    contiguous float32 [N, D].  outputs names some of "gate", "dgate"; an output not asked for is None, and one asked for has
    the same bits whether or not the other is.  P: float32 [N, D]; Q, V: float32 [rows, D] (rows >= the columns the graph refers
    to); all three 2-D views with unit inner stride and their own row strides (column blocks of one projection pass as they
    are).  Rows without entries give 0.  No per-entry tensor is built."""
    outputs = (outputs,) if isinstance(outputs, (str, bytes)) else tuple(outputs)
    for n in outputs:
        if n not in GATED_OUTPUTS:
            raise ValueError("outputs must name some of 'gate', 'dgate', got %r" % (n,))
    if not outputs:
        raise ValueError("outputs must name at least one of 'gate', 'dgate'")
    want = [n in outputs for n in GATED_OUTPUTS]
    _check_graph(row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
    for t in (P, Q, V):
        if not t.is_cuda:
            raise RuntimeError("P, Q and V must be CUDA tensors")
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.size(1):
            raise RuntimeError("P, Q and V must be 2-D float32 views with unit inner stride (gated aggregation is float32 only)")
    N, E, D = row_pointers.size(0) - 1, column_index.size(0), Q.size(1)
    if D == 0:
        raise RuntimeError("P, Q and V must have at least one column")
    if P.size(1) != D or V.size(1) != D:
        raise RuntimeError("P, Q and V must have the same width, got %d, %d and %d" % (P.size(1), D, V.size(1)))
    if V.size(0) != Q.size(0):
        raise RuntimeError("Q and V must have the same number of rows, got %d and %d" % (Q.size(0), V.size(0)))
    if P.device != Q.device or V.device != Q.device:
        raise RuntimeError("P, Q and V must be on one device")
    if P.size(0) != N:
        raise RuntimeError("P has %d rows but the graph has %d nodes" % (P.size(0), N))
    c = _planned_call((row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type), row_nzr, D, Q.size(0),
                      Q.device, ws_fn=_ws_bytes_gated)
    if E > 0 and Q.size(0) == 0:
        raise RuntimeError("Q and V have no rows but the graph has %d entries" % E)
    Z = [torch.empty((N, D), dtype=torch.float32, device=Q.device) if w else None for w in want]
    if N == 0:
        return tuple(Z)
    null = ctypes.c_void_p(0)
    with c:
        check(lib().hcspmm_forward_gated(_ptr(P), P.stride(0), _ptr(Q), Q.stride(0), _ptr(V), V.stride(0), Q.size(0),
                                         *(_ptr(z) if z is not None else null for z in Z), D, *c.graph, *c.ws))
    return tuple(Z)


EDGE_OPS = {"mul": 0, "add_relu": 1, "copy": 2}  # include/hcspmm.h HCSPMM_EDGE_OP_*


def _edge_op(op):
    if op not in EDGE_OPS:
        raise ValueError("op must be one of %s, got %r" % (", ".join(repr(k) for k in EDGE_OPS), op))
    return EDGE_OPS[op]


def _check_f32_view(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.size(1):
        raise RuntimeError("%s must be a 2-D float32 view with unit inner stride" % name)


def forward_edge_messages(X, F, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
                          op="add_relu", index=None):
    """Edge-feature messages -> [Z]: Z[r] = sum over the entries e of row r of m(X[col(e)], F[fi(e)]), fi(e) = index[e] (int32
    [E]) or e.  op: "mul" x * f, "add_relu" relu(x + f), "copy" f (X may be None).  X [rows, D] and F [f_rows, D] are float32
    views with unit inner stride; F is read on every call.  Deterministic, no atomics (hcspmm.h hcspmm_forward_edge_messages).
    The gradient with respect to X is this call on A^T's graph with index = entry_index_t (or, on a pattern-symmetric graph,
    the int32 transpose permutation): "mul" with X := dZ, "add_relu" as "copy" of edge_messages_grad's result."""
    code = _edge_op(op)
    _check_graph(row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow)
    _check_f32_view(F, "F")
    N, E, D = row_pointers.size(0) - 1, column_index.size(0), F.size(1)
    if X is None and op != "copy":
        raise RuntimeError("input may be None for op='copy' only")
    if X is not None:
        _check_f32_view(X, "input")
        if X.size(1) != D or X.device != F.device:
            raise RuntimeError("input and F must have the same width and device, got %s and %s" % (tuple(X.shape), tuple(F.shape)))
    if index is not None:
        _check_input(index, "index")
        if index.dtype != torch.int32 or index.dim() != 1 or index.numel() != E or index.device != F.device:
            raise RuntimeError("index must be an int32 [E] tensor with E = %d on the device of F, got %s %s"
                               % (E, index.dtype, tuple(index.shape)))
    elif F.size(0) < E:
        raise RuntimeError("F has %d rows but the graph has %d entries" % (F.size(0), E))
    if D == 0:
        raise RuntimeError("F must have at least one column")
    c = _planned_call((row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type),
                      row_nzr, D, X.size(0) if X is not None else 1 << 62, F.device)  # (copy: no gathered rows)
    Z = torch.empty((N, D), dtype=torch.float32, device=F.device)
    with c:
        check(lib().hcspmm_forward_edge_messages(_ptr(X), X.size(0) if X is not None else 0,
                                                 X.stride(0) if X is not None else D, _ptr(F), F.size(0), F.stride(0),
                                                 _ptr(index), code, _ptr(Z), D, *c.graph, *c.ws))
    return [Z]


def edge_messages_grad(dZ, X, F, row_pointers, column_index, op="add_relu"):
    """Gradient of forward_edge_messages (direct form) with respect to F -> float32 [E, D]: "mul" dZ[row(e)] * X[col(e)],
    "add_relu" dZ[row(e)] where X[col(e)] + F[e] > 0 and +0 elsewhere, "copy" dZ[row(e)] (X and F may be None).  Edge-parallel,
    every element written once (hcspmm.h hcspmm_edge_messages_grad)."""
    code = _edge_op(op)
    _check_graph(row_pointers, column_index)
    _check_f32_view(dZ, "dZ")
    N, E, D = row_pointers.size(0) - 1, column_index.size(0), dZ.size(1)
    if dZ.size(0) != N:
        raise RuntimeError("dZ has %d rows but the graph has %d nodes" % (dZ.size(0), N))
    if op != "copy":
        if X is None:
            raise RuntimeError("input may be None for op='copy' only")
        _check_f32_view(X, "input")
        if X.size(1) != D or X.device != dZ.device:
            raise RuntimeError("input must have the width and device of dZ")
    if op == "add_relu":
        if F is None:
            raise RuntimeError("F is required for op='add_relu'")
        _check_f32_view(F, "F")
        if F.size(1) != D or F.size(0) < E or F.device != dZ.device:
            raise RuntimeError("F must be [E, D] with E = %d, D = %d on the device of dZ, got %s" % (E, D, tuple(F.shape)))
    reads_x, reads_f = op != "copy", op == "add_relu"
    out = torch.empty((E, D), dtype=torch.float32, device=dZ.device)
    if D == 0:
        return out
    stream = ctypes.c_void_p(torch.cuda.current_stream(dZ.device).cuda_stream)
    with _on_device(dZ.device):
        check(lib().hcspmm_edge_messages_grad(_ptr(dZ), dZ.stride(0), _ptr(X) if reads_x else ctypes.c_void_p(0),
                                              X.size(0) if reads_x else 0, X.stride(0) if reads_x else D,
                                              _ptr(F) if reads_f else ctypes.c_void_p(0), F.stride(0) if reads_f else D, _ptr(out), D,
                                              code, _ptr(row_pointers), _ptr(column_index), N, E, D, stream))
    return out


_NORMS = {"sym": 0, "mean": 1}


def edge_norm(row_pointers, column_index, kind):
    """Edge values of a normalised aggregation, computed on the device -> float32 [E]:
    "sym" = 1/sqrt(deg_r * deg_c) (GCN), "mean" = 1/deg_r (GraphSAGE-mean); deg = row length."""
    if kind not in _NORMS:
        raise ValueError("kind must be 'sym' or 'mean', got %r" % (kind,))
    _check_graph(row_pointers, column_index)
    N, E = row_pointers.numel() - 1, column_index.numel()
    out = torch.empty(E, dtype=torch.float32, device=row_pointers.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(row_pointers.device).cuda_stream)
    with _on_device(row_pointers.device):
        check(lib().hcspmm_edge_norm_device(_ptr(row_pointers), _ptr(column_index), N, E, _NORMS[kind], _ptr(out), stream))
    return out


def transpose_permutation(row_pointers, column_index):
    """perm (int64, on the graph's device) with values[perm] = the values of A_w^T in A's own CSR order, for a
    pattern-symmetric graph (hcspmm_transpose_permutation; an asymmetric pattern raises)."""
    rp = _i32_host(row_pointers)
    col = _i32_host(column_index)
    N, E = rp.numel() - 1, col.numel()
    perm = torch.empty(E, dtype=torch.int32)
    check(lib().hcspmm_transpose_permutation(_ptr(rp), _ptr(col), N, E, _ptr(perm)))
    return perm.to(device=row_pointers.device, dtype=torch.int64)


def transpose_graph(row_pointers, column_index, num_cols=None):
    """A^T of any CSR graph (hcspmm_transpose_graph, a host counting sort) -> (row_pointers_t, column_index_t,
    entry_index_t), int32 on the inputs' device: entry e_t of row j of A^T is A's entry (i, j) with i = column_index_t[e_t]
    at CSR position entry_index_t[e_t].  num_cols: the columns of a rectangular block (default: square)."""
    rp = _i32_host(row_pointers)
    col = _i32_host(column_index)
    N, E = rp.numel() - 1, col.numel()
    M = N if num_cols is None else int(num_cols)
    if M < 0:
        raise RuntimeError("num_cols must not be negative, got %d" % M)
    rp_t = torch.empty(M + 1, dtype=torch.int32)
    col_t, eid_t = torch.empty(E, dtype=torch.int32), torch.empty(E, dtype=torch.int32)
    check(lib().hcspmm_transpose_graph(_ptr(rp), _ptr(col), N, M, E, _ptr(rp_t), _ptr(col_t), _ptr(eid_t)))
    dev = row_pointers.device
    return rp_t.to(dev), col_t.to(dev), eid_t.to(dev)


def _device_graph(row_pointers, column_index):
    """the checks of the entry points that BUILD graphs on the device -> (N, E, stream)"""
    _check_graph(row_pointers, column_index)
    if row_pointers.dim() != 1 or row_pointers.numel() < 1 or column_index.dim() != 1:
        raise RuntimeError("row_pointers [N + 1] and column_index [E] must be 1-D")
    if column_index.device != row_pointers.device:
        raise RuntimeError("column_index must be on the device of row_pointers")
    return (row_pointers.numel() - 1, column_index.numel(),
            ctypes.c_void_p(torch.cuda.current_stream(row_pointers.device).cuda_stream))


def transpose_graph_device(row_pointers, column_index, num_cols=None):
    """transpose_graph built on the device (hcspmm_transpose_graph_device, a stable radix sort by column) -> the same
    (row_pointers_t, column_index_t, entry_index_t), element for element, asynchronously on the current stream and with no host
    copy.  What transpose_graph validates is trusted here: ids in [0, num_cols), row_pointers[0] = 0, row_pointers[N] = E."""
    N, E, stream = _device_graph(row_pointers, column_index)
    M = N if num_cols is None else int(num_cols)
    if M < 0:
        raise RuntimeError("num_cols must not be negative, got %d" % M)
    dev = row_pointers.device
    rp_t = torch.empty(M + 1, dtype=torch.int32, device=dev)
    col_t, eid_t = torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev)
    ws_bytes = int(lib().hcspmm_transpose_graph_device_workspace_bytes(N, M, E))
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    with _on_device(dev):
        check(lib().hcspmm_transpose_graph_device(_ptr(row_pointers), _ptr(column_index), N, M, E, _ptr(rp_t), _ptr(col_t),
                                                  _ptr(eid_t), _ptr(ws), ws_bytes, stream))
    return rp_t, col_t, eid_t


# Rows longer than the fanout are selected by one wave up to this many entries and by a workgroup beyond (hcspmm.h
# HCSPMM_SAMPLE_WAVE_ROW_MAX); the other class limit is the fanout itself.
SAMPLE_WAVE_ROW_MAX = 512


def sample_row_pointers(row_pointers, fanout):
    """row_pointers_s of every sample of this graph at this fanout: the exclusive scan of min(deg, fanout), on the device
    (hcspmm_sample_row_pointers_device).  It does not depend on the seed: make it once per (graph, fanout)."""
    _check_input(row_pointers, "nodePointer")
    if row_pointers.dtype != torch.int32 or row_pointers.dim() != 1 or row_pointers.numel() < 1:
        raise RuntimeError("nodePointer must be a 1-D int32 tensor [N + 1]")
    if int(fanout) < 1:
        raise RuntimeError("fanout must be at least 1, got %d" % int(fanout))
    N, dev = row_pointers.numel() - 1, row_pointers.device
    rp_s = torch.empty(N + 1, dtype=torch.int32, device=dev)
    ws_bytes = int(lib().hcspmm_sample_workspace_bytes(N))
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    with _on_device(dev):
        check(lib().hcspmm_sample_row_pointers_device(_ptr(row_pointers), N, int(fanout), _ptr(rp_s), _ptr(ws), ws_bytes,
                                                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return rp_s


def sample_neighbors(row_pointers, column_index, fanout, seed, row_pointers_s=None):
    """A fanout-limited sample of every row's neighbours, on the device (hcspmm_sample_neighbors_device) ->
    (row_pointers_s, column_index_s, entry_index_s), int32: a row with at most `fanout` entries keeps them all, a longer one the
    `fanout` entries with the smallest key(e, seed) (include/hcspmm.h), in ascending CSR position; entry_index_s names the kept
    entries' positions in A, so edge values travel as values[entry_index_s] or through forward_weighted_indexed.  seed: any
    integer, taken modulo 2^64.  row_pointers_s: sample_row_pointers(row_pointers, fanout) when the caller kept it -- the call
    then reads nothing back from the device (without it E_s, four bytes, is read once)."""
    N, E, stream = _device_graph(row_pointers, column_index)
    if int(fanout) < 1:
        raise RuntimeError("fanout must be at least 1, got %d" % int(fanout))
    if row_pointers_s is None:
        row_pointers_s = sample_row_pointers(row_pointers, fanout)
    else:
        _check_input(row_pointers_s, "row_pointers_s")
        if row_pointers_s.dtype != torch.int32 or row_pointers_s.numel() != N + 1 or row_pointers_s.device != row_pointers.device:
            raise RuntimeError("row_pointers_s must be sample_row_pointers(row_pointers, fanout): int32 [N + 1] on the graph's device")
    E_s = _sampled_edges(row_pointers_s)
    dev = row_pointers.device
    col_s, eid_s = torch.empty(E_s, dtype=torch.int32, device=dev), torch.empty(E_s, dtype=torch.int32, device=dev)
    with _on_device(dev):
        check(lib().hcspmm_sample_neighbors_device(_ptr(row_pointers), _ptr(column_index), _ptr(row_pointers_s), N, E, int(fanout),
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(col_s), _ptr(eid_s), stream))
    return row_pointers_s, col_s, eid_s


_SAMPLED_EDGES = {}  # data_ptr of a row_pointers_s tensor -> (weak ref, E_s): the 4-byte read happens once per tensor


def _sampled_edges(row_pointers_s):
    key = row_pointers_s.data_ptr()
    hit = _SAMPLED_EDGES.get(key)
    if hit is not None and hit[0]() is row_pointers_s:
        return hit[1]
    E_s = int(row_pointers_s[-1].item())
    for k in [k for k, v in _SAMPLED_EDGES.items() if v[0]() is None]:
        del _SAMPLED_EDGES[k]
    _SAMPLED_EDGES[key] = (weakref.ref(row_pointers_s), E_s)
    return E_s


def plan_free_graph(row_pointers, column_index):
    """The eight graph tensors with which every entry point takes its plan-free, all-sparse-row path on (row_pointers,
    column_index), made on the device with no host copy: zero hybrid_type (every window on the sparse-row path, which reads
    row_pointers and column_index only), zero blockPartition, and [0] placeholders for row_nzr / col_nzr and for edgeToColumn /
    edgeToRow, which only dense-tile windows read.  For graphs that change from step to step (sample_neighbors,
    transpose_graph_device); a graph that is multiplied many times wants preprocess and its plan."""
    N, _, _ = _device_graph(row_pointers, column_index)
    dev = row_pointers.device
    windows = max((N + 15) // 16, 1)
    zeros = [torch.zeros(n, dtype=torch.int32, device=dev) for n in (windows, 1, 1, windows, 1, 1)]
    return [row_pointers, column_index] + zeros


def _check_view(t, name, dtype=None):
    # a 2-D row-major view: unit inner stride, any row stride (column slices of wider matrices need no copy)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if t.dtype not in _DTYPES or (dtype is not None and t.dtype != dtype) or t.dim() != 2 or t.stride(1) != 1 or \
            t.stride(0) < t.size(1):
        raise RuntimeError("%s must be a 2-D float32 / float16 / bfloat16 view with unit inner stride%s"
                           % (name, "" if dtype is None else ", of the dtype of A"))


def _sddmm(A, B, row_pointers, column_index, row_nzr, heads):
    """heads None: sddmm -> [E]; an int: sddmm_heads -> [heads, E]"""
    _check_graph(row_pointers, column_index)
    _check_view(A, "A")
    _check_view(B, "B", A.dtype)
    N, E, D = row_pointers.size(0) - 1, column_index.size(0), A.size(1)
    if A.size(0) != N:
        raise RuntimeError("A has %d rows but the graph has %d nodes" % (A.size(0), N))
    if B.size(1) != D:
        raise RuntimeError("B has %d columns but A has %d" % (B.size(1), D))
    if B.device != A.device:
        raise RuntimeError("B must be on the device of A")
    if heads is not None:
        _check_heads_width(D, heads, A.dtype)
    c = _planned_call((row_pointers, column_index), row_nzr, D, B.size(0), A.device, ws_fn=None)
    out = torch.empty(E if heads is None else (heads, E), dtype=torch.float32, device=A.device)
    operands = (_ptr(A), A.stride(0), _ptr(B), B.size(0), B.stride(0), _DTYPES[A.dtype], _ptr(out))
    with c:
        if heads is None:
            check(lib().hcspmm_sddmm(*operands, *c.graph, c.stream))
        else:
            check(lib().hcspmm_sddmm_heads(*operands, *c.graph, c.stream, heads))
    return out


def sddmm(A, B, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr):
    """Sampled dense-dense product on the stored entries -> float32 [E]: out[e] = <A[row(e)], B[column_index[e]]>
    (include/hcspmm.h hcspmm_sddmm).  A [N, D] and B [b_rows, D] are float32 / float16 / bfloat16 of one dtype, 2-D views
    with unit inner stride (column slices need no copy); 16-bit inputs are summed in fp32.  The graph tensors are those of
    forward_weighted: with a plan in row_nzr it is checked against this graph and B must have every row it gathers.  The
    gradient of forward_weighted with respect to its values is sddmm(dZ, X)."""
    return _sddmm(A, B, row_pointers, column_index, row_nzr, None)


def sddmm_heads(A, B, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
                heads):
    """Multi-head SDDMM -> float32 [heads, E]: out[h, e] = <A[row(e), h*Dh:(h+1)*Dh], B[column_index[e], h*Dh:(h+1)*Dh]>,
    all heads in one launch (hcspmm.h hcspmm_sddmm_heads).  A [N, D] and B [b_rows, D] float32 views with unit inner stride,
    D = heads * Dh, Dh % 4 == 0.  Each head is bit for bit sddmm on the column slices.  The gradient of
    forward_weighted_heads with respect to its values is sddmm_heads(dZ, X)."""
    return _sddmm(A, B, row_pointers, column_index, row_nzr, int(heads))


def _softmax_operand(t, name, E, device):
    _check_input(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError("%s must be a float32 tensor" % name)
    if t.dim() not in (1, 2) or t.size(-1) != E or t.numel() == 0 and E > 0:
        raise RuntimeError("%s must be [E] or [heads, E] with E = %d, got %s" % (name, E, tuple(t.shape)))
    if t.device != device:
        raise RuntimeError("%s must be on the device of row_pointers" % name)
    return 1 if t.dim() == 1 else t.size(0)


def edge_softmax(logits, row_pointers):
    """Softmax of float32 logits over each row's stored entries -> alpha of the same shape: [E] or [heads, E] (head-major:
    alpha[h] is a values vector forward_weighted takes as is).  Logits must be finite (hcspmm.h hcspmm_edge_softmax)."""
    _check_input(row_pointers, "nodePointer")
    N = row_pointers.numel() - 1
    E = logits.size(-1) if logits.dim() else -1
    heads = _softmax_operand(logits, "logits", E, row_pointers.device)
    alpha = torch.empty_like(logits)
    stream = ctypes.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)
    with _on_device(logits.device):
        check(lib().hcspmm_edge_softmax(_ptr(logits), _ptr(alpha), _ptr(row_pointers), N, E, heads, stream))
    return alpha


def edge_softmax_backward(alpha, grad_alpha, row_pointers):
    """grad_logits = alpha * (grad_alpha - sum over the row of alpha * grad_alpha), shapes as edge_softmax."""
    _check_input(row_pointers, "nodePointer")
    N = row_pointers.numel() - 1
    E = alpha.size(-1) if alpha.dim() else -1
    heads = _softmax_operand(alpha, "alpha", E, row_pointers.device)
    if grad_alpha.shape != alpha.shape:
        raise RuntimeError("grad_alpha must have the shape of alpha")
    _softmax_operand(grad_alpha, "grad_alpha", E, row_pointers.device)
    grad = torch.empty_like(alpha)
    stream = ctypes.c_void_p(torch.cuda.current_stream(alpha.device).cuda_stream)
    with _on_device(alpha.device):
        check(lib().hcspmm_edge_softmax_backward(_ptr(alpha), _ptr(grad_alpha), _ptr(grad), _ptr(row_pointers), N, E, heads,
                                                 stream))
    return grad


def _scores_operand(t, name, device):
    """GAT scores: float32 [rows] (one head) or [rows, heads], contiguous, on `device` -> (rows, heads)"""
    _check_input(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError("%s must be a float32 tensor" % name)
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.size(1) == 0):
        raise RuntimeError("%s must be [rows] or [rows, heads], got %s" % (name, tuple(t.shape)))
    if t.device != device:
        raise RuntimeError("%s must be on the device of row_pointers" % name)
    return t.size(0), 1 if t.dim() == 1 else t.size(1)


def _gat_graph(row_pointers, column_index, s_dst, s_src):
    _check_graph(row_pointers, column_index)
    N, E = row_pointers.numel() - 1, column_index.numel()
    n_dst, heads = _scores_operand(s_dst, "s_dst", row_pointers.device)
    src_rows, heads_src = _scores_operand(s_src, "s_src", row_pointers.device)
    if s_dst.dim() != s_src.dim() or heads != heads_src:
        raise RuntimeError("s_dst and s_src must have the same number of heads, got %s and %s"
                           % (tuple(s_dst.shape), tuple(s_src.shape)))
    if n_dst != N:
        raise RuntimeError("s_dst has %d rows but the graph has %d nodes" % (n_dst, N))
    return N, E, src_rows, heads


def gat_attention(s_dst, s_src, row_pointers, column_index, negative_slope=0.2):
    """GAT attention weights -> alpha float32 [E] (one head: s_* of shape [rows]) or [heads, E] (s_* [rows, heads]):
    alpha[h] = softmax over each row's entries of LeakyReLU(s_dst[row(e), h] + s_src[column_index[e], h]), bit for bit
    edge_softmax of those logits, in one launch for all heads (include/hcspmm.h hcspmm_gat_attention).  s_src may have
    any number of rows (a row block); column ids are trusted to be below it."""
    N, E, src_rows, heads = _gat_graph(row_pointers, column_index, s_dst, s_src)
    alpha = torch.empty((E,) if s_dst.dim() == 1 else (heads, E), dtype=torch.float32, device=s_dst.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(s_dst.device).cuda_stream)
    with _on_device(s_dst.device):
        check(lib().hcspmm_gat_attention(_ptr(s_dst), _ptr(s_src), src_rows, float(negative_slope), _ptr(alpha),
                                         _ptr(row_pointers), _ptr(column_index), N, E, heads, stream))
    return alpha


def _perm_i32(perm, E, device):
    _check_input(perm, "perm")
    if perm.dtype not in (torch.int32, torch.int64) or perm.dim() != 1 or perm.numel() != E:
        raise RuntimeError("perm must be an int32 / int64 [E] tensor with E = %d, got %s %s" % (E, perm.dtype, tuple(perm.shape)))
    if perm.device != device:
        raise RuntimeError("perm must be on the device of row_pointers")
    return perm if perm.dtype == torch.int32 else perm.to(torch.int32)


def _gat_attention_backward(alpha, grad_alpha, s_dst, s_src, row_pointers, column_index, row_pointers_t, perm, negative_slope):
    """row_pointers_t None: the pattern-symmetric form (perm = transpose_permutation's); else the directed form (perm =
    entry_index_t)"""
    N, E, src_rows, heads = _gat_graph(row_pointers, column_index, s_dst, s_src)
    if src_rows != N:
        raise RuntimeError("s_src has %d rows but the backward needs one per node (%d)" % (src_rows, N))
    shape = (E,) if s_dst.dim() == 1 else (heads, E)
    for t, n in ((alpha, "alpha"), (grad_alpha, "grad_alpha")):
        _check_input(t, n)
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise RuntimeError("%s must be float32 of shape %s, got %s %s" % (n, shape, t.dtype, tuple(t.shape)))
        if t.device != row_pointers.device:
            raise RuntimeError("%s must be on the device of row_pointers" % n)
    if row_pointers_t is None:
        perm = _perm_i32(perm, E, row_pointers.device)
    else:
        _transposed_i32(row_pointers_t, "row_pointers_t", N + 1, row_pointers.device)
        _transposed_i32(perm, "entry_index_t", E, row_pointers.device)
    grad_s_dst, grad_s_src = torch.empty_like(s_dst), torch.empty_like(s_src)
    grad_scores = torch.empty(shape, dtype=torch.float32, device=alpha.device)
    operands = (_ptr(alpha), _ptr(grad_alpha), _ptr(s_dst), _ptr(s_src), float(negative_slope), _ptr(row_pointers),
                _ptr(column_index))
    outputs = (E, heads, _ptr(grad_scores), _ptr(grad_s_dst), _ptr(grad_s_src),
               ctypes.c_void_p(torch.cuda.current_stream(alpha.device).cuda_stream))
    with _on_device(alpha.device):
        if row_pointers_t is None:
            check(lib().hcspmm_gat_attention_backward(*operands, _ptr(perm), N, *outputs))
        else:
            check(lib().hcspmm_gat_attention_backward_directed(*operands, _ptr(row_pointers_t), _ptr(perm), N, N, *outputs))
    return grad_s_dst, grad_s_src, grad_scores


def gat_attention_backward(alpha, grad_alpha, s_dst, s_src, row_pointers, column_index, perm, negative_slope=0.2):
    """Backward of gat_attention on a square, pattern-symmetric graph -> (grad_s_dst, grad_s_src, grad_scores), shaped as
    s_dst, s_src and alpha; grad_scores is the gradient of z = s_dst[row] + s_src[col].  perm is transpose_permutation's
    (int64 as it returns it, or an int32 copy; the kernel reads int32).  Two launches (hcspmm_gat_attention_backward)."""
    return _gat_attention_backward(alpha, grad_alpha, s_dst, s_src, row_pointers, column_index, None, perm, negative_slope)


def _transposed_i32(t, name, n, device):
    _check_input(t, name)
    if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n:
        raise RuntimeError("%s must be an int32 tensor of %d elements, got %s %s" % (name, n, t.dtype, tuple(t.shape)))
    if t.device != device:
        raise RuntimeError("%s must be on the device of row_pointers" % name)
    return t


def gat_attention_backward_directed(alpha, grad_alpha, s_dst, s_src, row_pointers, column_index, row_pointers_t, entry_index_t,
                                    negative_slope=0.2):
    """gat_attention_backward on any square graph: (row_pointers_t, entry_index_t) are transpose_graph's, and grad_s_src sums
    over the rows of A^T (hcspmm_gat_attention_backward_directed).  With (row_pointers, perm as int32) of a pattern-symmetric
    graph it returns gat_attention_backward's bits."""
    return _gat_attention_backward(alpha, grad_alpha, s_dst, s_src, row_pointers, column_index, row_pointers_t, entry_index_t,
                                   negative_slope)


def _gatv2_operands(H_dst, H_src, att, row_pointers, column_index):
    """-> (N, E, D, heads) of a GATv2 call: H_dst [N, D] and H_src [src_rows, D] float32 views with unit inner stride, att
    [heads, Dh] (or [Dh] for one head) contiguous, D = heads * Dh, Dh % 4 == 0"""
    _check_graph(row_pointers, column_index)
    _check_view(H_dst, "H_dst", torch.float32)
    _check_view(H_src, "H_src", torch.float32)
    _check_input(att, "att")
    if att.dtype != torch.float32 or att.dim() not in (1, 2) or att.numel() == 0:
        raise RuntimeError("att must be a float32 [Dh] or [heads, Dh] tensor, got %s %s" % (att.dtype, tuple(att.shape)))
    N, E, D = row_pointers.numel() - 1, column_index.numel(), H_dst.size(1)
    heads = 1 if att.dim() == 1 else att.size(0)
    if H_dst.size(0) != N:
        raise RuntimeError("H_dst has %d rows but the graph has %d nodes" % (H_dst.size(0), N))
    if H_src.size(1) != D:
        raise RuntimeError("H_src has %d columns but H_dst has %d" % (H_src.size(1), D))
    if att.numel() != D:
        raise RuntimeError("att has %d elements but H_dst has %d columns" % (att.numel(), D))
    if H_src.device != H_dst.device or att.device != H_dst.device or row_pointers.device != H_dst.device:
        raise RuntimeError("H_src, att and the graph must be on the device of H_dst")
    return N, E, D, heads  # (Dh % 4 and the slope are the library's to refuse: HCSPMM_EINVAL)


def gatv2_scores(H_dst, H_src, att, row_pointers, column_index, negative_slope=0.2):
    """GATv2 attention logits -> float32 [heads, E] ([E] for a 1-D att):
    out[h, e] = sum_k att[h, k] * LeakyReLU(H_dst[row(e), h*Dh + k] + H_src[column_index[e], h*Dh + k]), all heads in one
    launch (include/hcspmm.h hcspmm_gatv2_scores).  H_dst [N, D] and H_src [src_rows, D] are float32 2-D views with unit
    inner stride (the halves of one [N, 2 D] projection need no copy), att [heads, Dh] contiguous, D = heads * Dh,
    Dh % 4 == 0.  H_src may have any number of rows (a row block); column ids are trusted to be below it.  edge_softmax of
    the result is the attention; each head is bit for bit the single-head call on its column slice."""
    N, E, D, heads = _gatv2_operands(H_dst, H_src, att, row_pointers, column_index)
    out = torch.empty((E,) if att.dim() == 1 else (heads, E), dtype=torch.float32, device=H_dst.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(H_dst.device).cuda_stream)
    with _on_device(H_dst.device):
        check(lib().hcspmm_gatv2_scores(_ptr(H_dst), H_dst.stride(0), _ptr(H_src), H_src.size(0), H_src.stride(0), _ptr(att),
                                        float(negative_slope), _ptr(out), _ptr(row_pointers), _ptr(column_index), N, E, D,
                                        heads, stream))
    return out


def _gatv2_scores_backward(grad_logits, H_dst, H_src, att, row_pointers, column_index, row_pointers_t, column_index_t, perm,
                           negative_slope):
    """row_pointers_t None: the pattern-symmetric form (perm = transpose_permutation's); else the directed form (A^T's arrays,
    perm = entry_index_t)"""
    N, E, D, heads = _gatv2_operands(H_dst, H_src, att, row_pointers, column_index)
    if H_src.size(0) != N:
        raise RuntimeError("H_src has %d rows but the backward needs one per node (%d)" % (H_src.size(0), N))
    shape = (E,) if att.dim() == 1 else (heads, E)
    _check_input(grad_logits, "grad_logits")
    if grad_logits.dtype != torch.float32 or tuple(grad_logits.shape) != shape:
        raise RuntimeError("grad_logits must be float32 of shape %s, got %s %s" % (shape, grad_logits.dtype, tuple(grad_logits.shape)))
    if grad_logits.device != H_dst.device:
        raise RuntimeError("grad_logits must be on the device of H_dst")
    if row_pointers_t is None:
        perm = _perm_i32(perm, E, row_pointers.device)
    else:
        _transposed_i32(row_pointers_t, "row_pointers_t", N + 1, row_pointers.device)
        _transposed_i32(column_index_t, "column_index_t", E, row_pointers.device)
        _transposed_i32(perm, "entry_index_t", E, row_pointers.device)
    L = lib()
    grad_dst = torch.empty((N, D), dtype=torch.float32, device=H_dst.device)
    grad_src = torch.empty((N, D), dtype=torch.float32, device=H_dst.device)
    grad_att = torch.empty_like(att)
    ws_bytes = int(L.hcspmm_gatv2_backward_workspace_bytes(N, E, D, heads))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=H_dst.device)
    operands = (_ptr(grad_logits), _ptr(H_dst), H_dst.stride(0), _ptr(H_src), H_src.stride(0), _ptr(att), float(negative_slope),
                _ptr(row_pointers), _ptr(column_index))
    outputs = (E, D, heads, _ptr(grad_dst), D, _ptr(grad_src), D, _ptr(grad_att), _ptr(ws), ws_bytes,
               ctypes.c_void_p(torch.cuda.current_stream(H_dst.device).cuda_stream))
    with _on_device(H_dst.device):
        if row_pointers_t is None:
            check(L.hcspmm_gatv2_scores_backward(*operands, _ptr(perm), N, *outputs))
        else:
            check(L.hcspmm_gatv2_scores_backward_directed(*operands, _ptr(row_pointers_t), _ptr(column_index_t), _ptr(perm), N, N,
                                                          *outputs))
    return grad_dst, grad_src, grad_att


def gatv2_scores_backward(grad_logits, H_dst, H_src, att, row_pointers, column_index, perm, negative_slope=0.2):
    """Backward of gatv2_scores on a square, pattern-symmetric graph -> (grad_H_dst, grad_H_src, grad_att), contiguous and
    shaped as H_dst, H_src and att.  grad_logits is float32 of gatv2_scores' shape; perm is transpose_permutation's (int64
    as it returns it, or an int32 copy; the kernel reads int32).  Three launches, no atomics: two calls give the same bits
    (hcspmm_gatv2_scores_backward; the workspace is allocated here)."""
    return _gatv2_scores_backward(grad_logits, H_dst, H_src, att, row_pointers, column_index, None, None, perm, negative_slope)


def gatv2_scores_backward_directed(grad_logits, H_dst, H_src, att, row_pointers, column_index, row_pointers_t, column_index_t,
                                   entry_index_t, negative_slope=0.2):
    """gatv2_scores_backward on any square graph: (row_pointers_t, column_index_t, entry_index_t) are transpose_graph's, and
    grad_H_src walks the rows of A^T (hcspmm_gatv2_scores_backward_directed).  With (row_pointers, column_index, perm as
    int32) of a pattern-symmetric graph it returns gatv2_scores_backward's bits."""
    return _gatv2_scores_backward(grad_logits, H_dst, H_src, att, row_pointers, column_index, row_pointers_t, column_index_t,
                                  entry_index_t, negative_slope)


def update(X, W):
    """X @ W for X [N, D] (fp32, contiguous) and W [D, H] (any strides: a transposed view needs no copy) through the
    library's streaming MFMA update kernel (hcspmm_dense_update) -- the layers' torch.mm(X, weights), which for N in the
    millions and D, H of a few dozen is a stream over X.  Returns None when the operands are not of that kind (caller: torch.mm)."""
    if not (X.is_cuda and W.is_cuda and X.dtype == W.dtype == torch.float32 and X.dim() == W.dim() == 2
            and X.size(1) == W.size(0) and X.is_contiguous() and X.size(0) > 0 and X.size(1) > 0 and W.size(1) > 0):
        return None
    out = torch.empty((X.size(0), W.size(1)), dtype=torch.float32, device=X.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(X.device).cuda_stream)
    with _on_device(X.device):
        check(lib().hcspmm_dense_update(_ptr(X), _ptr(W), W.stride(0), W.stride(1), _ptr(out), X.size(0), X.size(1), W.size(1), stream))
    return out


def weight_grad(A, B):
    """dW = A^T B for A [N, D], B [N, H] (fp32, unit inner stride): the weight gradient of the update GEMM in the
    layers' backward passes (reference: torch.mm(X.t(), d_out), GNN_model.py:79,101,...) through the split-K MFMA
    kernel of hcspmm_weight_grad.  Returns None when the shape is outside the kernel's range (caller: library GEMM)."""
    L = lib()
    if not (A.is_cuda and B.is_cuda and A.dtype == B.dtype == torch.float32 and A.dim() == B.dim() == 2
            and A.size(0) == B.size(0) and A.stride(1) == 1 and B.stride(1) == 1
            and A.stride(0) >= A.size(1) and B.stride(0) >= B.size(1)):  # (rows that overlap, e.g. an expanded row: not taken)
        return None
    N, D, H = A.size(0), A.size(1), B.size(1)
    ws_bytes = int(L.hcspmm_weight_grad_workspace(N, D, H))
    if ws_bytes == 0:
        return None
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=A.device)
    out = torch.empty((D, H), dtype=torch.float32, device=A.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
    with torch.cuda.device(A.device):
        check(L.hcspmm_weight_grad(_ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out), N, D, H, _ptr(ws), ws_bytes, stream))
    return out


# The reference's dim-specialised variants compute the same product (hybrid_all.cpp:223-308);
# forward_fixed32 silently truncated to 32 columns for D > 32 -- not reproduced.
forward_more = forward
forward_fixed32 = forward
forward_fixed64 = forward


def _fused(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
           weights, output=None):
    c = _graph_args(X, (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type), row_nzr)
    N, D = c.N, c.D
    if not weights.is_cuda or weights.dtype != torch.float32 or weights.dim() != 2 or weights.size(0) != D:
        raise RuntimeError("weights must be a CUDA float32 tensor of shape [embedding_dim, hidden_dim]")
    H = weights.size(1)
    if output is None:
        output = torch.empty((N, H), dtype=torch.float32, device=X.device)
    else:
        _check_input(output, "output")
        if output.dtype != torch.float32 or output.numel() != N * H:
            raise RuntimeError("output must be float32 with num_nodes*hidden_dim elements")
    out2 = torch.empty((N, D), dtype=torch.float32, device=X.device)
    with c:
        check(lib().hcspmm_forward_fused(_ptr(X), _ptr(output), _ptr(out2), _ptr(weights), weights.stride(0), weights.stride(1), H,
                                         *c.graph, *c.ws))
    return [output, out2]


def forward_fixed32_fused(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                          col_nzr, weights):
    """-> [(A*X)*weights, A*X]  (hybrid_all.cpp:310-339).  `weights` may be a transposed view."""
    return _fused(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
                  weights)


forward_fixed64_fused = forward_fixed32_fused
forward_GIN_final_fused = forward_fixed32_fused


def forward_final_fused(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                        col_nzr, weights, output):
    """-> [output (the caller's tensor, written in place), A*X]  (hybrid_all.cpp:405-435)."""
    return _fused(X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr,
                  weights, output)


forward_final_fused_64 = forward_final_fused

# hybrid_all.cpp:516-523: every backward* name is bound to the matching forward function.
backward = forward
backward_fixed32 = forward_fixed32
backward_fixed32_fused = forward_fixed32_fused
backward_final_fused = forward_final_fused
backward_fixed64 = forward_fixed64
backward_fixed64_fused = forward_fixed64_fused
backward_final_fused_64 = forward_final_fused_64
backward_GIN_final_fused = forward_GIN_final_fused


def loi_reorder(row_pointers, column_index, variant="new_direct", batch=0, list_cap=0, threads=0):
    """LOI layout reorder (LOI.cpp:660-805 + main's output order) -> (perm[N], group_sizes).
    variant "fast" = the relaxed parallel form (hcspmm_loi_reorder_fast: capped column-list walks, `batch` seeds per round,
    deterministic for a given (batch, list_cap) whatever `threads`; NOT the reference's permutation -- batch=1, list_cap=-1 is).
    variant "new" = reorder_plus_new (LOI.cpp:505-658, symmetric-graph form); "plus_direct" / "plus" = the windowed
    variants reorder_plus_direct / reorder_plus (LOI.cpp:286-484 / :98-284; defined for graphs of at least 50 rows
    without empty rows -- other inputs raise); a HCSPMM_LOI_* number is accepted as well."""
    L = lib()
    rp = _i32_host(row_pointers)
    col = _i32_host(column_index)
    N, E = rp.numel() - 1, col.numel()
    perm = torch.empty(N, dtype=torch.int32)
    gs = torch.empty(max(N, 1), dtype=torch.int32)
    ng = ctypes.c_int64(0)
    if variant == "fast":
        params = (ctypes.c_int32 * 4)(int(batch), int(list_cap), int(threads), 0)
        check(L.hcspmm_loi_reorder_fast(_ptr(rp), _ptr(col), N, E, ctypes.cast(params, ctypes.c_void_p), _ptr(perm), _ptr(gs),
                                        ctypes.byref(ng)))
        return perm, gs[:ng.value].clone()
    v = variant if isinstance(variant, int) else {"new_direct": 0, "new": 1, "plus_direct": 2, "plus": 3}[variant]
    check(L.hcspmm_loi_reorder_variant(_ptr(rp), _ptr(col), N, E, v, _ptr(perm), _ptr(gs), ctypes.byref(ng)))
    return perm, gs[:ng.value].clone()


def apply_permutation(row_pointers, column_index, perm):
    """Relabel a CSR graph with a LOI permutation -> (row_pointers', column_index')."""
    L = lib()
    rp = _i32_host(row_pointers)
    col = _i32_host(column_index)
    p = _i32_host(perm)
    N, E = rp.numel() - 1, col.numel()
    rp2 = torch.empty(N + 1, dtype=torch.int32)
    col2 = torch.empty(E, dtype=torch.int32)
    check(L.hcspmm_apply_permutation(_ptr(rp), _ptr(col), N, E, _ptr(p), _ptr(rp2), _ptr(col2)))
    return rp2, col2
