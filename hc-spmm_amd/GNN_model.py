"""GNN layers over the HCSPMM operators -- counterpart of the reference's GNN_model.py (class names
and call conventions kept so HC-SpMM_main.py-style drivers run unchanged).

Two layer families, each a torch.autograd.Function built by `_make_layer_function`:

  update-then-aggregate (GCN):   Y = A (X W)        dX = (A dY) W^T      dW = X^T (A dY)
  aggregate-then-update (GIN):   Y = (A X) W        dX = A (dY W^T)      dW = (A X)^T dY

The backward pass aggregates with A, not A^T, as the reference does (symmetric graphs;
GNN_model.py:98,120,181).  Which HCSPMM entry point each stage calls follows the reference:

  class                       forward                                   backward
  HCSPMMFunctionFirst         mm -> forward_fixed32          (:134-136)  forward_fixed32, mm, mm     (:150-160)
  HCSPMMFunctionFixed32       mm -> forward_fixed32          (:87-89)    forward_fixed32_fused(W^T)  (:98-101)
  HCSPMMFunctionFinal         mm -> forward                  (:110-111)  forward_final_fused(W^T, output) (:120-124)
  HCSPMMFunction              mm -> forward                  (:67-69)    forward, mm, mm             (:76-80)
  HCSPMMFunction_GINFirst     forward -> mm                  (:190-194)  mm, mm, forward             (:201-205)
  HCSPMMFunction_GINFixed32   forward_fixed32_fused(W)       (:169)      mm, mm, forward_fixed32     (:178-181)
  HCSPMMFunction_GINFinal     forward_GIN_final_fused(W)     (:215)      mm, mm, forward_fixed32     (:227-230)
  HCSPMMFunction_SAG          forward_fixed32                (:39)       forward                     (:54)
"""
import math
import time

import torch

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    def tqdm(x):
        return x

import HCSPMM

HYGNN = HCSPMM  # HC-SpMM_main.py:52 still calls the extension by its earlier name

N_GRAPH = 8  # row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr


def gen_test_tensor(X_prime):
    """Known-answer features: row i filled with the value i (reference GNN_model.py:13-23), so
    (A X)[r, :] = sum of r's neighbour ids -- exact in fp32."""
    n, d = X_prime.size(0), X_prime.size(1)
    return torch.arange(n, dtype=torch.float32, device=X_prime.device).unsqueeze(1).expand(n, d).contiguous()


def _weight_grad(kept, d):
    """dW = kept^T d  (reference: torch.mm(X.t(), d), GNN_model.py:79,101,124,160,181,205,230).  The product has a
    tiny output (dim x hidden) and K = number of nodes; the library GEMM torch.mm picks for that shape on MI355X
    runs a single output tile over the whole K (400-500 us at 233 K nodes, 40 % of a GCN epoch:
    profiles/r01/gnn_epoch_kernels.log).  Splitting K into 256 batches of a batched GEMM and summing the partial
    products is the same arithmetic in a fixed order, 8x faster (profiles/r01/weight_grad_timing.log) and closer to
    the fp64 product."""
    n, G = kept.size(0), 256
    if n >= 4096 and hasattr(HCSPMM, "weight_grad"):  # native split-K MFMA kernel (include/hcspmm.h hcspmm_weight_grad)
        out = HCSPMM.weight_grad(kept, d)
        if out is not None:
            return out
    if n < 64 * G or not (kept.is_contiguous() and d.is_contiguous()):
        return torch.mm(kept.transpose(0, 1), d)
    m = (n // G) * G
    out = torch.bmm(kept[:m].view(G, m // G, kept.size(1)).transpose(1, 2), d[:m].view(G, m // G, d.size(1))).sum(0)
    if m < n:
        out = out + torch.mm(kept[m:].transpose(0, 1), d[m:])
    return out


def _mm(X, W):
    """X @ W (reference: torch.mm(X, weights) / torch.mm(d, weights.transpose(0, 1)), GNN_model.py:67,76,87,110,134,150,178,194,
    201,215,227).  N is in the millions and the widths a few dozen, so the product is one pass over X: the library's own update
    kernel (HCSPMM.update: W staged in LDS, 16-byte loads, fp32 MFMA) streams it at twice the rate of the library GEMM torch.mm
    picks for such shapes on MI355X (profiles/r04/gnn_epoch_kernels.log)."""
    if X.size(0) >= 4096 and hasattr(HCSPMM, "update"):
        out = HCSPMM.update(X.contiguous(), W)
        if out is not None:
            return out
    return torch.mm(X, W)


def _make_layer_function(name, aggregate_first, fwd_agg, bwd_agg, fwd_fused=None, bwd_fused=None, takes_output=False):
    """Build one autograd Function.  fwd_agg / bwd_agg name the HCSPMM A*X entry points; *_fused,
    when given, name the fused aggregate+update entry point used instead of (A*X then mm)."""

    def forward(ctx, X, weights, *rest):
        graph, extra = rest[:N_GRAPH], rest[N_GRAPH:]
        if aggregate_first:
            if fwd_fused is not None:
                out, agg = getattr(HCSPMM, fwd_fused)(X, *graph, weights)[:2]
            else:
                agg = getattr(HCSPMM, fwd_agg)(X, *graph)[0]
                out = _mm(agg, weights)
            ctx.save_for_backward(agg, weights, *graph)
        else:
            out = getattr(HCSPMM, fwd_agg)(_mm(X, weights), *graph)[0]
            ctx.save_for_backward(X, weights, *graph, *extra)
        return out

    def backward(ctx, d_out):
        saved = ctx.saved_tensors
        kept, weights, graph, extra = saved[0], saved[1], saved[2:2 + N_GRAPH], saved[2 + N_GRAPH:]
        d_out = d_out.contiguous()
        # (the input features of a first layer need no gradient: the reference computes one anyway -- at 4.86 M x 96 that product
        # alone was 6 % of a GCN epoch)
        need_dx = ctx.needs_input_grad[0]
        if aggregate_first:  # kept = A X
            d_w = _weight_grad(kept, d_out)
            d_x = getattr(HCSPMM, bwd_agg)(_mm(d_out, weights.transpose(0, 1)), *graph)[0] if need_dx else None
        else:  # kept = X
            if bwd_fused is not None:
                d_x, d_agg = getattr(HCSPMM, bwd_fused)(d_out, *graph, weights.transpose(0, 1), *extra)[:2]
            else:
                d_agg = getattr(HCSPMM, bwd_agg)(d_out, *graph)[0]
                d_x = _mm(d_agg, weights.transpose(0, 1)) if need_dx else None
            d_w = _weight_grad(kept, d_agg)
        return (d_x, d_w) + (None,) * (N_GRAPH + (1 if takes_output else 0))

    return type(name, (torch.autograd.Function,), {"forward": staticmethod(forward), "backward": staticmethod(backward),
                                                   "__doc__": "see module docstring"})


HCSPMMFunction = _make_layer_function("HCSPMMFunction", False, "forward", "forward")
HCSPMMFunctionFirst = _make_layer_function("HCSPMMFunctionFirst", False, "forward_fixed32", "forward_fixed32")
HCSPMMFunctionFixed32 = _make_layer_function("HCSPMMFunctionFixed32", False, "forward_fixed32", None,
                                             bwd_fused="forward_fixed32_fused")
HCSPMMFunctionFinal = _make_layer_function("HCSPMMFunctionFinal", False, "forward", None,
                                           bwd_fused="forward_final_fused", takes_output=True)
HCSPMMFunction_GINFirst = _make_layer_function("HCSPMMFunction_GINFirst", True, "forward", "forward")
HCSPMMFunction_GINFixed32 = _make_layer_function("HCSPMMFunction_GINFixed32", True, None, "forward_fixed32",
                                                 fwd_fused="forward_fixed32_fused")
HCSPMMFunction_GINFinal = _make_layer_function("HCSPMMFunction_GINFinal", True, None, "forward_fixed32",
                                               fwd_fused="forward_GIN_final_fused")


class HCSPMMFunction_SAG(torch.autograd.Function):
    """Bare aggregation A*X (the --single_kernel path, reference GNN_model.py:26-57)."""

    @staticmethod
    def forward(ctx, X, *graph):
        ctx.save_for_backward(*graph)
        return HCSPMM.forward_fixed32(X, *graph)[0]

    @staticmethod
    def backward(ctx, d_out):
        return (HCSPMM.forward(d_out.contiguous(), *ctx.saved_tensors)[0],) + (None,) * N_GRAPH


class SAG(torch.nn.Module):
    """Holds the graph tensors and times the aggregation kernel (reference GNN_model.py:236-262)."""

    def __init__(self, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                 col_nzr):
        super().__init__()
        self.graph = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                      col_nzr)
        (self.row_pointers, self.column_index, self.blockPartition, self.edgeToColumn, self.edgeToRow,
         self.hybrid_type, self.row_nzr, self.col_nzr) = self.graph

    def forward(self, X):
        return HCSPMMFunction_SAG.apply(X, *self.graph)

    def profile(self, X, num_rounds=200):
        torch.cuda.synchronize()
        start = time.perf_counter()
        for _ in tqdm(range(num_rounds)):
            HCSPMMFunction_SAG.apply(X, *self.graph)
        torch.cuda.synchronize()
        dur = time.perf_counter() - start
        print("=> SAG profiling avg (ms): {:.3f}".format(dur * 1e3 / num_rounds))
        print()
        return dur * 1e3 / num_rounds


class HCSPMMFunction_Weighted(torch.autograd.Function):
    """Edge-weighted aggregation A_w X (HCSPMM.forward_weighted).  Backward: dX = A_w^T dY, which for a pattern-symmetric
    graph is forward_weighted on the same graph and plan with values_t = values[perm] (HCSPMM.transpose_permutation).  The
    gradient with respect to the values is an SDDMM this library does not have yet."""

    @staticmethod
    def forward(ctx, X, values, values_t, *graph):
        if values.requires_grad:
            raise NotImplementedError("HCSPMM: the gradient with respect to the edge values (an SDDMM) is not implemented; "
                                      "pass values that do not require grad")
        ctx.save_for_backward(values_t, *graph)
        return HCSPMM.forward_weighted(X.contiguous(), values, *graph)[0]

    @staticmethod
    def backward(ctx, d_out):
        values_t, *graph = ctx.saved_tensors
        d_x = HCSPMM.forward_weighted(d_out.contiguous(), values_t, *graph)[0] if ctx.needs_input_grad[0] else None
        return (d_x, None, None) + (None,) * N_GRAPH


class _Update(torch.autograd.Function):
    """X W with the library's update and weight-gradient kernels (_mm / _weight_grad) on both passes."""

    @staticmethod
    def forward(ctx, X, W):
        X = X.contiguous()
        ctx.save_for_backward(X, W)
        return _mm(X, W)

    @staticmethod
    def backward(ctx, d_out):
        X, W = ctx.saved_tensors
        d_out = d_out.contiguous()
        d_x = _mm(d_out, W.transpose(0, 1)) if ctx.needs_input_grad[0] else None
        d_w = _weight_grad(X, d_out) if ctx.needs_input_grad[1] else None
        return d_x, d_w


_TRANSPOSED = {}  # (row_pointers, column_index) pointers and sizes -> (weak refs, perm): the host pass runs once per graph


def transpose_permutation(row_pointers, column_index):
    """HCSPMM.transpose_permutation, cached per graph tensor pair."""
    import weakref
    key = (row_pointers.data_ptr(), column_index.data_ptr(), row_pointers.numel(), column_index.numel())
    hit = _TRANSPOSED.get(key)
    if hit is not None and hit[0]() is row_pointers and hit[1]() is column_index:
        return hit[2]
    try:
        perm = HCSPMM.transpose_permutation(row_pointers, column_index)
    except RuntimeError as e:
        raise RuntimeError("HCSPMM: the edge-weighted backward needs a graph whose sparsity pattern is symmetric (A_w^T is "
                           "then A's pattern with permuted values); this one is not") from e
    for k in [k for k, v in _TRANSPOSED.items() if v[0]() is None or v[1]() is None]:
        del _TRANSPOSED[k]
    _TRANSPOSED[key] = (weakref.ref(row_pointers), weakref.ref(column_index), perm)
    return perm


_TRANSPOSED_GRAPH = {}  # as _TRANSPOSED -> (weak refs, the nine tensors of transposed_graph)


def transposed_graph(graph):
    """A^T of a square graph, for the backward of message passing over a directed edge_index: the eight graph tensors of A^T
    -- HCSPMM.transpose_graph, then HCSPMM.preprocess on A^T, so A^T has its own windows, classification and plan and
    in-degree hubs are balanced like out-degree hubs -- plus entry_index_t (int32 [E]: the position in A of every entry of
    A^T).  Cached per (row_pointers, column_index) tensor pair; graph = the eight graph tensors of A."""
    import weakref
    row_pointers, column_index = graph[0], graph[1]
    key = (row_pointers.data_ptr(), column_index.data_ptr(), row_pointers.numel(), column_index.numel())
    hit = _TRANSPOSED_GRAPH.get(key)
    if hit is not None and hit[0]() is row_pointers and hit[1]() is column_index:
        return hit[2]
    n = row_pointers.numel() - 1
    try:
        rp_t, col_t, eid_t = HCSPMM.transpose_graph(row_pointers, column_index)
    except RuntimeError as e:
        raise RuntimeError("HCSPMM: transposed_graph needs a square graph whose rows hold strictly ascending column ids "
                           "below the number of nodes (%d)" % n) from e
    out = (rp_t, col_t) + tuple(HCSPMM.preprocess(col_t, rp_t, n, col_t.numel(), (n + 15) // 16)) + (eid_t,)
    for k in [k for k, v in _TRANSPOSED_GRAPH.items() if v[0]() is None or v[1]() is None]:
        del _TRANSPOSED_GRAPH[k]
    _TRANSPOSED_GRAPH[key] = (weakref.ref(row_pointers), weakref.ref(column_index), out)
    return out


_SAMPLE_ROW_POINTERS = {}  # (row_pointers pointer and size, fanout) -> (weak ref, row_pointers_s): one scan per (graph, fanout)


def sampled_graph(graph, fanout, seed):
    """A fanout-limited random neighbourhood of every node (GraphSAGE's; redraw it every epoch with seed = the epoch) ->
    (graph_s, entry_index_s): graph_s = the eight graph tensors of the sample (HCSPMM.sample_neighbors, then
    HCSPMM.plan_free_graph: every entry point takes its plan-free sparse-row path), entry_index_s = int32 [E_s], the position in
    A of every kept entry (edge values of A travel as values[entry_index_s]).  A sample is a directed graph: its transpose is
    built on the device as well (HCSPMM.transpose_graph_device, plan_free_graph) and entered where transposed_graph looks, so
    every directed=True layer and function works on graph_s as it stands and nothing is copied to the host.  row_pointers_s
    depends on the graph and the fanout only and is made once for them; graph = the eight graph tensors of A."""
    import weakref
    row_pointers, column_index = graph[0], graph[1]
    key = (row_pointers.data_ptr(), row_pointers.numel(), int(fanout))
    hit = _SAMPLE_ROW_POINTERS.get(key)
    if hit is None or hit[0]() is not row_pointers:
        for k in [k for k, v in _SAMPLE_ROW_POINTERS.items() if v[0]() is None]:
            del _SAMPLE_ROW_POINTERS[k]
        hit = _SAMPLE_ROW_POINTERS[key] = (weakref.ref(row_pointers), HCSPMM.sample_row_pointers(row_pointers, int(fanout)))
    rp_s, col_s, eid_s = HCSPMM.sample_neighbors(row_pointers, column_index, int(fanout), int(seed), hit[1])
    graph_s = tuple(HCSPMM.plan_free_graph(rp_s, col_s))
    rp_t, col_t, eid_t = HCSPMM.transpose_graph_device(rp_s, col_s)
    for k in [k for k, v in _TRANSPOSED_GRAPH.items() if v[0]() is None or v[1]() is None]:
        del _TRANSPOSED_GRAPH[k]
    _TRANSPOSED_GRAPH[(rp_s.data_ptr(), col_s.data_ptr(), rp_s.numel(), col_s.numel())] = (
        weakref.ref(rp_s), weakref.ref(col_s), tuple(HCSPMM.plan_free_graph(rp_t, col_t)) + (eid_t,))
    return graph_s, eid_s


class EdgeWeightedAggregateDirected(torch.autograd.Function):
    """A_w X on any square graph, edge_weight [E] or [heads, E]: the forward is EdgeWeightedAggregate(Heads)'s;
    dX = A_w^T dY = HCSPMM.forward_weighted_indexed(dY, w, entry_index_t) on A^T's graph tensors and plan (the values are read
    in place through the index, no permuted copy) and dw = HCSPMM.sddmm(_heads)(dY, X) on A.  tail = the eight graph tensors
    of A followed by transposed_graph's nine."""

    @staticmethod
    def forward(ctx, X, edge_weight, *tail):
        X = X.contiguous()
        edge_weight = edge_weight.contiguous()
        ctx.save_for_backward(X, edge_weight, *tail)
        fn = HCSPMM.forward_weighted if edge_weight.dim() == 1 else HCSPMM.forward_weighted_heads
        return fn(X, edge_weight, *tail[:N_GRAPH])[0]

    @staticmethod
    def backward(ctx, d_out):
        X, edge_weight, *tail = ctx.saved_tensors
        graph, graph_t, eid_t = tail[:N_GRAPH], tail[N_GRAPH:2 * N_GRAPH], tail[2 * N_GRAPH]
        d_out = d_out.contiguous()
        d_x = d_w = None
        if ctx.needs_input_grad[0]:
            d_x = HCSPMM.forward_weighted_indexed(d_out, edge_weight, eid_t, *graph_t)[0]
        if ctx.needs_input_grad[1]:
            d_w = (HCSPMM.sddmm(d_out, X, *graph) if edge_weight.dim() == 1
                   else HCSPMM.sddmm_heads(d_out, X, *graph, edge_weight.size(0)))
        return (d_x, d_w) + (None,) * len(tail)


def weighted_aggregate(X, edge_weight, graph, directed=False):
    """A_w X with autograd for X (graph = the eight graph tensors).  directed=True: the pattern need not be symmetric (the
    backward runs on transposed_graph(graph))."""
    if edge_weight.requires_grad:
        raise NotImplementedError("HCSPMM: the gradient with respect to the edge values (an SDDMM) is not implemented; "
                                  "pass values that do not require grad")
    if directed:
        return EdgeWeightedAggregateDirected.apply(X, edge_weight, *graph, *transposed_graph(graph))
    values_t = edge_weight.detach()[transpose_permutation(graph[0], graph[1])].contiguous()
    return HCSPMMFunction_Weighted.apply(X, edge_weight, values_t, *graph)


class HCSPMMFunction_WeightedFP8(HCSPMMFunction_Weighted):
    """A_w X with X stored in 8 bits for the forward: quantise X per row (HCSPMM.quantize_fp8), then aggregate the codes with
    values[e] * scale[col[e]] (HCSPMM.forward_weighted_fp8).  The backward is HCSPMMFunction_Weighted's, unchanged
    (straight-through: the quantiser counts as the identity), so dX is the fp32 layer's for the same dY."""

    @staticmethod
    def forward(ctx, X, values, values_t, *graph):
        if values.requires_grad:
            raise NotImplementedError("HCSPMM: the gradient with respect to the edge values (an SDDMM) is not implemented; "
                                      "pass values that do not require grad")
        ctx.save_for_backward(values_t, *graph)
        Xq, scale = HCSPMM.quantize_fp8(X.contiguous())
        return HCSPMM.forward_weighted_fp8(Xq, scale, values, *graph)[0]


class EdgeWeightedAggregateDirectedFP8(EdgeWeightedAggregateDirected):
    """HCSPMMFunction_WeightedFP8 on any square graph: EdgeWeightedAggregateDirected's backward (A^T's own graph tensors)."""

    @staticmethod
    def forward(ctx, X, edge_weight, *tail):
        X = X.contiguous()
        edge_weight = edge_weight.contiguous()
        ctx.save_for_backward(X, edge_weight, *tail)
        Xq, scale = HCSPMM.quantize_fp8(X)
        return HCSPMM.forward_weighted_fp8(Xq, scale, edge_weight, *tail[:N_GRAPH])[0]


def aggregate_fp8(X, edge_weight, graph, directed=False):
    """weighted_aggregate with 8-bit feature storage in the forward: A_w (scale * e4m3(X / scale)), one fp32 scale per row of
    X, accumulated in fp32.  The backward is weighted_aggregate's exact fp32 one.  X's width must be a multiple of 4."""
    if edge_weight.requires_grad:
        raise NotImplementedError("HCSPMM: the gradient with respect to the edge values (an SDDMM) is not implemented; "
                                  "pass values that do not require grad")
    if X.size(1) % 4 != 0:
        raise ValueError("aggregate_fp8 takes feature widths that are multiples of 4, got %d" % X.size(1))
    if directed:
        return EdgeWeightedAggregateDirectedFP8.apply(X, edge_weight, *graph, *transposed_graph(graph))
    values_t = edge_weight.detach()[transpose_permutation(graph[0], graph[1])].contiguous()
    return HCSPMMFunction_WeightedFP8.apply(X, edge_weight, values_t, *graph)


class _UpdateOfAggregateFP8(torch.autograd.Function):
    """agg8 W for agg8 = aggregate_fp8(X, ...), with the fp32 layer's weight gradient: dW = (A_w X)^T dY needs the fp32
    aggregate, which the 8-bit forward never computed -- the backward computes it (one forward_weighted) instead of keeping
    the quantised one.  d(agg8) = dY W^T goes on through aggregate_fp8's backward, so X, which is only read here, gets no
    gradient from this function."""

    @staticmethod
    def forward(ctx, agg8, W, X, edge_weight, *graph):
        ctx.save_for_backward(W, X, edge_weight, *graph)
        return _mm(agg8.contiguous(), W)

    @staticmethod
    def backward(ctx, d_out):
        W, X, edge_weight, *graph = ctx.saved_tensors
        d_out = d_out.contiguous()
        d_agg = _mm(d_out, W.transpose(0, 1)) if ctx.needs_input_grad[0] else None
        d_w = None
        if ctx.needs_input_grad[1]:
            d_w = _weight_grad(HCSPMM.forward_weighted(X.contiguous(), edge_weight.contiguous(), *graph)[0], d_out)
        return (d_agg, d_w, None, None) + (None,) * len(graph)


class EdgeWeightedAggregate(torch.autograd.Function):
    """A_w X with the gradient for both operands: dX = A_w^T dY = forward_weighted(dY, w[perm]) as in
    HCSPMMFunction_Weighted, and dw[e] = <dY[row(e)], X[col(e)]> = HCSPMM.sddmm(dY, X)."""

    @staticmethod
    def forward(ctx, X, edge_weight, perm, *graph):
        X = X.contiguous()
        edge_weight = edge_weight.contiguous()
        ctx.save_for_backward(X, edge_weight, perm, *graph)
        return HCSPMM.forward_weighted(X, edge_weight, *graph)[0]

    @staticmethod
    def backward(ctx, d_out):
        X, edge_weight, perm, *graph = ctx.saved_tensors
        d_out = d_out.contiguous()
        d_x = HCSPMM.forward_weighted(d_out, edge_weight[perm].contiguous(), *graph)[0] if ctx.needs_input_grad[0] else None
        d_w = HCSPMM.sddmm(d_out, X, *graph) if ctx.needs_input_grad[1] else None
        return (d_x, d_w, None) + (None,) * N_GRAPH


def edge_weighted_aggregate(X, edge_weight, graph, directed=False):
    """A_w X with autograd for X and edge_weight (float32 [E], aligned with column_index), e.g. learned or attention
    weights; graph = the eight graph tensors, whose pattern must be symmetric (the backward's A_w^T) unless directed=True:
    the backward then runs on transposed_graph(graph)."""
    if directed:
        return EdgeWeightedAggregateDirected.apply(X, edge_weight, *graph, *transposed_graph(graph))
    perm = transpose_permutation(graph[0], graph[1])
    return EdgeWeightedAggregate.apply(X, edge_weight, perm, *graph)


class EdgeWeightedAggregateHeads(torch.autograd.Function):
    """Multi-head A_w X: columns [h*Dh, (h+1)*Dh) of the result are A_{w[h]} X[:, h*Dh:(h+1)*Dh] for w [heads, E]
    (HCSPMM.forward_weighted_heads, one launch), with the gradient for both operands:
    dX = forward_weighted_heads(dY, w[:, perm]) and dw = HCSPMM.sddmm_heads(dY, X)."""

    @staticmethod
    def forward(ctx, X, edge_weight, perm, *graph):
        X = X.contiguous()
        edge_weight = edge_weight.contiguous()
        ctx.save_for_backward(X, edge_weight, perm, *graph)
        return HCSPMM.forward_weighted_heads(X, edge_weight, *graph)[0]

    @staticmethod
    def backward(ctx, d_out):
        X, edge_weight, perm, *graph = ctx.saved_tensors
        d_out = d_out.contiguous()
        d_x = d_w = None
        if ctx.needs_input_grad[0]:
            d_x = HCSPMM.forward_weighted_heads(d_out, edge_weight[:, perm].contiguous(), *graph)[0]
        if ctx.needs_input_grad[1]:
            d_w = HCSPMM.sddmm_heads(d_out, X, *graph, edge_weight.size(0))
        return (d_x, d_w, None) + (None,) * N_GRAPH


def edge_weighted_aggregate_heads(X, edge_weight, graph, directed=False):
    """Multi-head A_w X with autograd for X [N, heads*Dh] and edge_weight [heads, E] (float32, Dh % 4 == 0); graph = the
    eight graph tensors, whose pattern must be symmetric (the backward's A_w^T) unless directed=True: the backward then
    runs on transposed_graph(graph)."""
    if directed:
        return EdgeWeightedAggregateDirected.apply(X, edge_weight, *graph, *transposed_graph(graph))
    perm = transpose_permutation(graph[0], graph[1])
    return EdgeWeightedAggregateHeads.apply(X, edge_weight, perm, *graph)


class EdgeSoftmax(torch.autograd.Function):
    """Softmax of logits ([E] or [heads, E], float32) over each row's stored entries (HCSPMM.edge_softmax), with its
    backward (HCSPMM.edge_softmax_backward)."""

    @staticmethod
    def forward(ctx, logits, row_pointers):
        alpha = HCSPMM.edge_softmax(logits.contiguous(), row_pointers)
        ctx.save_for_backward(alpha, row_pointers)
        return alpha

    @staticmethod
    def backward(ctx, d_alpha):
        alpha, row_pointers = ctx.saved_tensors
        return HCSPMM.edge_softmax_backward(alpha, d_alpha.contiguous(), row_pointers), None


_PERM_I32 = {}  # id of a cached int64 perm -> (weak ref, int32 copy): the attention backward's kernel reads int32


def transpose_permutation_i32(row_pointers, column_index):
    """transpose_permutation as an int32 device tensor, cached per graph tensor pair (raises for an asymmetric pattern)."""
    import weakref
    perm = transpose_permutation(row_pointers, column_index)
    hit = _PERM_I32.get(id(perm))
    if hit is not None and hit[0]() is perm:
        return hit[1]
    for k in [k for k, v in _PERM_I32.items() if v[0]() is None]:
        del _PERM_I32[k]
    perm32 = perm.to(torch.int32)
    _PERM_I32[id(perm)] = (weakref.ref(perm), perm32)
    return perm32


class GATAttention(torch.autograd.Function):
    """GAT attention weights alpha [heads, E] = softmax over each row of LeakyReLU(s_dst[row] + s_src[col]) from node-major
    scores s_dst, s_src [N, heads] (HCSPMM.gat_attention, one launch), with the gradients of both scores
    (HCSPMM.gat_attention_backward, two launches; perm32 = transpose_permutation_i32 of the graph)."""

    @staticmethod
    def forward(ctx, s_dst, s_src, negative_slope, perm32, row_pointers, column_index):
        s_dst, s_src = s_dst.contiguous(), s_src.contiguous()
        alpha = HCSPMM.gat_attention(s_dst, s_src, row_pointers, column_index, negative_slope)
        ctx.negative_slope = negative_slope
        ctx.save_for_backward(alpha, s_dst, s_src, perm32, row_pointers, column_index)
        return alpha

    @staticmethod
    def backward(ctx, d_alpha):
        alpha, s_dst, s_src, perm32, row_pointers, column_index = ctx.saved_tensors
        d_dst, d_src, _ = HCSPMM.gat_attention_backward(alpha, d_alpha.contiguous(), s_dst, s_src, row_pointers, column_index,
                                                        perm32, ctx.negative_slope)
        return d_dst, d_src, None, None, None, None


class GATAttentionDirected(torch.autograd.Function):
    """GATAttention on any square graph: the backward's column side walks A^T (HCSPMM.gat_attention_backward_directed with
    transposed_graph's row_pointers_t and entry_index_t)."""

    @staticmethod
    def forward(ctx, s_dst, s_src, negative_slope, row_pointers, column_index, row_pointers_t, entry_index_t):
        s_dst, s_src = s_dst.contiguous(), s_src.contiguous()
        alpha = HCSPMM.gat_attention(s_dst, s_src, row_pointers, column_index, negative_slope)
        ctx.negative_slope = negative_slope
        ctx.save_for_backward(alpha, s_dst, s_src, row_pointers, column_index, row_pointers_t, entry_index_t)
        return alpha

    @staticmethod
    def backward(ctx, d_alpha):
        alpha, s_dst, s_src, row_pointers, column_index, row_pointers_t, entry_index_t = ctx.saved_tensors
        d_dst, d_src, _ = HCSPMM.gat_attention_backward_directed(alpha, d_alpha.contiguous(), s_dst, s_src, row_pointers,
                                                                 column_index, row_pointers_t, entry_index_t, ctx.negative_slope)
        return d_dst, d_src, None, None, None, None, None


def gat_attention(s_dst, s_src, graph, negative_slope=0.2, directed=False):
    """GAT attention weights [heads, E] ([E] for 1-D scores) with autograd for both node-major scores; graph = the eight
    graph tensors, whose pattern must be symmetric (checked before any launch: the backward sums over A^T) unless
    directed=True: the backward then walks transposed_graph(graph)."""
    if directed:
        gt = transposed_graph(graph)
        return GATAttentionDirected.apply(s_dst, s_src, float(negative_slope), graph[0], graph[1], gt[0], gt[N_GRAPH])
    perm32 = transpose_permutation_i32(graph[0], graph[1])
    return GATAttention.apply(s_dst, s_src, float(negative_slope), perm32, graph[0], graph[1])


class GATv2Scores(torch.autograd.Function):
    """GATv2 attention logits [heads, E]: l[h, e] = sum_k att[h, k] * LeakyReLU(H_dst[row(e), h*Dh + k] + H_src[col(e), h*Dh + k])
    from node features H_dst, H_src [N, heads * Dh] (float32 views with unit inner stride: the halves of one projection need
    no copy) and att [heads, Dh] (HCSPMM.gatv2_scores, one launch), with the gradients of all three
    (HCSPMM.gatv2_scores_backward, three launches; perm32 = transpose_permutation_i32 of the graph).  No [E, D] tensor in
    either pass."""

    @staticmethod
    def forward(ctx, H_dst, H_src, att, negative_slope, perm32, row_pointers, column_index):
        att = att.contiguous()
        logits = HCSPMM.gatv2_scores(H_dst, H_src, att, row_pointers, column_index, negative_slope)
        ctx.negative_slope = negative_slope
        ctx.save_for_backward(H_dst, H_src, att, perm32, row_pointers, column_index)
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        H_dst, H_src, att, perm32, row_pointers, column_index = ctx.saved_tensors
        d_dst, d_src, d_att = HCSPMM.gatv2_scores_backward(d_logits.contiguous(), H_dst, H_src, att, row_pointers, column_index,
                                                           perm32, ctx.negative_slope)
        return d_dst, d_src, d_att, None, None, None, None


class GATv2ScoresDirected(torch.autograd.Function):
    """GATv2Scores on any square graph: the backward's grad_H_src walks A^T (HCSPMM.gatv2_scores_backward_directed with
    transposed_graph's row_pointers_t, column_index_t and entry_index_t)."""

    @staticmethod
    def forward(ctx, H_dst, H_src, att, negative_slope, row_pointers, column_index, row_pointers_t, column_index_t, entry_index_t):
        att = att.contiguous()
        logits = HCSPMM.gatv2_scores(H_dst, H_src, att, row_pointers, column_index, negative_slope)
        ctx.negative_slope = negative_slope
        ctx.save_for_backward(H_dst, H_src, att, row_pointers, column_index, row_pointers_t, column_index_t, entry_index_t)
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        H_dst, H_src, att, row_pointers, column_index, row_pointers_t, column_index_t, entry_index_t = ctx.saved_tensors
        d_dst, d_src, d_att = HCSPMM.gatv2_scores_backward_directed(d_logits.contiguous(), H_dst, H_src, att, row_pointers,
                                                                    column_index, row_pointers_t, column_index_t, entry_index_t,
                                                                    ctx.negative_slope)
        return (d_dst, d_src, d_att) + (None,) * 6


def gatv2_attention(H_dst, H_src, att, graph, negative_slope=0.2, directed=False):
    """GATv2 attention weights alpha [heads, E] = edge softmax of GATv2Scores' logits, with autograd for H_dst, H_src and att;
    graph = the eight graph tensors, whose pattern must be symmetric (checked before any launch: the backward sums over
    A^T) unless directed=True: the backward then walks transposed_graph(graph)."""
    if directed:
        gt = transposed_graph(graph)
        logits = GATv2ScoresDirected.apply(H_dst, H_src, att, float(negative_slope), graph[0], graph[1], gt[0], gt[1], gt[N_GRAPH])
        return EdgeSoftmax.apply(logits, graph[0])
    perm32 = transpose_permutation_i32(graph[0], graph[1])
    logits = GATv2Scores.apply(H_dst, H_src, att, float(negative_slope), perm32, graph[0], graph[1])
    return EdgeSoftmax.apply(logits, graph[0])


class ExtremumAggregate(torch.autograd.Function):
    """Max or min of each row's neighbour features (HCSPMM.forward_max / forward_min, with the argmax) and its gradient
    dX[j][d] = sum of dY[i][d] over the entries (i, j) that won (i, d) (HCSPMM.forward_extremum_backward: A^T walked on
    the same plan, deterministic; perm32 = transpose_permutation_i32 of the graph)."""

    @staticmethod
    def forward(ctx, X, reduce, perm32, *graph):
        fn = HCSPMM.forward_max if reduce == "max" else HCSPMM.forward_min
        Z, arg = fn(X.contiguous(), *graph, True)
        ctx.save_for_backward(arg, perm32, *graph)
        ctx.mark_non_differentiable(arg)
        return Z

    @staticmethod
    def backward(ctx, d_out):
        arg, perm32, *graph = ctx.saved_tensors
        d_x = HCSPMM.forward_extremum_backward(d_out.contiguous(), arg, perm32, *graph) if ctx.needs_input_grad[0] else None
        return (d_x, None, None) + (None,) * N_GRAPH


class ExtremumAggregateDirected(torch.autograd.Function):
    """ExtremumAggregate on any square graph: the forward on A, the backward (HCSPMM.forward_extremum_backward, which walks
    whatever graph it is handed) on A^T's graph tensors and plan with entry_index_t in the place of the permutation.
    tail = the eight graph tensors of A followed by transposed_graph's nine."""

    @staticmethod
    def forward(ctx, X, reduce, *tail):
        fn = HCSPMM.forward_max if reduce == "max" else HCSPMM.forward_min
        Z, arg = fn(X.contiguous(), *tail[:N_GRAPH], True)
        ctx.save_for_backward(arg, *tail[N_GRAPH:])
        ctx.mark_non_differentiable(arg)
        return Z

    @staticmethod
    def backward(ctx, d_out):
        arg, *rest = ctx.saved_tensors
        graph_t, eid_t = rest[:N_GRAPH], rest[N_GRAPH]
        d_x = HCSPMM.forward_extremum_backward(d_out.contiguous(), arg, eid_t, *graph_t) if ctx.needs_input_grad[0] else None
        return (d_x, None) + (None,) * (2 * N_GRAPH + 1)


def extremum_aggregate(X, graph, reduce="max", directed=False):
    """max / min over each row's neighbours with autograd for X (float32 [N, D]); graph = the eight graph tensors, whose
    pattern must be symmetric (checked before any launch: the backward walks A^T) unless directed=True: the backward then
    runs on transposed_graph(graph).  Rows without entries give 0."""
    if reduce not in ("max", "min"):
        raise ValueError("reduce must be 'max' or 'min', got %r" % (reduce,))
    if directed:
        return ExtremumAggregateDirected.apply(X, reduce, *graph, *transposed_graph(graph))
    perm32 = transpose_permutation_i32(graph[0], graph[1])
    return ExtremumAggregate.apply(X, reduce, perm32, *graph)


_EDGE_ROWS = {}  # (row_pointers pointer and size) -> (weak ref, row of every stored entry as int64)


def edge_rows(row_pointers):
    """row(e) for every stored entry (int64, on the graph's device), cached per row_pointers tensor."""
    import weakref
    key = (row_pointers.data_ptr(), row_pointers.numel())
    hit = _EDGE_ROWS.get(key)
    if hit is not None and hit[0]() is row_pointers:
        return hit[1]
    n = row_pointers.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n, device=row_pointers.device), (row_pointers[1:] - row_pointers[:-1]).long())
    for k in [k for k, v in _EDGE_ROWS.items() if v[0]() is None]:
        del _EDGE_ROWS[k]
    _EDGE_ROWS[key] = (weakref.ref(row_pointers), rows)
    return rows


class _Conv(torch.nn.Module):
    """fixed: 1 = first layer, 0 = hidden layer, 2 = last layer (reference GNN_model.py:264-302)."""
    first_fn = hidden_fn = last_fn = None
    last_takes_output = False

    def __init__(self, input_dim, output_dim, fixed=0, directed=False):
        super().__init__()
        self.weights = torch.nn.Parameter(torch.randn(input_dim, output_dim))
        self.fixed = fixed
        self.directed = bool(directed)  # the edge_weight path only: the binary layer functions aggregate with A, as the reference
        # "fp8": the edge_weight path aggregates 8-bit codes of its input (aggregate_fp8: quantised forward, exact fp32 backward)
        self.feature_storage = "fp32"

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.weights.size(1))
        self.weights.data.uniform_(-stdv, stdv)

    aggregate_first = False

    def forward(self, X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                col_nzr, output, edge_weight=None):
        """edge_weight (float32 [E], aligned with column_index): aggregate with A_w (e.g. HCSPMM.edge_norm's "sym" / "mean"
        values) -- weighted aggregation + the update, no fused operators; None: the binary layer functions."""
        graph = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr)
        if self.feature_storage not in ("fp32", "fp8"):
            raise ValueError("feature_storage must be 'fp32' or 'fp8', got %r" % (self.feature_storage,))
        if self.feature_storage == "fp8":
            if edge_weight is None:
                raise ValueError("feature_storage = 'fp8' needs an edge_weight: the fused binary layer functions stay fp32")
            if self.aggregate_first:
                agg8 = aggregate_fp8(X, edge_weight, graph, self.directed)
                return _UpdateOfAggregateFP8.apply(agg8, self.weights, X, edge_weight, *graph)
            return aggregate_fp8(_Update.apply(X, self.weights), edge_weight, graph, self.directed)
        if edge_weight is not None:
            if self.aggregate_first:
                return _Update.apply(weighted_aggregate(X, edge_weight, graph, self.directed), self.weights)
            return weighted_aggregate(_Update.apply(X, self.weights), edge_weight, graph, self.directed)
        if self.fixed == 0:
            return self.hidden_fn.apply(X, self.weights, *graph)
        if self.fixed == 2:
            extra = (output,) if self.last_takes_output else ()
            return self.last_fn.apply(X, self.weights, *graph, *extra)
        return self.first_fn.apply(X, self.weights, *graph)


class GCNConv(_Conv):
    first_fn, hidden_fn, last_fn = HCSPMMFunctionFirst, HCSPMMFunctionFixed32, HCSPMMFunctionFinal
    last_takes_output = True


class GINConv(_Conv):
    first_fn, hidden_fn, last_fn = HCSPMMFunction_GINFirst, HCSPMMFunction_GINFixed32, HCSPMMFunction_GINFinal
    aggregate_first = True


class GATConv(torch.nn.Module):
    """Graph attention layer (GAT), `heads` heads averaged: per head k
        h_k = X W_k                                                       (the library's update, _Update)
        l_e = LeakyReLU(<a_dst_k, h_k[row(e)]> + <a_src_k, h_k[col(e)]>)  (row = destination, col = source)
        alpha_k = softmax of l over each row's entries;   out_k = A_alpha_k h_k   (edge_weighted_aggregate)
    -> mean_k out_k  [N, output_dim].  The per-node scores <a_dst_k, h_k> and <a_src_k, h_k> go node-major [N, heads] into
    gat_attention, which computes every head's logits and softmax in one launch and their backward in two (no per-entry
    torch op); the backward is autograd over these pieces.  _Conv's call signature, so that Net builds it; the attention
    weights are the edge values, so edge_weight is refused.  The pattern must be symmetric unless directed=True (message
    passing over a directed edge_index: the backward runs on transposed_graph).

    concat=True concatenates the heads instead -> [N, heads * output_dim] (the hidden layers of the GAT paper): one
    update X W_cat for all heads, both scores as one product H A_blk (A_blk block-diagonal [heads * output_dim, 2 heads]
    from a_dst / a_src; both products run on the library's update and weight-gradient kernels in both passes),
    gat_attention, and one multi-head aggregation (edge_weighted_aggregate_heads).  The kernels need output_dim % 4 == 0.
    The parameters are the same in both modes, so a state dict loads into either."""

    def __init__(self, input_dim, output_dim, fixed=0, heads=1, negative_slope=0.2, concat=False, directed=False):
        super().__init__()
        self.fixed, self.heads, self.negative_slope, self.concat = fixed, int(heads), float(negative_slope), bool(concat)
        self.directed = bool(directed)
        if self.concat and output_dim % 4 != 0:
            raise ValueError("GATConv(concat=True) needs output_dim (the width of one head) to be a multiple of 4, got %d"
                             % output_dim)
        self.weights = torch.nn.Parameter(torch.empty(self.heads, input_dim, output_dim))  # W_k = weights[k], contiguous
        self.a_src = torch.nn.Parameter(torch.empty(self.heads, output_dim))
        self.a_dst = torch.nn.Parameter(torch.empty(self.heads, output_dim))
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.weights.size(2))
        for p in (self.weights, self.a_src, self.a_dst):
            p.data.uniform_(-stdv, stdv)

    def forward(self, X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                col_nzr, output=None, edge_weight=None):
        if edge_weight is not None:
            raise ValueError("GATConv computes its edge values from the features: edge_weight is not accepted")
        graph = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr)
        if not self.directed:
            transpose_permutation_i32(row_pointers, column_index)  # an asymmetric pattern is refused before any launch (cached)
        if self.concat:
            return self._forward_concat(X, graph)
        hs = [_Update.apply(X, self.weights[k]) for k in range(self.heads)]
        s_dst = torch.stack([h @ self.a_dst[k] for k, h in enumerate(hs)], 1)  # [N, heads]
        s_src = torch.stack([h @ self.a_src[k] for k, h in enumerate(hs)], 1)
        alpha = gat_attention(s_dst, s_src, graph, self.negative_slope, self.directed)  # [heads, E]
        out = edge_weighted_aggregate(hs[0], alpha[0], graph, self.directed)
        for k in range(1, self.heads):
            out = out + edge_weighted_aggregate(hs[k], alpha[k], graph, self.directed)
        return out / self.heads if self.heads > 1 else out

    def _forward_concat(self, X, graph):
        heads, din, dout = self.weights.shape
        w_cat = self.weights.permute(1, 0, 2).reshape(din, heads * dout)  # column block k = W_k
        h = _Update.apply(X, w_cat)  # [N, heads * dout]
        a_blk = torch.cat([torch.block_diag(*self.a_dst.unsqueeze(2)), torch.block_diag(*self.a_src.unsqueeze(2))], 1)
        s = _Update.apply(h, a_blk)  # [N, 2 heads]: s_dst | s_src
        alpha = gat_attention(s[:, :heads], s[:, heads:], graph, self.negative_slope, self.directed)  # [heads, E]
        return edge_weighted_aggregate_heads(h, alpha, graph, self.directed)


class GATv2Conv(torch.nn.Module):
    """GATv2 layer (Brody et al., "How attentive are graph attention networks?"): the non-linearity sits inside the score,
        [H_src | H_dst] = X [W_src | W_dst]                  (one update, _Update; [N, 2 * heads * output_dim])
        l_k[e] = <att_k, LeakyReLU(H_dst_k[row(e)] + H_src_k[col(e)])>   (row = destination, col = source)
        alpha_k = softmax of l_k over each row's entries;   out_k = A_alpha_k H_src_k
    through gatv2_attention on the two halves of the projection (views, no copy) and one multi-head aggregation
    (edge_weighted_aggregate_heads).  concat=True returns the heads side by side [N, heads * output_dim], otherwise their
    mean [N, output_dim].  share_weights=True uses one projection for both roles (H_dst = H_src, [N, heads * output_dim]).
    No per-entry torch op and no [E, D] tensor in either pass.  The kernels need output_dim % 4 == 0.  _Conv's call
    signature, so that Net builds it; the attention weights are the edge values, so edge_weight is refused.  The pattern must
    be symmetric unless directed=True (the backward then runs on transposed_graph)."""

    def __init__(self, input_dim, output_dim, fixed=0, heads=1, negative_slope=0.2, concat=False, share_weights=False,
                 directed=False):
        super().__init__()
        self.fixed, self.heads, self.negative_slope = fixed, int(heads), float(negative_slope)
        self.directed = bool(directed)
        self.concat, self.share_weights, self.output_dim = bool(concat), bool(share_weights), int(output_dim)
        if self.heads < 1:
            raise ValueError("GATv2Conv needs heads >= 1, got %d" % self.heads)
        if output_dim < 4 or output_dim % 4 != 0:
            raise ValueError("GATv2Conv needs output_dim (the width of one head) to be a multiple of 4, got %d" % output_dim)
        width = self.heads * self.output_dim
        # column block 0 = W_src, block 1 = W_dst (absent with share_weights); within a block, head k's columns are contiguous
        self.weights = torch.nn.Parameter(torch.empty(input_dim, width if self.share_weights else 2 * width))
        self.att = torch.nn.Parameter(torch.empty(self.heads, self.output_dim))
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.output_dim)
        for p in (self.weights, self.att):
            p.data.uniform_(-stdv, stdv)

    def forward(self, X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                col_nzr, output=None, edge_weight=None):
        if edge_weight is not None:
            raise ValueError("GATv2Conv computes its edge values from the features: edge_weight is not accepted")
        graph = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr)
        if not self.directed:
            transpose_permutation_i32(row_pointers, column_index)  # an asymmetric pattern is refused before any launch (cached)
        width = self.heads * self.output_dim
        h = _Update.apply(X, self.weights)
        h_src = h[:, :width]
        h_dst = h_src if self.share_weights else h[:, width:]
        alpha = gatv2_attention(h_dst, h_src, self.att, graph, self.negative_slope, self.directed)  # [heads, E]
        out = edge_weighted_aggregate_heads(h_src, alpha, graph, self.directed)  # [N, heads * output_dim]
        if self.concat or self.heads == 1:
            return out
        return out.view(out.size(0), self.heads, self.output_dim).mean(1)


class SAGEConv(torch.nn.Module):
    """GraphSAGE layer:  out = X W_root + AGG(X) W_neigh, AGG over each row's neighbours:
      "max" / "min"  extremum_aggregate (GraphSAGE-pool without the pre-MLP, PyG aggr="max" / "min");
      "mean"         edge_weighted_aggregate with HCSPMM.edge_norm(..., "mean") values, computed once per graph.
    Both products run on _Update (the library's update and weight-gradient kernels).  _Conv's call signature, so that Net
    builds it; the aggregation is fixed by `aggr`, so edge_weight is refused.  The pattern must be symmetric unless
    directed=True (the backward then runs on transposed_graph)."""

    def __init__(self, input_dim, output_dim, fixed=0, aggr="max", directed=False):
        super().__init__()
        if aggr not in ("max", "min", "mean"):
            raise ValueError("SAGEConv aggr must be 'max', 'min' or 'mean', got %r" % (aggr,))
        self.fixed, self.aggr, self.directed = fixed, aggr, bool(directed)
        self.weights_root = torch.nn.Parameter(torch.empty(input_dim, output_dim))
        self.weights_neigh = torch.nn.Parameter(torch.empty(input_dim, output_dim))
        self._mean = None  # (row_pointers, column_index, values) of the last graph
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.weights_root.size(1))
        for p in (self.weights_root, self.weights_neigh):
            p.data.uniform_(-stdv, stdv)

    def _mean_values(self, row_pointers, column_index):
        m = self._mean
        if m is None or m[0] is not row_pointers or m[1] is not column_index:
            self._mean = m = (row_pointers, column_index, HCSPMM.edge_norm(row_pointers, column_index, "mean"))
        return m[2]

    def forward(self, X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                col_nzr, output=None, edge_weight=None):
        if edge_weight is not None:
            raise ValueError("SAGEConv aggregates with its own `aggr`: edge_weight is not accepted")
        graph = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr)
        if self.aggr == "mean":
            agg = edge_weighted_aggregate(X, self._mean_values(row_pointers, column_index), graph, self.directed)
        else:
            agg = extremum_aggregate(X, graph, self.aggr, self.directed)
        return _Update.apply(X, self.weights_root) + _Update.apply(agg, self.weights_neigh)


class MultiAggregate(torch.autograd.Function):
    """Sum, sum of squares, max and min of each row's neighbour features from ONE gather pass (HCSPMM.forward_multi) ->
    (Z_sum, Z_sumsq, Z_max, Z_min), with the gradient for X composed from existing launches on the graph the backward walks:
      dX = A^T [g_sum | g_sumsq] (one binary HCSPMM.forward over both, 2 D wide), the second half times 2 X,
         + HCSPMM.forward_extremum_backward(g_max, arg_max) + HCSPMM.forward_extremum_backward(g_min, arg_min).
    tail = the eight graph tensors of A, the eight of the graph the backward walks (A itself when the pattern is symmetric, else
    transposed_graph's) and the int32 index of its entries into A's (the transpose permutation, or entry_index_t)."""

    @staticmethod
    def forward(ctx, X, *tail):
        X = X.contiguous()
        z_sum, z_sumsq, z_max, z_min, arg_max, arg_min = HCSPMM.forward_multi(X, *tail[:N_GRAPH])
        ctx.save_for_backward(X, arg_max, arg_min, *tail[N_GRAPH:])
        ctx.set_materialize_grads(False)  # an aggregate the layer does not use costs no launch in the backward
        return z_sum, z_sumsq, z_max, z_min

    @staticmethod
    def backward(ctx, g_sum, g_sumsq, g_max, g_min):
        X, arg_max, arg_min, *rest = ctx.saved_tensors
        graph_b, index = rest[:N_GRAPH], rest[N_GRAPH]
        if not ctx.needs_input_grad[0]:
            return (None,) * (2 * N_GRAPH + 2)
        D = X.size(1)
        d_x = None
        if g_sum is not None and g_sumsq is not None:
            t = HCSPMM.forward(torch.cat((g_sum, g_sumsq), 1), *graph_b)[0]
            d_x = t[:, :D] + 2.0 * X * t[:, D:]
        elif g_sum is not None:
            d_x = HCSPMM.forward(g_sum.contiguous(), *graph_b)[0]
        elif g_sumsq is not None:
            d_x = 2.0 * X * HCSPMM.forward(g_sumsq.contiguous(), *graph_b)[0]
        for g, arg in ((g_max, arg_max), (g_min, arg_min)):
            if g is not None:
                d = HCSPMM.forward_extremum_backward(g.contiguous(), arg, index, *graph_b)
                d_x = d if d_x is None else d_x + d
        if d_x is None:
            d_x = torch.zeros_like(X)
        return (d_x,) + (None,) * (2 * N_GRAPH + 1)


def multi_aggregate(X, graph, directed=False):
    """(sum, sum of squares, max, min) over each row's neighbours from one gather pass, with autograd for X (float32 [N, D]);
    graph = the eight graph tensors, whose pattern must be symmetric (checked before any launch: the backward walks A^T)
    unless directed=True: the backward then runs on transposed_graph(graph).  Rows without entries give 0 in all four."""
    if directed:
        return MultiAggregate.apply(X, *graph, *transposed_graph(graph))
    perm32 = transpose_permutation_i32(graph[0], graph[1])
    return MultiAggregate.apply(X, *graph, *graph, perm32)


class PNAConv(torch.nn.Module):
    """Principal neighbourhood aggregation:  out = X W_root + S W_neigh, S = the concatenation over scalers (outer) and
    aggregators (inner) of scaler(deg) * aggregator(neighbours), all aggregators from one multi_aggregate pass.  With
    deg = clamp(row length, 1):  mean = sum / deg;  std = sqrt(relu(sumsq / deg - mean^2) + 1e-5) (PyG's formula);  max, min.
    Scalers: identity, amplification log(deg + 1) / delta, attenuation delta / log(deg + 1), delta =
    avg_log_deg or, when that is None, the mean of log(deg + 1) over the graph, computed once per row_pointers tensor and kept
    on the device (no host synchronisation, so the layer captures into a HIP graph without a warm-up).  Both products run on
    _Update.  _Conv's call signature, so that Net builds it; edge_weight is refused.  The pattern must be
    symmetric unless directed=True (the backward then runs on transposed_graph)."""

    AGGREGATORS = ("mean", "min", "max", "std")
    SCALERS = ("identity", "amplification", "attenuation")

    def __init__(self, input_dim, output_dim, aggregators=("mean", "min", "max", "std"),
                 scalers=("identity", "amplification", "attenuation"), avg_log_deg=None, directed=False):
        super().__init__()
        aggregators, scalers = tuple(aggregators), tuple(scalers)
        for names, known, what in ((aggregators, self.AGGREGATORS, "aggregators"), (scalers, self.SCALERS, "scalers")):
            if not names or any(n not in known for n in names):
                raise ValueError("PNAConv %s must be among %s, got %r" % (what, ", ".join(repr(k) for k in known), names))
        self.directed = bool(directed)
        self.aggregators, self.scalers = aggregators, scalers
        self.avg_log_deg = None if avg_log_deg is None else float(avg_log_deg)
        self.weights_root = torch.nn.Parameter(torch.empty(input_dim, output_dim))
        self.weights_neigh = torch.nn.Parameter(torch.empty(len(scalers) * len(aggregators) * input_dim, output_dim))
        self._degrees = None  # (row_pointers, deg [N, 1], log(deg + 1) [N, 1], delta) of the last graph
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.weights_root.size(1))
        for p in (self.weights_root, self.weights_neigh):
            p.data.uniform_(-stdv, stdv)

    def degree_terms(self, row_pointers):
        """(deg, log(deg + 1), delta) of a graph: float32 [N, 1], [N, 1] and avg_log_deg or a 0-dim tensor on the graph's device,
        cached per row_pointers tensor"""
        m = self._degrees
        if m is None or m[0] is not row_pointers:
            deg = (row_pointers[1:] - row_pointers[:-1]).clamp(min=1).to(torch.float32).unsqueeze(1)
            log_deg = torch.log(deg + 1.0)
            delta = self.avg_log_deg if self.avg_log_deg is not None else log_deg.mean()
            self._degrees = m = (row_pointers, deg, log_deg, delta)
        return m[1:]

    def scaled_aggregates(self, z_sum, z_sumsq, z_max, z_min, row_pointers):
        """S [N, scalers x aggregators x D] from the four aggregates of multi_aggregate"""
        deg, log_deg, delta = self.degree_terms(row_pointers)
        mean = z_sum / deg
        parts = []
        for a in self.aggregators:
            if a == "mean":
                parts.append(mean)
            elif a == "std":
                parts.append(torch.sqrt(torch.relu(z_sumsq / deg - mean * mean) + 1e-5))
            else:
                parts.append(z_min if a == "min" else z_max)
        agg = torch.cat(parts, 1)
        scaled = []
        for s in self.scalers:
            if s == "identity":
                scaled.append(agg)
            elif s == "amplification":
                scaled.append(agg * (log_deg / delta))
            else:
                scaled.append(agg * (delta / log_deg))
        return torch.cat(scaled, 1) if len(scaled) > 1 else scaled[0]

    def forward(self, X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                col_nzr, output=None, edge_weight=None):
        if edge_weight is not None:
            raise ValueError("PNAConv aggregates with its own aggregators: edge_weight is not accepted")
        graph = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr)
        S = self.scaled_aggregates(*multi_aggregate(X, graph, self.directed), row_pointers)
        return _Update.apply(X, self.weights_root) + _Update.apply(S, self.weights_neigh)


class SoftmaxAggregate(torch.autograd.Function):
    """Per-channel softmax aggregation of each row's neighbour features, Z[i] = sum_j p_ij X[j] with p_ij the softmax over row
    i's entries of t * X[j] (HCSPMM.forward_softmax: one online-softmax gather pass), with gradients for X and t:
      dX = HCSPMM.softmax_backward on the graph the backward walks -- the weights are recomputed from the forward's row maxima
           M and normalisers L, no per-entry tensor is kept;
      dt = sum_i dZ[i] * (Q[i] - Z[i]^2), Q the softmax-weighted mean of the squares (asked of the forward only when t needs a
           gradient), summed over the rows (and the columns, for a t of one element).
    t: a Python float or a tensor of 1 or D elements.  tail = the eight graph tensors of A followed by the eight of the graph the
    backward walks (A itself when the pattern is symmetric, else transposed_graph's)."""

    @staticmethod
    def forward(ctx, X, t, *tail):
        X = X.contiguous()
        learnt = isinstance(t, torch.Tensor)
        beta = t.detach() if learnt else float(t)
        need_t = learnt and ctx.needs_input_grad[1]
        Z, M, L, Q = HCSPMM.forward_softmax(X, beta, *tail[:N_GRAPH], ("M", "L", "Q") if need_t else ("M", "L"))
        ctx.beta = None if learnt else beta
        ctx.save_for_backward(X, Z, M, L, Q, beta if learnt else None, *tail[N_GRAPH:])
        return Z

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward is a launch, not a graph of differentiable ops
    def backward(ctx, d_out):
        X, Z, M, L, Q, beta, *graph_b = ctx.saved_tensors
        d_out = d_out.contiguous()
        d_x = d_t = None
        if ctx.needs_input_grad[0]:
            d_x = HCSPMM.softmax_backward(d_out, Z, M, L, X, ctx.beta if beta is None else beta, *graph_b)
        if ctx.needs_input_grad[1]:
            per_column = (d_out * (Q - Z * Z)).sum(0)
            d_t = (per_column.sum() if beta.numel() == 1 else per_column).reshape(beta.shape)
        return (d_x, d_t) + (None,) * (2 * N_GRAPH)


def softmax_aggregate(X, graph, t=1.0, directed=False):
    """Softmax aggregation over each row's neighbours (DeeperGCN; PyG SoftmaxAggregation), per feature column:
    Z[i] = sum_j softmax_j(t * X[j]) X[j], with autograd for X (float32 [N, D]) and for t when it is a tensor that requires grad
    (1 or D elements; a float otherwise).  t -> +-inf approaches max / min, t = 0 is the mean.  graph = the eight graph tensors,
    whose pattern must be symmetric (checked before any launch: the backward walks A^T) unless directed=True: the backward then
    runs on transposed_graph(graph).  Rows without entries give 0."""
    if directed:
        return SoftmaxAggregate.apply(X, t, *graph, *transposed_graph(graph)[:N_GRAPH])
    transpose_permutation_i32(graph[0], graph[1])  # an asymmetric pattern is refused before any launch (cached)
    return SoftmaxAggregate.apply(X, t, *graph, *graph)


class GENConv(torch.nn.Module):
    """DeeperGCN's generalised aggregation layer with the softmax aggregator:
      out = (X + softmax_aggregate(relu(X) + eps, t)) W
    one softmax_aggregate pass and one product on _Update.  t is the inverse temperature: a float, or with learn_t=True a scalar
    Parameter initialised to it (its gradient costs no kernel: SoftmaxAggregate).  _Conv's call signature, so that Net builds
    it; edge_weight is refused.  The pattern must be symmetric unless directed=True (the backward then runs on
    transposed_graph)."""

    def __init__(self, input_dim, output_dim, t=1.0, learn_t=False, eps=1e-7, directed=False):
        super().__init__()
        self.directed, self.eps = bool(directed), float(eps)
        self.weights = torch.nn.Parameter(torch.empty(input_dim, output_dim))
        self.initial_t = float(t)
        self.t = torch.nn.Parameter(torch.empty(())) if learn_t else self.initial_t
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.weights.size(1))
        self.weights.data.uniform_(-stdv, stdv)
        if isinstance(self.t, torch.Tensor):
            self.t.data.fill_(self.initial_t)

    def forward(self, X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                col_nzr, output=None, edge_weight=None):
        if edge_weight is not None:
            raise ValueError("GENConv aggregates with its own softmax weights: edge_weight is not accepted")
        graph = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr)
        agg = softmax_aggregate(torch.relu(X) + self.eps, graph, self.t, self.directed)
        return _Update.apply(X + agg, self.weights)


class GatedAggregate(torch.autograd.Function):
    """Z[i] = sum over the entries (i, j) of sigmoid(P[i] + Q[j]) * V[j] (HCSPMM.forward_gated: one gather pass, no per-entry
    tensor), with gradients for P, Q and V from the same launch -- no kernel beyond the forward's.  With G = dZ:
      dP = G * T, T[i] = sum_j sigmoid'(P[i] + Q[j]) * V[j]: the forward launch's second output, asked for only when P needs a
           gradient;
      dV = Y_gate and dQ = V * Y_dgate of ONE two-output call on the graph the backward walks, with own rows Q and gathered
           (P, G): fl(Q[j] + P[i]) has the bits of fl(P[i] + Q[j]), so the gates are the forward's.
    A training step is two gather passes.  tail = the eight graph tensors of A followed by the eight of the graph the backward
    walks (A itself when the pattern is symmetric, else transposed_graph's)."""

    @staticmethod
    def forward(ctx, P, Q, V, *tail):
        need_p = ctx.needs_input_grad[0]
        Z, T = HCSPMM.forward_gated(P, Q, V, *tail[:N_GRAPH], ("gate", "dgate") if need_p else ("gate",))
        ctx.save_for_backward(P, Q, V, T, *tail[N_GRAPH:])
        return Z

    @staticmethod
    @torch.autograd.function.once_differentiable  # the backward is a launch, not a graph of differentiable ops
    def backward(ctx, d_out):
        P, Q, V, T, *graph_b = ctx.saved_tensors
        d_out = d_out.contiguous()
        d_p = d_q = d_v = None
        if ctx.needs_input_grad[0]:
            d_p = d_out * T
        need_q, need_v = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if need_q or need_v:
            names = (("gate",) if need_v else ()) + (("dgate",) if need_q else ())
            d_v, y_dgate = HCSPMM.forward_gated(Q, P, d_out, *graph_b, names)
            if need_q:
                d_q = V * y_dgate
        return (d_p, d_q, d_v) + (None,) * (2 * N_GRAPH)


def gated_aggregate(P, Q, V, graph, directed=False):
    """Gated sum over each row's neighbours, Z[i] = sum_j sigmoid(P[i] + Q[j]) * V[j] per feature column, with autograd for P
    [N, D], Q and V (float32 views with unit inner stride: column blocks of one projection pass as they are).  graph = the eight
    graph tensors, whose pattern must be symmetric (checked before any launch: the backward walks A^T) unless directed=True:
    the backward then runs on transposed_graph(graph).  Rows without entries give 0."""
    if directed:
        return GatedAggregate.apply(P, Q, V, *graph, *transposed_graph(graph)[:N_GRAPH])
    transpose_permutation_i32(graph[0], graph[1])  # an asymmetric pattern is refused before any launch (cached)
    return GatedAggregate.apply(P, Q, V, *graph, *graph)


class ResGatedGraphConv(torch.nn.Module):
    """Residual gated graph convolution (Bresson & Laurent; PyG ResGatedGraphConv, the GatedGCN of the GNN benchmarks):
      out[i] = X[i] W_s + sum_j sigmoid(X[i] W_k + X[j] W_q) * (X[j] W_v)
    ONE product X [W_k | W_q | W_v | W_s] on _Update gives [N, 4H] -- Q and V sit side by side in a gathered row -- then
    gated_aggregate on its column blocks, without a copy.  root_weight=False drops the X W_s term (weights [input_dim, 3H]);
    bias=True adds a learnt [H] vector.  _Conv's call signature, so that Net builds it; edge_weight is refused.  The pattern
    must be symmetric unless directed=True (the backward then runs on transposed_graph)."""

    def __init__(self, input_dim, output_dim, directed=False, root_weight=True, bias=False):
        super().__init__()
        self.directed, self.root_weight, self.output_dim = bool(directed), bool(root_weight), int(output_dim)
        self.weights = torch.nn.Parameter(torch.empty(input_dim, (4 if root_weight else 3) * output_dim))
        self.bias = torch.nn.Parameter(torch.empty(output_dim)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.output_dim)
        self.weights.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.zero_()

    def forward(self, X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                col_nzr, output=None, edge_weight=None):
        if edge_weight is not None:
            raise ValueError("ResGatedGraphConv weighs its messages with its own gates: edge_weight is not accepted")
        graph = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr)
        H = self.output_dim
        proj = _Update.apply(X, self.weights)
        out = gated_aggregate(proj[:, :H], proj[:, H:2 * H], proj[:, 2 * H:3 * H], graph, self.directed)
        if self.root_weight:
            out = out + proj[:, 3 * H:]
        return out if self.bias is None else out + self.bias


class EdgeMessageAggregate(torch.autograd.Function):
    """Z[i] = sum over the entries e = (i, j) of m(X[j], F[e]) (HCSPMM.forward_edge_messages; op "mul" x * f, "add_relu"
    relu(x + f), "copy" f) with gradients for X and F [E, D].  dF is HCSPMM.edge_messages_grad; dX is the same forward on A^T:
    "mul" with dZ in the place of X, "add_relu" as the "copy" of dF, F read through the index.  tail = the eight graph tensors of
    A, the eight of the graph the backward walks (A itself when the pattern is symmetric, else transposed_graph's) and the int32
    index of its entries into A's (the transpose permutation, or entry_index_t)."""

    @staticmethod
    def forward(ctx, X, F, op, *tail):
        X = None if X is None else X.contiguous()
        F = F.contiguous()
        ctx.op = op
        ctx.save_for_backward(X, F, *tail)
        return HCSPMM.forward_edge_messages(X, F, *tail[:N_GRAPH], op)[0]

    @staticmethod
    def backward(ctx, d_out):
        X, F, *tail = ctx.saved_tensors
        graph, graph_b, index = tail[:N_GRAPH], tail[N_GRAPH:2 * N_GRAPH], tail[2 * N_GRAPH]
        need_x, need_f = ctx.needs_input_grad[0] and ctx.op != "copy", ctx.needs_input_grad[1]
        d_out = d_out.contiguous()
        d_x = d_f = None
        if ctx.op == "mul":
            if need_f:
                d_f = HCSPMM.edge_messages_grad(d_out, X, None, graph[0], graph[1], "mul")
            if need_x:
                d_x = HCSPMM.forward_edge_messages(d_out, F, *graph_b, "mul", index)[0]
        elif need_x or need_f:  # one pass serves both: dX sums dF over A^T's rows
            d_f = HCSPMM.edge_messages_grad(d_out, X, F, graph[0], graph[1], ctx.op)
            if need_x:
                d_x = HCSPMM.forward_edge_messages(None, d_f, *graph_b, "copy", index)[0]
            if not need_f:
                d_f = None
        return (d_x, d_f, None) + (None,) * len(tail)


def edge_message_aggregate(X, F, graph, op="add_relu", directed=False):
    """Sum over each row's entries of a message of the neighbour's row and the entry's own feature vector, with autograd for
    X [N, D] and F [E, D] (float32; F aligned with column_index): op "mul" X[j] * F[e] (continuous-filter convolutions),
    "add_relu" relu(X[j] + F[e]) (GINE), "copy" F[e] (X may be None).  graph = the eight graph tensors, whose pattern must be
    symmetric (checked before any launch: the backward walks A^T) unless directed=True: the backward then runs on
    transposed_graph(graph).  Rows without entries give 0."""
    if op not in ("mul", "add_relu", "copy"):
        raise ValueError("op must be 'mul', 'add_relu' or 'copy', got %r" % (op,))
    if F.dim() != 2 or F.size(0) != graph[1].numel():
        raise ValueError("F must hold one row per stored entry: [%d, D], got %s" % (graph[1].numel(), tuple(F.shape)))
    if directed:
        gt = transposed_graph(graph)
        return EdgeMessageAggregate.apply(X, F, op, *graph, *gt)
    perm32 = transpose_permutation_i32(graph[0], graph[1])
    return EdgeMessageAggregate.apply(X, F, op, *graph, *graph, perm32)


class GINEConv(torch.nn.Module):
    """GIN with edge attributes (GINE):  out = ((1 + eps) X + sum_j relu(X_j + edge_attr W_e)) W, the sum one
    edge_message_aggregate over the projected edge attributes, both products on _Update.  edge_attr is float32 [E, edge_dim],
    aligned with column_index; W_e [edge_dim, input_dim]; eps is learnt with train_eps=True.  _Conv's call signature with
    edge_attr in the place of edge_weight.  The pattern must be symmetric unless directed=True."""

    def __init__(self, input_dim, output_dim, edge_dim, eps=0.0, train_eps=False, fixed=0, directed=False):
        super().__init__()
        self.fixed, self.directed = fixed, bool(directed)
        self.weights = torch.nn.Parameter(torch.empty(input_dim, output_dim))
        self.weights_edge = torch.nn.Parameter(torch.empty(edge_dim, input_dim))
        self.initial_eps = float(eps)
        if train_eps:
            self.eps = torch.nn.Parameter(torch.empty(()))
        else:
            self.register_buffer("eps", torch.empty(()))
        self.reset_parameters()

    def reset_parameters(self):
        for p in (self.weights, self.weights_edge):
            stdv = 1.0 / math.sqrt(p.size(1))
            p.data.uniform_(-stdv, stdv)
        self.eps.data.fill_(self.initial_eps)

    def forward(self, X, row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr,
                col_nzr, output=None, edge_attr=None):
        if edge_attr is None:
            raise ValueError("GINEConv needs edge_attr [E, edge_dim]")
        graph = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr)
        if not self.directed:
            transpose_permutation_i32(row_pointers, column_index)  # an asymmetric pattern is refused before any launch (cached)
        agg = edge_message_aggregate(X, _Update.apply(edge_attr, self.weights_edge), graph, "add_relu", self.directed)
        return _Update.apply((1.0 + self.eps) * X + agg, self.weights)
