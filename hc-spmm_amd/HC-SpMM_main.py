#!/usr/bin/env python3
"""GCN / GIN / GINE / GAT / GATv2 / SAGE / PNA / GEN / ResGated training driver and single-kernel profiler over the HCSPMM operators -- counterpart
of the reference's HC-SpMM_main.py (same eight flags, HC-SpMM_main.py:18-27, same printed lines
"Prep. (ms)" :54 and "=> SAG profiling avg (ms)" GNN_model.py:261, same model shape :66-110, same
schedule: 9 untimed warm-up epochs then --epochs timed ones, Adam lr 0.01, nll_loss :114-158).

Run from this directory:  python HC-SpMM_main.py --dataset example --model gcn
The graph is read from ./Dataset/<name>.txt ("dst,src" 1-based lines).
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "hybrid_kernel")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import HCSPMM  # noqa: E402  (the torch extension built in hybrid_kernel/)
from config import BLK_H  # noqa: E402
from dataset import HCSPMM_dataset  # noqa: E402
from GNN_model import SAG, GATConv, GATv2Conv, GCNConv, GENConv, GINConv, GINEConv, PNAConv, ResGatedGraphConv, SAGEConv, sampled_graph, tqdm  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", type=str, default="DD_A_our_3", help="dataset")
    p.add_argument("--dim", type=int, default=96, help="input embedding dimension")
    p.add_argument("--num_layers", type=int, default=6, help="num layers")
    p.add_argument("--hidden", type=int, default=32, help="hidden dimension")
    p.add_argument("--classes", type=int, default=22, help="number of output classes")
    p.add_argument("--epochs", type=int, default=200, help="number of epoches")
    p.add_argument("--model", type=str, default="gcn", help="GNN model", choices=["gcn", "gin", "gine", "gat", "gatv2", "sage", "pna", "gen", "resgated"])
    p.add_argument("--single_kernel", action="store_true", help="whether to profile a single SAG kernel")
    # addition (the reference keeps this idea commented out, HC-SpMM_main.py:143-155): replay the whole
    # training step from a HIP graph -- on small graphs an epoch is launch-bound, not kernel-bound
    p.add_argument("--graph", action="store_true", help="capture the training step into a HIP graph and replay it")
    # addition: window classifier (hcspmm.h: 0 the reference's intended rule, 2 as shipped, 3 / 4 the MI355X refits
    # for embedding widths below / from 64)
    p.add_argument("--rule", type=int, default=-1, choices=[-1, 0, 1, 2, 3, 4],
                   help="window classifier rule (-1: the module's default, the width-agnostic MI355X refit; 0: the reference's coefficients)")
    # addition: measure the launch-plan variants no size rule predicts (column slices, panel width) on THIS graph and
    # GPU and keep the fastest (hcspmm.tune_plan: a few plan builds and a few hundred launches before the first epoch)
    p.add_argument("--tune", action="store_true", help="tune the launch plan on this graph before training")
    # addition: the LOI layout reorder as a step of the driver.  The reference ships it as a separate file-to-file program
    # (LOI.cpp main, :807-896, writes reorder_direct.txt) and no code that applies the order; here the graph is relabelled in
    # memory before preprocess, features and labels move with their vertices.  "fast": the relaxed parallel variant
    # (hcspmm_loi_reorder_fast); "exact": reorder_plus_new_direct bit for bit (seconds on large graphs).
    p.add_argument("--loi", type=str, default="none", choices=["none", "fast", "exact"], help="reorder the graph (LOI) before preprocessing")
    # aggregation with edge values: "sym" = D^-1/2 A D^-1/2 (GCN), "mean" = D^-1 A (GraphSAGE-mean), deg = row length
    # (HCSPMM.edge_norm); "none" = the binary A of the reference
    p.add_argument("--norm", type=str, default="none", choices=["none", "sym", "mean"], help="edge normalisation of A")
    # addition: attention heads of --model gat / gatv2 (GNN_model.GATConv / GATv2Conv: the heads' outputs are averaged)
    p.add_argument("--heads", type=int, default=1, help="attention heads (--model gat / gatv2)")
    # addition: the first and hidden GAT layers concatenate their heads (hidden / heads features each), the last averages
    # addition: neighbour aggregation of --model sage (GNN_model.SAGEConv: out = X W_root + AGG(X) W_neigh)
    p.add_argument("--aggr", type=str, default=None, choices=["max", "min", "mean"], help="aggregation of --model sage (default max)")
    p.add_argument("--gat-concat", action="store_true",
                   help="--model gat / gatv2: concatenate the heads of the first and hidden layers (hidden / heads features per head)")
    # addition: message passing over a directed graph (GNN_model.transposed_graph: the backward aggregates with A^T)
    p.add_argument("--directed", action="store_true",
                   help="the graph's pattern need not be symmetric: the layers' backward runs on the transposed graph")
    # addition: 8-bit feature storage in the aggregation (GNN_model.aggregate_fp8: e4m3 codes + one fp32 scale per row in the
    # forward, the exact fp32 backward); after training the model is evaluated once with each storage type
    p.add_argument("--fp8", action="store_true", help="aggregate 8-bit (e4m3) features in the forward (--model gcn / gin with --norm)")
    # addition: --model gine (GNN_model.GINEConv: sum_j relu(x_j + e_ij W_e)); the datasets carry no edge attributes, so --edge-dim
    # of them per stored entry are drawn once from a seeded generator
    p.add_argument("--edge-dim", type=int, default=8, help="edge attributes per entry (--model gine; synthesised, seeded)")
    # addition: --model gen (GNN_model.GENConv: DeeperGCN's softmax aggregation, out = (x + sum_j softmax_j(t x_j) x_j) W)
    p.add_argument("--gen-t", type=float, default=1.0, help="inverse temperature t of --model gen")
    p.add_argument("--gen-learn-t", action="store_true", help="--model gen: learn t (one scalar per layer)")
    # addition: GraphSAGE's neighbour sampling (GNN_model.sampled_graph): every epoch trains on a fresh sample of at most K
    # neighbours per node, drawn on the device with seed = the epoch; a sample is a directed graph, so this implies --directed
    p.add_argument("--sample-fanout", type=int, default=0,
                   help="train every epoch on a fresh sample of at most K neighbours per node (0: off); implies --directed")
    args = p.parse_args(argv)
    if args.sample_fanout < 0:
        p.error("--sample-fanout must not be negative")
    if args.sample_fanout > 0:
        if args.model in ("gcn", "gin") and args.norm == "none":
            p.error("--sample-fanout with --model %s needs --norm: a sample is a directed graph, and the fused binary layer "
                    "functions have no directed form (their backward aggregates with A, as the reference does)" % args.model)
        if args.graph:
            p.error("--sample-fanout redraws the graph every epoch: the step cannot be replayed from a HIP graph")
        args.directed = True
    if args.model == "gen" and args.aggr is not None:
        p.error("--aggr does not apply to --model gen: GENConv aggregates with its softmax weights")
    if args.model == "gen" and args.norm != "none":
        p.error("--norm does not apply to --model gen: its edge values are the softmax weights")
    # addition: --model resgated (GNN_model.ResGatedGraphConv: out = x W_s + sum_j sigmoid(x W_k + x_j W_q) * x_j W_v, the sum one
    # gated gather pass); its edge values are the gates
    if args.model == "resgated":
        if args.aggr is not None:
            p.error("--aggr does not apply to --model resgated: ResGatedGraphConv sums its gated messages")
        if args.norm != "none":
            p.error("--norm does not apply to --model resgated: its edge values are the gates")
        if args.fp8:
            p.error("--fp8 does not apply to --model resgated: the gated aggregation is fp32")
        if args.heads > 1:
            p.error("--heads does not apply to --model resgated: the gate is per feature column")
    # addition: --model pna (GNN_model.PNAConv: mean / min / max / std of the neighbours from one gather pass, times degree scalers);
    # its aggregators are the layer's own, so --aggr is refused
    if args.model == "pna" and args.aggr is not None:
        p.error("--aggr does not apply to --model pna: PNAConv combines mean, min, max and std")
    if args.aggr is None:
        args.aggr = "max"
    if args.edge_dim < 1:
        p.error("--edge-dim must be at least 1")
    if args.model == "gine" and args.norm != "none":
        p.error("--norm does not apply to --model gine: its messages carry the edge attributes")
    if args.fp8:
        if args.model not in ("gcn", "gin") or args.norm == "none":
            p.error("--fp8 needs --model gcn or gin and --norm sym or mean: the binary layer functions and the other models stay fp32")
        widths = (args.dim, args.hidden) if args.model == "gin" else (args.hidden, args.classes)  # what the layers aggregate
        if any(w % 4 != 0 for w in widths):
            p.error("--fp8 aggregates widths %s, which must be multiples of 4" % (widths,))
    if args.directed and args.model in ("gcn", "gin") and args.norm == "none":
        p.error("--directed with --model %s needs --norm: the binary layer functions aggregate with A in the backward, as the "
                "reference does" % args.model)
    if args.model in ("gat", "gatv2") and args.norm != "none":
        p.error("--norm does not apply to --model %s: its edge values are the attention weights" % args.model)
    if args.model == "sage" and args.norm != "none":
        p.error("--norm does not apply to --model sage: its aggregation is --aggr")
    if args.model == "pna" and args.norm != "none":
        p.error("--norm does not apply to --model pna: its aggregators and degree scalers are the layer's own")
    if args.heads < 1:
        p.error("--heads must be at least 1")
    if args.gat_concat and args.model not in ("gat", "gatv2"):
        p.error("--gat-concat applies to --model gat / gatv2 only")
    if args.gat_concat and args.hidden % (4 * args.heads) != 0:
        p.error("--gat-concat needs --hidden to be a multiple of 4 * heads (= %d): each head's width must be a multiple of 4"
                % (4 * args.heads))
    if args.model == "gatv2" and not args.gat_concat and args.hidden % 4 != 0:
        p.error("--model gatv2 needs --hidden to be a multiple of 4 (the width of one head)")
    return args


def nll_loss(log_probs, target):
    """F.nll_loss(log_probs, target) (reference HC-SpMM_main.py:118) as gather + mean: torch's nll_loss reduces
    233 K rows in one workgroup on this stack (154 + 96 us forward + backward, 9 % of a Reddit-scale epoch:
    profiles/r01/gnn_epoch_kernels.log); the same number from two parallel kernels."""
    return -log_probs.gather(1, target.long().unsqueeze(1)).mean()


class _FirstColumns(nn.Module):
    """conv built `width` columns wide, of which the first `keep` are the layer's output: the GATv2 kernels take head widths
    that are multiples of 4, a class count need not be one."""

    def __init__(self, conv, keep):
        super().__init__()
        self.conv, self.keep = conv, keep

    def forward(self, *args, **kwargs):
        return self.conv(*args, **kwargs)[:, :self.keep]


class Net(nn.Module):
    """conv1 (first) -> ReLU -> dropout -> (num_layers - 2) x [hidden conv -> ReLU] -> conv2 (last)
    -> log_softmax   (reference HC-SpMM_main.py:66-110)."""

    def __init__(self, conv_cls, dataset, graph, output, hidden, num_layers, edge_weight=None, edge_attr=None):
        super().__init__()
        self.dataset, self.graph, self.output = dataset, graph, output
        self.ew = {} if edge_weight is None else {"edge_weight": edge_weight}
        if edge_attr is not None:
            self.ew["edge_attr"] = edge_attr
        self.conv1 = conv_cls(dataset.num_features, hidden, 1)
        self.hidden_layers = nn.ModuleList(conv_cls(hidden, hidden, 0) for _ in range(num_layers - 2))
        self.conv2 = conv_cls(hidden, dataset.num_classes, 2)
        self.relu = nn.ReLU()

    def forward(self):
        x = self.relu(self.conv1(self.dataset.x, *self.graph, self.output, **self.ew))
        x = F.dropout(x, training=self.training)
        for conv in self.hidden_layers:
            x = self.relu(conv(x, *self.graph, self.output, **self.ew))
        x = self.conv2(x, *self.graph, self.output, **self.ew)
        return F.log_softmax(x, dim=1)


def set_feature_storage(model, storage):
    """feature_storage of every GCNConv / GINConv of the model ("fp32" or "fp8")."""
    for m in model.modules():
        if isinstance(m, (GCNConv, GINConv)):
            m.feature_storage = storage


def main(argv=None):
    args = parse_args(argv)
    print(args)
    if not torch.cuda.is_available():
        raise RuntimeError("HC-SpMM_main.py needs a GPU: the HCSPMM operators have no CPU path")
    device = torch.device("cuda:0")
    dataset = HCSPMM_dataset(os.path.join("./Dataset/", args.dataset + ".txt"), args.dim, args.classes,
                             load_from_txt=True, device=device)
    num_nodes, num_edges = dataset.num_nodes, dataset.num_edges
    num_row_windows = (num_nodes + BLK_H - 1) // BLK_H
    if args.loi != "none":
        start = time.perf_counter()
        reorder = HCSPMM.loi_reorder_fast if args.loi == "fast" else HCSPMM.loi_reorder
        perm, group_sizes = reorder(dataset.row_pointers, dataset.column_index)
        dataset.row_pointers, dataset.column_index = HCSPMM.apply_permutation(dataset.row_pointers, dataset.column_index, perm)
        order = perm.to(device=device, dtype=torch.long)  # new vertex i is old vertex perm[i]
        dataset.x, dataset.y = dataset.x[order], dataset.y[order]
        print("LOI (ms):\t{:.3f}\t{} groups, {} of them full".format((time.perf_counter() - start) * 1e3, group_sizes.numel(),
                                                                   int((group_sizes == 16).sum())))
    column_index = dataset.column_index.to(device)
    row_pointers = dataset.row_pointers.to(device)
    output = torch.zeros(num_nodes, args.hidden, device=device)

    if args.rule >= 0 and hasattr(HCSPMM, "set_rule"):
        HCSPMM.set_rule(args.rule)
    start = time.perf_counter()
    blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr = HCSPMM.preprocess(
        column_index, row_pointers, num_nodes, num_edges, num_row_windows)
    torch.cuda.synchronize()
    print("Prep. (ms):\t{:.3f}".format((time.perf_counter() - start) * 1e3))
    if args.tune:
        import hcspmm  # the ctypes front-end of the same library: its plan tensors are what HCSPMM.forward* take as row_nzr
        start = time.perf_counter()
        row_nzr, report = hcspmm.tune_plan(row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type,
                                           args.hidden)
        print("Tune (ms):\t{:.3f}\tbest {} at {:.4f} ms, automatic plan {:.4f} ms".format(
            (time.perf_counter() - start) * 1e3, {k: v for k, v in report[0].items() if k != "ms"}, report[0]["ms"],
            next(r["ms"] for r in report if not r.get("slice_threshold") and not r.get("panel_cols"))))
    graph = (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow, hybrid_type, row_nzr, col_nzr)
    edge_weight = None
    if args.norm != "none":  # once, on the (reordered) graph; every layer aggregates with it
        edge_weight = HCSPMM.edge_norm(row_pointers, column_index, args.norm)

    if args.single_kernel:
        return SAG(*graph).profile(dataset.x)

    directed = args.directed
    if args.model in ("gcn", "gin"):
        def conv_cls(input_dim, output_dim, fixed):
            return (GCNConv if args.model == "gcn" else GINConv)(input_dim, output_dim, fixed, directed=directed)
    if args.model == "sage":
        def conv_cls(input_dim, output_dim, fixed):
            return SAGEConv(input_dim, output_dim, fixed, aggr=args.aggr, directed=directed)
    if args.model == "pna":
        def conv_cls(input_dim, output_dim, fixed):
            if fixed == 2:  # the last layer, as for sage
                return SAGEConv(input_dim, output_dim, fixed, aggr=args.aggr, directed=directed)
            return PNAConv(input_dim, output_dim, directed=directed)
    if args.model == "gen":
        def conv_cls(input_dim, output_dim, fixed):
            return GENConv(input_dim, output_dim, t=args.gen_t, learn_t=args.gen_learn_t, directed=directed)
    if args.model == "resgated":
        def conv_cls(input_dim, output_dim, fixed):
            return ResGatedGraphConv(input_dim, output_dim, directed=directed)
    if args.model == "gat":
        def conv_cls(input_dim, output_dim, fixed):
            if args.gat_concat and fixed != 2:  # first / hidden layers: heads x (hidden / heads) features, concatenated
                return GATConv(input_dim, output_dim // args.heads, fixed, heads=args.heads, concat=True, directed=directed)
            return GATConv(input_dim, output_dim, fixed, heads=args.heads, directed=directed)
    if args.model == "gatv2":
        def conv_cls(input_dim, output_dim, fixed):
            if args.gat_concat and fixed != 2:
                return GATv2Conv(input_dim, output_dim // args.heads, fixed, heads=args.heads, concat=True, directed=directed)
            if output_dim % 4 != 0:  # (the class count of the last layer)
                return _FirstColumns(GATv2Conv(input_dim, (output_dim + 3) // 4 * 4, fixed, heads=args.heads, directed=directed),
                                     output_dim)
            return GATv2Conv(input_dim, output_dim, fixed, heads=args.heads, directed=directed)
    edge_attr = None
    if args.model == "gine":
        gen = torch.Generator().manual_seed(0)
        edge_attr = torch.rand(num_edges, args.edge_dim, generator=gen).to(device)

        def conv_cls(input_dim, output_dim, fixed):
            return GINEConv(input_dim, output_dim, args.edge_dim, fixed=fixed, directed=directed)
    model = Net(conv_cls, dataset, graph, output, args.hidden, args.num_layers, edge_weight, edge_attr).to(device)
    if args.fp8:
        set_feature_storage(model, "fp8")
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01, capturable=args.graph)

    epoch = [0]

    def draw_sample():
        """this epoch's sample in the model's place of the graph, with the edge values that go with it"""
        graph_s, entry_index_s = sampled_graph(graph, args.sample_fanout, seed=epoch[0])
        epoch[0] += 1
        model.graph = graph_s
        if edge_weight is not None:  # the normalisation of the SAMPLED graph: its degrees are the sample's
            model.ew["edge_weight"] = HCSPMM.edge_norm(graph_s[0], graph_s[1], args.norm)
        if edge_attr is not None:  # an entry's attributes travel with it
            model.ew["edge_attr"] = edge_attr[entry_index_s.long()]

    def train():
        model.train()
        if args.sample_fanout > 0:
            draw_sample()
        optimizer.zero_grad()
        loss = nll_loss(model()[:], dataset.y[:])
        loss.backward()
        optimizer.step()
        return loss

    for _ in range(1, 10):  # dry run
        train()
    torch.cuda.synchronize()
    step = train
    if args.graph:
        # the HCSPMM operators neither synchronise nor allocate outside torch's allocator, so the
        # whole step (forward, backward, Adam) captures; static_loss is overwritten by every replay
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            optimizer.zero_grad(set_to_none=True)
            with torch.cuda.graph(graph, stream=side):
                static_loss = train()
        torch.cuda.current_stream().wait_stream(side)

        def step():
            graph.replay()
            return static_loss
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = None
    for _ in tqdm(range(1, args.epochs + 1)):
        loss = step()
    torch.cuda.synchronize()
    print("Train (ms/epoch):\t{:.3f}\tfinal loss {:.4f}".format((time.perf_counter() - t0) * 1e3 / max(args.epochs, 1),
                                                                 float(loss.detach()) if loss is not None else float("nan")))
    if args.sample_fanout > 0:  # evaluation aggregates over the full neighbourhoods
        model.graph = graph
        if edge_weight is not None:
            model.ew["edge_weight"] = edge_weight
        if edge_attr is not None:
            model.ew["edge_attr"] = edge_attr
        model.eval()
        with torch.no_grad():
            print("Eval (full graph):\tloss {:.4f}".format(float(nll_loss(model(), dataset.y))))
    if args.fp8:
        log_probs = {}
        model.eval()
        with torch.no_grad():
            for storage in ("fp8", "fp32"):
                set_feature_storage(model, storage)
                log_probs[storage] = model()
        set_feature_storage(model, "fp8")
        agree = (log_probs["fp8"].argmax(1) == log_probs["fp32"].argmax(1)).float().mean()
        print("FP8 eval:\targmax agreement {:.4f}\tmax |log-prob diff| {:.4e}".format(
            float(agree), float((log_probs["fp8"] - log_probs["fp32"]).abs().max())))
    return model


if __name__ == "__main__":
    main()
