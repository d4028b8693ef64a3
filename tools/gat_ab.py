"""Cost of the GAT attention kernels (include/hcspmm.h hcspmm_gat_attention*) on one GPU, timed
with HIP events (median of --steps after --warmup), the variants alternated within one process.  Per workload (made
pattern-symmetric where it is not: A + A^T) and head count, D = 32 -> 32:
  * one GATConv step (forward + backward) three ways: the round-6 formulation (torch-gather logits, EdgeSoftmax,
    edge_weighted_aggregate), the shipped GATConv (gat_attention), plain torch; and the largest relative difference of Y
    and of the gradients, shipped against round-6;
  * gat_attention against edge_softmax on the same logits, gat_attention_backward against edge_softmax_backward.

  python tools/gat_ab.py [--workloads rd_like,reddit,community_loi,dense] [--heads 1,4] [--steps 20] [--warmup 5]
  python tools/gat_ab.py --only round6|new --workloads rd_like --heads 1   (one variant's step alone, for a profiler)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel")]


def _times(fns, steps, warmup):
    """median ms of each fn, the fns alternated step by step"""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return [sorted(t)[len(t) // 2] for t in ts]


def _torch_softmax(x, rows, N):
    import torch
    m = torch.full((N,), -float("inf"), device=x.device).scatter_reduce(0, rows, x, "amax")
    ex = torch.exp(x - m[rows])
    return ex / torch.zeros(N, device=x.device).index_add(0, rows, ex)[rows]


def _symmetric(rp, col):
    """the pattern of A + A^T (GAT needs a symmetric pattern; dense's planted windows are not)"""
    import numpy as np
    N = len(rp) - 1
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(rp))
    key = rows * N + col
    if np.array_equal(np.sort(col.astype(np.int64) * N + rows), key):
        return rp, col
    key = np.unique(np.concatenate([key, col.astype(np.int64) * N + rows]))
    out = np.zeros(N + 1, np.int32)
    np.cumsum(np.bincount(key // N, minlength=N), out=out[1:])
    return out, (key % N).astype(np.int32)


def round6_forward(conv, X, g, rows, cols):
    """GATConv.forward as round 6 shipped it: per-head torch gathers for the logits, then EdgeSoftmax"""
    import torch
    import GNN_model
    hs, logits = [], []
    for k in range(conv.heads):
        h = GNN_model._Update.apply(X, conv.weights[k])
        hs.append(h)
        logits.append(torch.nn.functional.leaky_relu((h @ conv.a_dst[k])[rows] + (h @ conv.a_src[k])[cols], conv.negative_slope))
    alpha = GNN_model.EdgeSoftmax.apply(torch.stack(logits), g[0])
    out = GNN_model.edge_weighted_aggregate(hs[0], alpha[0], g)
    for k in range(1, conv.heads):
        out = out + GNN_model.edge_weighted_aggregate(hs[k], alpha[k], g)
    return out / conv.heads if conv.heads > 1 else out


def torch_forward(conv, X, rows, cols, N):
    import torch
    outs = []
    for k in range(conv.heads):
        h = X @ conv.weights[k]
        logit = torch.nn.functional.leaky_relu((h @ conv.a_dst[k])[rows] + (h @ conv.a_src[k])[cols], conv.negative_slope)
        alpha = _torch_softmax(logit, rows, N)
        outs.append(torch.zeros_like(h).index_add(0, rows, alpha[:, None] * h[cols]))
    return torch.stack(outs).mean(0) if conv.heads > 1 else outs[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rd_like,reddit,community_loi,dense")
    ap.add_argument("--heads", default="1,4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["round6", "new"], default=None)
    args = ap.parse_args()
    import torch
    import bench
    import hcspmm
    import GNN_model
    dev = torch.device("cuda:0")
    D = 32
    for wl in args.workloads.split(","):
        n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
        rp, col = _symmetric(*bench.make_local_block(wl, n_local, e_local, vw, 0))
        N, E = len(rp) - 1, len(col)
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        rows = torch.repeat_interleave(torch.arange(N, device=dev), (rp_d[1:] - rp_d[:-1]).long())
        cols = col_d.long()
        g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=D))
        for heads in [int(h) for h in args.heads.split(",")]:
            t0 = time.time()
            torch.manual_seed(heads)
            conv = GNN_model.GATConv(D, D, 0, heads=heads).to(dev)
            X = torch.randn(N, D, device=dev, requires_grad=True)
            G = torch.randn(N, D, device=dev)
            params = [X, conv.weights, conv.a_src, conv.a_dst]

            def step(fwd):
                def run():
                    for p in params:
                        p.grad = None
                    (fwd() * G).sum().backward()
                return run

            new_step = step(lambda: conv(X, *g, None))
            old_step = step(lambda: round6_forward(conv, X, g, rows, cols))
            if args.only:
                fn = new_step if args.only == "new" else old_step
                for _ in range(args.warmup + args.steps):
                    fn()
                torch.cuda.synchronize()
                print("%s %s heads %d: %d steps done" % (args.only, wl, heads, args.warmup + args.steps), flush=True)
                continue
            # agreement, shipped against round-6
            res = []
            for fwd in (lambda: conv(X, *g, None), lambda: round6_forward(conv, X, g, rows, cols)):
                for p in params:
                    p.grad = None
                Y = fwd()
                (Y * G).sum().backward()
                res.append([Y.detach().clone()] + [p.grad.clone() for p in params])
            diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(*res))
            t_new, t_old = _times([new_step, old_step], args.steps, args.warmup)
            t_torch = _times([step(lambda: torch_forward(conv, X, rows, cols, N))], max(5, args.steps // 4), 2)[0]
            # the attention kernels against the edge softmax on the same logits
            s_dst, s_src = torch.randn(N, heads, device=dev), torch.randn(N, heads, device=dev)
            perm32 = GNN_model.transpose_permutation_i32(rp_d, col_d)
            logits = torch.nn.functional.leaky_relu(s_dst[rows] + s_src[cols], 0.2).t().contiguous()
            alpha = hcspmm.gat_attention(s_dst, s_src, rp_d, col_d)
            assert torch.equal(alpha, hcspmm.edge_softmax(logits, rp_d)), "gat_attention differs from edge_softmax"
            ga = torch.randn_like(alpha)
            t_ga, t_sm, t_gab, t_smb = _times(
                [lambda: hcspmm.gat_attention(s_dst, s_src, rp_d, col_d), lambda: hcspmm.edge_softmax(logits, rp_d),
                 lambda: hcspmm.gat_attention_backward(alpha, ga, s_dst, s_src, rp_d, col_d, perm32),
                 lambda: hcspmm.edge_softmax_backward(alpha, ga, rp_d)], args.steps * 2, args.warmup)
            print("%-14s heads=%d N=%d E=%d | step: new %.3f ms | round-6 %.3f ms (new %.2fx faster) | torch %.3f ms "
                  "(new %.2fx faster) | max rel diff %.2g | gat_attention %.4f ms vs edge_softmax %.4f ms (%.2fx) | "
                  "backward %.4f ms vs edge_softmax_backward %.4f ms (%.2fx) | %.0f s"
                  % (wl, heads, N, E, t_new, t_old, t_old / t_new, t_torch, t_torch / t_new, diff, t_ga, t_sm, t_ga / t_sm,
                     t_gab, t_smb, t_gab / t_smb, time.time() - t0), flush=True)
            del conv, X, G, res, logits, alpha, ga
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
