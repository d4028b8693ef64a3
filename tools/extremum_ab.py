"""Cost of the max / min aggregation (include/hcspmm.h hcspmm_forward_extremum*) on one GPU, timed
with HIP events (median of --steps after --warmup), the variants alternated within one process.  Per workload (made
pattern-symmetric where it is not: A + A^T) and width D:
  * forward_max with and without arg against forward_weighted at the same D;
  * forward_extremum_backward against the forward (with arg);
  * both against the torch formulation: index_select of every entry + scatter_reduce("amax"), and its autograd backward;
  * (--layer) one SAGEConv(aggr="max") training step against the same layer built in torch.

  python tools/extremum_ab.py [--workloads rd_like,community_loi,reddit] [--dims 32,128] [--layer 32]
  python tools/extremum_ab.py --only layer --workloads rd_like --layer 32   (the layer step alone, for a profiler)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel"),
                os.path.join(ROOT, "tools")]

from gat_ab import _symmetric, _times  # noqa: E402


def torch_max(X, rows, col):
    """the torch formulation: every entry's row gathered (E x D), then reduced per row (rows = row of each entry)"""
    import torch
    src = X.index_select(0, col)
    return torch.zeros(X.size(0), X.size(1), device=X.device).scatter_reduce(
        0, rows[:, None].expand_as(src), src, "amax", include_self=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rd_like,community_loi,reddit")
    ap.add_argument("--dims", default="32,128")
    ap.add_argument("--layer", default="32")
    ap.add_argument("--layer-workloads", default="rd_like,reddit")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["layer"], default=None)
    args = ap.parse_args()
    import torch
    import bench
    import hcspmm
    import GNN_model
    dev = torch.device("cuda:0")
    wls = args.workloads.split(",")
    for wl in dict.fromkeys(wls + args.layer_workloads.split(",")):
        n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
        rp, col = _symmetric(*bench.make_local_block(wl, n_local, e_local, vw, 0))
        N, E = len(rp) - 1, len(col)
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=32))
        perm = hcspmm.transpose_permutation(rp_d, col_d).to(torch.int32)
        rows = torch.repeat_interleave(torch.arange(N, device=dev), (rp_d[1:] - rp_d[:-1]).long())
        col64 = col_d.long()
        ones = torch.ones(E, device=dev)
        for D in ([int(d) for d in args.dims.split(",")] if wl in wls and not args.only else []):
            t0 = time.time()
            X = torch.randn(N, D, device=dev)
            G = torch.randn(N, D, device=dev)
            Z, arg = hcspmm.forward_max(X, *g)
            assert torch.equal(Z, torch_max(X, rows, col64)), (wl, D)  # continuous data: the same values
            Xt = X.clone().requires_grad_(True)
            Zt = torch_max(Xt, rows, col64)
            t_arg, t_noarg, t_w, t_bwd, t_tf = _times(
                [lambda: hcspmm.forward_max(X, *g), lambda: hcspmm.forward_max(X, *g, return_arg=False),
                 lambda: hcspmm.forward_weighted(X, ones, *g), lambda: hcspmm.forward_extremum_backward(G, arg, perm, *g),
                 lambda: torch_max(X, rows, col64)], args.steps, args.warmup)
            t_tb, = _times([lambda: torch.autograd.grad(Zt, Xt, G, retain_graph=True)], args.steps, args.warmup)
            print("%-14s D=%-4d N=%d E=%d | max+arg %.4f ms (%.2fx weighted) | max %.4f ms (%.2fx weighted) | "
                  "forward_weighted %.4f ms | backward %.4f ms (%.2fx forward) | torch fwd %.4f ms (%.1fx slower) | "
                  "torch bwd %.4f ms (%.1fx slower) | %.0f s"
                  % (wl, D, N, E, t_arg, t_arg / t_w, t_noarg, t_noarg / t_w, t_w, t_bwd, t_bwd / t_arg, t_tf, t_tf / t_arg,
                     t_tb, t_tb / t_bwd, time.time() - t0), flush=True)
            del X, G, Z, arg, Xt, Zt
            torch.cuda.empty_cache()
        for D in ([int(d) for d in args.layer.split(",")] if wl in args.layer_workloads.split(",") else []):
            t0 = time.time()
            torch.manual_seed(D)
            conv = GNN_model.SAGEConv(D, D, 0, aggr="max").to(dev)
            # distinct values: no ties, where torch's amax gradient would split among the tied entries (this library's goes to
            # the lowest entry, deterministically)
            X = (torch.randperm(N * D, device=dev).float() / (N * D) - 0.5).view(N, D).requires_grad_(True)
            G = torch.randn(N, D, device=dev)
            Wr = conv.weights_root.detach().clone().requires_grad_(True)
            Wn = conv.weights_neigh.detach().clone().requires_grad_(True)

            def torch_layer():
                return X @ Wr + torch_max(X, rows, col64) @ Wn

            def step(fwd, params):
                def run():
                    for p in params:
                        p.grad = None
                    (fwd() * G).sum().backward()
                return run

            new_step = step(lambda: conv(X, *g, None), [X, conv.weights_root, conv.weights_neigh])
            old_step = step(torch_layer, [X, Wr, Wn])
            if args.only:
                for _ in range(args.warmup + args.steps):
                    new_step()
                torch.cuda.synchronize()
                print("layer %s D=%d: %d steps done" % (wl, D, args.warmup + args.steps), flush=True)
                continue
            new_step()
            res_new = [conv(X, *g, None).detach().clone(), X.grad.clone(), conv.weights_root.grad.clone()]
            old_step()
            res_old = [torch_layer().detach().clone(), X.grad.clone(), Wr.grad.clone()]
            diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(res_new, res_old))
            t_new, t_old = _times([new_step, old_step], args.steps, args.warmup)
            print("%-14s layer D=%-4d N=%d E=%d | SAGEConv(max) step: new %.3f ms | torch %.3f ms (new %.2fx faster) | "
                  "max rel diff %.2g | %.0f s" % (wl, D, N, E, t_new, t_old, t_old / t_new, diff, time.time() - t0), flush=True)
            del conv, X, G
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
