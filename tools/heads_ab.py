"""Cost of the multi-head kernels (include/hcspmm.h hcspmm_forward_weighted_heads / hcspmm_sddmm_heads; DESIGN.md
section 3.11) on one GPU, timed with HIP events (median of --steps after --warmup), the variants alternated within one
process.  Per workload (made pattern-symmetric where it is not: A + A^T) and heads x Dh:
  * forward_weighted_heads against one forward_weighted at the same D, and against `heads` forward_weighted launches on
    the column slices (what a per-head layer does);
  * sddmm_heads against `heads` sddmm calls on the column slices;
  * (--layer) one concatenating GATConv step (forward + backward) against the same layer assembled from the existing
    pieces: per-head _Update, torch score products, gat_attention, per-head edge_weighted_aggregate, torch.cat.

  python tools/heads_ab.py [--workloads rd_like,community_loi,reddit] [--shapes 4x8,8x8,4x16,4x32] [--layer 8x8,4x16]
  python tools/heads_ab.py --only layer --workloads rd_like --layer 8x8   (the new layer step alone, for a profiler)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel"),
                os.path.join(ROOT, "tools")]

from gat_ab import _symmetric, _times  # noqa: E402


def pieces_forward(conv, X, g):
    """GATConv(concat=True) from the pieces that existed before the multi-head kernels"""
    import torch
    import GNN_model
    hs = [GNN_model._Update.apply(X, conv.weights[k]) for k in range(conv.heads)]
    s_dst = torch.stack([h @ conv.a_dst[k] for k, h in enumerate(hs)], 1)
    s_src = torch.stack([h @ conv.a_src[k] for k, h in enumerate(hs)], 1)
    alpha = GNN_model.gat_attention(s_dst, s_src, g, conv.negative_slope)
    return torch.cat([GNN_model.edge_weighted_aggregate(h, alpha[k], g) for k, h in enumerate(hs)], 1)


def _shapes(s):
    return [tuple(int(v) for v in x.split("x")) for x in s.split(",") if x]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rd_like,community_loi,reddit")
    ap.add_argument("--shapes", default="4x8,8x8,4x16,4x32")
    ap.add_argument("--layer", default="8x8,4x16")
    ap.add_argument("--layer-workloads", default="rd_like")
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
        for heads, dh in (_shapes(args.shapes) if wl in wls and not args.only else []):
            t0 = time.time()
            D = heads * dh
            X = torch.randn(N, D, device=dev)
            V = torch.rand(heads, E, device=dev)
            v0 = V[0].contiguous()
            vh = [V[h].contiguous() for h in range(heads)]
            xs = [X[:, h * dh:(h + 1) * dh].contiguous() for h in range(heads)]
            got = hcspmm.forward_weighted_heads(X, V, *g)[0]
            for h in range(heads):  # the bit contract, once per shape
                want = hcspmm.forward_weighted(X, vh[h], *g)[0]
                assert torch.equal(got[:, h * dh:(h + 1) * dh], want[:, h * dh:(h + 1) * dh]), (wl, heads, dh, h)
            t_mh, t_one, t_per = _times([lambda: hcspmm.forward_weighted_heads(X, V, *g),
                                         lambda: hcspmm.forward_weighted(X, v0, *g),
                                         lambda: [hcspmm.forward_weighted(xs[h], vh[h], *g) for h in range(heads)]],
                                        args.steps, args.warmup)
            t_sh, t_sp = _times([lambda: hcspmm.sddmm_heads(X, X, *g, heads),
                                 lambda: [hcspmm.sddmm(X[:, h * dh:(h + 1) * dh], X[:, h * dh:(h + 1) * dh], *g)
                                          for h in range(heads)]], args.steps, args.warmup)
            print("%-14s %dx%-3d N=%d E=%d | forward_weighted_heads %.4f ms | forward_weighted same D %.4f ms (%.3fx) | "
                  "%d per-head launches %.4f ms (heads kernel %.2fx faster) | sddmm_heads %.4f ms vs %d sddmm %.4f ms "
                  "(%.2fx faster) | %.0f s"
                  % (wl, heads, dh, N, E, t_mh, t_one, t_mh / t_one, heads, t_per, t_per / t_mh, t_sh, heads, t_sp,
                     t_sp / t_sh, time.time() - t0), flush=True)
            del X, V, v0, vh, xs, got
            torch.cuda.empty_cache()
        for heads, dh in (_shapes(args.layer) if wl in args.layer_workloads.split(",") else []):
            t0 = time.time()
            torch.manual_seed(heads)
            conv = GNN_model.GATConv(32, dh, 0, heads=heads, concat=True).to(dev)
            X = torch.randn(N, 32, device=dev, requires_grad=True)
            G = torch.randn(N, heads * dh, device=dev)
            params = [X, conv.weights, conv.a_src, conv.a_dst]

            def step(fwd):
                def run():
                    for p in params:
                        p.grad = None
                    (fwd() * G).sum().backward()
                return run

            new_step = step(lambda: conv(X, *g, None))
            old_step = step(lambda: pieces_forward(conv, X, g))
            if args.only:
                for _ in range(args.warmup + args.steps):
                    new_step()
                torch.cuda.synchronize()
                print("layer %s %dx%d: %d steps done" % (wl, heads, dh, args.warmup + args.steps), flush=True)
                continue
            res = []
            for fwd in (lambda: conv(X, *g, None), lambda: pieces_forward(conv, X, g)):
                for p in params:
                    p.grad = None
                Y = fwd()
                (Y * G).sum().backward()
                res.append([Y.detach().clone()] + [p.grad.clone() for p in params])
            diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(*res))
            t_new, t_old = _times([new_step, old_step], args.steps, args.warmup)
            print("%-14s layer %dx%-3d N=%d E=%d | concat step: new %.3f ms | from pieces %.3f ms (new %.2fx faster) | "
                  "max rel diff %.2g | %.0f s" % (wl, heads, dh, N, E, t_new, t_old, t_old / t_new, diff, time.time() - t0),
                  flush=True)
            del conv, X, G, res
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
