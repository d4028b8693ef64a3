"""Should the multi-head backward read its values through an index?  (include/hcspmm.h hcspmm_forward_weighted_indexed;
DESIGN.md section 3.14.)  The backward dX = A_w^T dY of the multi-head layers on a pattern-symmetric graph, two forms with
the same bits, timed with HIP events on one GPU and alternated step by step within one process:
  (a) values[:, perm].contiguous() (a torch gather through the int64 permutation) + forward_weighted_heads -- the reference;
  (b) one forward_weighted_indexed call with the int32 permutation.
Each of --repeats rounds gives the median of --steps steps (after --warmup) of both; the spread of (a) is max - min of its
round medians.  The rule printed at the end of each line: (b) replaces (a) only when median(a) - median(b) exceeds that spread.

Then, for the record, one GATv2Conv step (forward + backward, 4 heads x 8 columns, concatenated) on the RD-sized graph as
generated (pattern-symmetric, directed=False) and with shuffled direction (the same generator with symmetric=False,
directed=True: its own transposed graph and plan).

  python tools/indexed_values_ab.py [--cases rd_like:4x8,reddit:8x8,reddit:4x32] [--steps 30] [--warmup 10] [--repeats 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel"),
                os.path.join(ROOT, "tools")]

from gat_ab import _symmetric, _times  # noqa: E402


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="rd_like:4x8,reddit:8x8,reddit:4x32")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-layer", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    import hcspmm
    from hcspmm import graphs
    if not torch.cuda.is_available():
        raise SystemExit("indexed_values_ab.py needs a GPU: it measures, and a CPU has nothing to say about these kernels")
    dev = torch.device("cuda:0")
    cases = [(c.split(":")[0], tuple(int(v) for v in c.split(":")[1].split("x"))) for c in args.cases.split(",") if c]
    built = {}
    for wl, (heads, dh) in cases:
        if wl not in built:
            t0 = time.time()
            n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
            rp, col = _symmetric(*bench.make_local_block(wl, n_local, e_local, vw, 0))
            N, E = len(rp) - 1, len(col)
            rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
            g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=32))
            perm = hcspmm.transpose_permutation(rp_d, col_d)
            built[wl] = (N, E, g, perm, perm.to(torch.int32))
            print("%-8s N=%d E=%d | graph, plan and permutation ready in %.0f s" % (wl, N, E, time.time() - t0), flush=True)
        N, E, g, perm, perm32 = built[wl]
        D = heads * dh
        dY = torch.randn(N, D, device=dev)
        V = torch.rand(heads, E, device=dev)

        def form_a():
            return hcspmm.forward_weighted_heads(dY, V[:, perm].contiguous(), *g)[0]

        def form_b():
            return hcspmm.forward_weighted_indexed(dY, V, perm32, *g)[0]

        def gather_only():
            return V[:, perm].contiguous()

        assert torch.equal(form_a(), form_b()), (wl, heads, dh)  # the bit contract, at the size that is timed
        rounds = [_times([form_a, form_b, gather_only], args.steps, args.warmup) for _ in range(args.repeats)]
        ta, tb, tg = ([r[k] for r in rounds] for k in range(3))
        spread = max(ta) - min(ta)
        gain = _median(ta) - _median(tb)
        print("%-8s %dx%-3d | (a) gather + forward_weighted_heads %.4f ms (rounds %s; spread %.4f ms; the gather alone %.4f ms) | "
              "(b) forward_weighted_indexed %.4f ms (rounds %s) | a - b = %+.4f ms (%.1f %% of a) -> %s"
              % (wl, heads, dh, _median(ta), " ".join("%.4f" % t for t in ta), spread, _median(tg), _median(tb),
                 " ".join("%.4f" % t for t in tb), gain, 100.0 * gain / _median(ta),
                 "(b) is faster beyond the spread of (a)" if gain > spread else "stay on (a)"), flush=True)
        del dY, V
        torch.cuda.empty_cache()
    if args.no_layer:
        return
    built.clear()
    torch.cuda.empty_cache()
    import GNN_model
    import HCSPMM
    n_local, e_local, _, _, _ = bench.WORKLOADS["rd_like"]
    for name, symmetric in (("symmetric", True), ("directed", False)):
        t0 = time.time()
        rp, col = graphs.powerlaw_graph(n_local, e_local, seed=3, symmetric=symmetric)
        N, E = len(rp) - 1, len(col)
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        g = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16))
        torch.manual_seed(4)
        conv = GNN_model.GATv2Conv(32, 8, 0, heads=4, concat=True, directed=not symmetric).to(dev)
        X = torch.randn(N, 32, device=dev, requires_grad=True)
        G = torch.randn(N, 32, device=dev)
        params = [X, conv.weights, conv.att]

        def step():
            for p in params:
                p.grad = None
            (conv(X, *g, None) * G).sum().backward()

        step()  # (directed: builds and caches the transposed graph and its plan, outside the timed window)
        torch.cuda.synchronize()
        ready = time.time() - t0
        rounds = [_times([step], args.steps, args.warmup)[0] for _ in range(args.repeats)]
        print("rd_like  GATv2Conv 4x8 step, %-9s pattern N=%d E=%d longest row %d, longest column %d | %.3f ms (rounds %s) | "
              "ready in %.0f s" % (name, N, E, int((rp[1:] - rp[:-1]).max()), int(np.bincount(col).max()),
                                   _median(rounds), " ".join("%.3f" % t for t in rounds), ready), flush=True)
        del conv, X, G, g, rp_d, col_d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
