"""What do the edge-feature message kernels buy over composing the same sum in torch?  (include/hcspmm.h
hcspmm_forward_edge_messages / hcspmm_edge_messages_grad)  Per case -- a bench.py workload and an
embedding width -- on one graph and plan, timed with HIP events on one GPU and alternated step by step within one process:
  (a) forward_edge_messages for mul / add_relu / copy, direct (F[e]) and indexed: the dX launch, on A^T's graph and plan with
      index = entry_index_t;
  (b) edge_messages_grad for the three ops;
  (c) the torch composition of the direct forward: gather X[col], the elementwise op against F, index_add_ over the rows;
  (d) forward_weighted on the same graph, for scale (one scalar per entry instead of a row of F).
Each of --repeats rounds gives the median of --steps steps (after --warmup); a line reports the median of the round medians
and, for the direct forward, the achieved bytes per second over the compulsory traffic 4 E D (the F stream) + 4 N D (X once)
+ 4 N D (Z).  The one condition: (a) direct is not slower than (c) on any line -- a line that misses it says so.

  python tools/edge_messages_ab.py [--cases rd_like:32,rd_like:128,...] [--steps 20] [--warmup 5] [--repeats 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "tools")]

from gat_ab import _times  # noqa: E402

OPS = ("mul", "add_relu", "copy")
WORKLOADS = ("rd_like", "community_loi", "yh_like", "reddit")  # yh_like: graphs.molecule_graph of 3.1 M nodes


def _median(v):
    return sorted(v)[len(v) // 2]


def _graph(bench, wl):
    if wl == "community_loi":  # bench.py's: the community graph after the relaxed parallel LOI reorder
        import torch
        import hcspmm
        n, e, _, vw, _ = bench.WORKLOADS["community"]
        rp, col = (torch.from_numpy(a) for a in bench.make_local_block("community", n, e, vw, 0))
        perm, _ = hcspmm.loi_reorder(rp, col, variant="fast")
        rp, col = hcspmm.apply_permutation(rp, col, perm)
        return rp.numpy(), col.numpy()
    n, e, _, vw, _ = bench.WORKLOADS[wl]
    return bench.make_local_block(wl, n, e, vw, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join("%s:%d" % (w, d) for w in WORKLOADS for d in (32, 128)))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    import bench
    import hcspmm
    if not torch.cuda.is_available():
        raise SystemExit("edge_messages_ab.py needs a GPU: it measures, and a CPU has nothing to say about these kernels")
    dev = torch.device("cuda:0")
    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",") if c]
    built = {}
    missed = 0
    for wl, D in cases:
        if wl not in built:
            built.clear()
            torch.cuda.empty_cache()
            t0 = time.time()
            rp, col = _graph(bench, wl)
            N, E = len(rp) - 1, len(col)
            rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
            rp_t, col_t, eid_t = hcspmm.transpose_graph(rp_d, col_d)
            rows = torch.repeat_interleave(torch.arange(N, device=dev), (rp_d[1:] - rp_d[:-1]).long())
            built[wl] = (N, E, rp_d, col_d, rp_t, col_t, eid_t, rows, col_d.long(), torch.rand(E, device=dev))
            print("%-13s N=%d E=%d | graph and its transpose ready in %.0f s" % (wl, N, E, time.time() - t0), flush=True)
        N, E, rp_d, col_d, rp_t, col_t, eid_t, rows, col64, values = built[wl]
        g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=D))
        gt = (rp_t, col_t) + tuple(hcspmm.preprocess(col_t, rp_t, N, E, (N + 15) // 16, dim=D))
        X, F, dZ = torch.randn(N, D, device=dev), torch.randn(E, D, device=dev), torch.randn(N, D, device=dev)

        def direct(op):
            return lambda: hcspmm.forward_edge_messages(X, F, *g, op)[0]

        def indexed(op):
            return lambda: hcspmm.forward_edge_messages(X, F, *gt, op, eid_t)[0]

        def grad(op):
            return lambda: hcspmm.edge_messages_grad(dZ, X, F, rp_d, col_d, op)

        def composed(op):
            def run():
                m = F if op == "copy" else X.index_select(0, col64)
                if op == "mul":
                    m = m.mul_(F)
                elif op == "add_relu":
                    m = m.add_(F).relu_()
                return torch.zeros(N, D, device=dev).index_add_(0, rows, m)
            return run

        fns = [f(op) for f in (direct, indexed, grad, composed) for op in OPS] + [lambda: hcspmm.forward_weighted(X, values, *g)[0]]
        rounds = [_times(fns, args.steps, args.warmup) for _ in range(args.repeats)]
        ms = [_median([r[k] for r in rounds]) for k in range(len(fns))]
        lo = [min(r[k] for r in rounds) for k in range(len(fns))]
        hi = [max(r[k] for r in rounds) for k in range(len(fns))]
        compulsory = 4.0 * E * D + 8.0 * N * D
        for i, op in enumerate(OPS):
            a, b, c, t = ms[i], ms[3 + i], ms[6 + i], ms[9 + i]
            ok = a <= t
            missed += 0 if ok else 1
            print("%-13s D=%-3d %-8s | (a) direct %.4f ms (rounds %.4f-%.4f) = %.2f TB/s of %.0f MB compulsory | indexed on A^T %.4f ms "
                  "| (b) grad_F %.4f ms | (c) torch gather + op + index_add_ %.4f ms (rounds %.4f-%.4f), c / a = %.2f -> %s"
                  % (wl, D, op, a, lo[i], hi[i], compulsory / a / 1e9, compulsory / 1e6, b, c, t, lo[9 + i], hi[9 + i], t / a,
                     "ok" if ok else "MISSED: the kernel is slower than the composition"), flush=True)
        print("%-13s D=%-3d          | (d) forward_weighted %.4f ms (rounds %.4f-%.4f)" % (wl, D, ms[12], lo[12], hi[12]), flush=True)
        del X, F, dZ, g, gt
        torch.cuda.empty_cache()
    print("lines on which (a) is slower than (c): %d" % missed, flush=True)


if __name__ == "__main__":
    main()
