"""Cost of the one-pass sum / sum-of-squares / max / min aggregation (include/hcspmm.h hcspmm_forward_multi; DESIGN.md section
3.17) on one GPU, timed with HIP events (median of --steps after --warmup), the variants alternated within one process.  Per
workload (made pattern-symmetric where it is not: A + A^T) and width D:
  (a) forward_multi with all six outputs;
  (b) the four launches it replaces: forward(X), forward(X * X) with the squaring included, forward_max and forward_min, both
      with arg;
  (c) forward_max with arg alone;
  (d) (--layer) one PNAConv training step against the same layer with multi_aggregate replaced by the composition.
The bar is (a) < (b) on every point: the pass gathers a quarter of (b)'s bytes and writes the same outputs.

Every workload is a step of its own: a child process under its own time limit; the run stops at the first step that fails.
The parent never opens the GPU.

  python tools/multi_aggr_ab.py [--workloads rd_like,community_loi,reddit] [--dims 32,128] [--layer 32] [--log FILE]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel"),
                os.path.join(ROOT, "tools")]


def step(args, wl):
    import torch
    import bench
    import hcspmm
    import GNN_model
    from gat_ab import _symmetric, _times
    dev = torch.device("cuda:0")
    n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
    if wl == "community_loi":  # bench.py's workload: the community graph after the relaxed parallel LOI reorder
        rp, col = _symmetric(*bench.make_local_block("community", n_local, e_local, vw, 0))
        rpt, colt = torch.from_numpy(rp), torch.from_numpy(col)
        perm, _ = hcspmm.loi_reorder(rpt, colt, variant="fast")
        rp, col = (t.numpy() for t in hcspmm.apply_permutation(rpt, colt, perm))
    else:
        rp, col = _symmetric(*bench.make_local_block(wl, n_local, e_local, vw, 0))
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=32))

    def composition(X):
        return (hcspmm.forward(X, *g)[0], hcspmm.forward(X * X, *g)[0], *hcspmm.forward_max(X, *g), *hcspmm.forward_min(X, *g))

    for D in [int(d) for d in args.dims.split(",") if d]:
        t0 = time.time()
        X = torch.randn(N, D, device=dev)
        new = hcspmm.forward_multi(X, *g)
        s, q, zx, ax, zn, an = composition(X)
        for a, b in ((new[2], zx), (new[3], zn), (new[4], ax), (new[5], an)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (wl, D)
        sum_diff = float(((new[0] - s).abs() / hcspmm.forward(X.abs(), *g)[0].clamp_min(1e-30)).max())
        t_a, t_b, t_c = _times([lambda: hcspmm.forward_multi(X, *g), lambda: composition(X), lambda: hcspmm.forward_max(X, *g)],
                               args.steps, args.warmup)
        print("%-14s D=%-4d N=%d E=%d | (a) forward_multi %.4f ms | (b) four launches %.4f ms: (a)/(b) %.3f %s | "
              "(c) forward_max+arg %.4f ms: (a)/(c) %.3f | sum vs forward: %.1e of sum|x| | %.0f s"
              % (wl, D, N, E, t_a, t_b, t_a / t_b, "ok" if t_a < t_b else "MISSES THE BAR", t_c, t_a / t_c, sum_diff,
                 time.time() - t0), flush=True)
        del X, new, s, q, zx, ax, zn, an
        torch.cuda.empty_cache()

    perm32 = GNN_model.transpose_permutation_i32(rp_d, col_d)

    class Binary(torch.autograd.Function):  # A X with the gradient A^T dY = A dY (the pattern is symmetric)
        @staticmethod
        def forward(ctx, X):
            return hcspmm.forward(X.contiguous(), *g)[0]

        @staticmethod
        def backward(ctx, d):
            return hcspmm.forward(d.contiguous(), *g)[0]

    def composed_aggregate(X, graph, directed=False):
        return (Binary.apply(X), Binary.apply(X * X), GNN_model.ExtremumAggregate.apply(X, "max", perm32, *graph),
                GNN_model.ExtremumAggregate.apply(X, "min", perm32, *graph))

    for D in [int(d) for d in args.layer.split(",") if d]:
        t0 = time.time()
        torch.manual_seed(D)
        conv = GNN_model.PNAConv(D, D).to(dev)
        X = torch.randn(N, D, device=dev).requires_grad_(True)
        G = torch.randn(N, D, device=dev)
        one_pass = GNN_model.multi_aggregate

        def train_step(aggregate):
            def run():
                for p in (X, conv.weights_root, conv.weights_neigh):
                    p.grad = None
                GNN_model.multi_aggregate = aggregate
                try:
                    out = conv(X, *g, None)
                finally:
                    GNN_model.multi_aggregate = one_pass
                (out * G).sum().backward()
            return run

        new_step, old_step = train_step(one_pass), train_step(composed_aggregate)
        new_step()
        res_new = [X.grad.clone(), conv.weights_neigh.grad.clone()]
        old_step()
        res_old = [X.grad.clone(), conv.weights_neigh.grad.clone()]
        diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(res_new, res_old))
        t_new, t_old = _times([new_step, old_step], args.steps, args.warmup)
        print("%-14s layer D=%-4d N=%d E=%d | (d) PNAConv step: one pass %.3f ms | composition %.3f ms: ratio %.3f | "
              "max rel diff of the gradients %.2g | %.0f s" % (wl, D, N, E, t_new, t_old, t_new / t_old, diff, time.time() - t0),
              flush=True)
        del conv, X, G
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rd_like,community_loi,reddit")
    ap.add_argument("--dims", default="32,128")
    ap.add_argument("--layer", default="32")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per workload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r15", "multi_ab.log"))
    ap.add_argument("--step", default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as log:
        for wl in args.workloads.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", wl, "--dims", args.dims, "--layer", args.layer,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_timeout)
                out, rc = r.stdout, r.returncode
            except subprocess.TimeoutExpired as e:
                out, rc = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), 124
            print(out, end="", flush=True)
            log.write(out)
            log.flush()
            if rc != 0:
                msg = "step %s failed with status %d: stopping here\n" % (wl, rc)
                print(msg, end="", flush=True)
                log.write(msg)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
