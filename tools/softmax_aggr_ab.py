"""Cost of the softmax neighbour aggregation (include/hcspmm.h hcspmm_forward_softmax / hcspmm_softmax_backward; DESIGN.md
section 3.18) on one GPU, timed with HIP events (median of --steps after --warmup), the variants alternated within one process
and the whole comparison repeated --runs times in that process, so that the spread stands next to the means.  Per workload
(made pattern-symmetric where it is not: A + A^T) and width D:
  (a) forward_softmax with Z, M, L, Q;      (a') with Z alone (return_stats=False);
  (b) softmax_backward on the same graph;
  (c) forward_multi with all six outputs: the same gathers, more state, no transcendental;
  (d) the binary forward: the gathers alone;
  (e) the torch composition of the forward (index_select + scatter_reduce + exp + two index_add), skipped where its [E, D]
      tensors would exceed --torch-bytes.
What is expected, and recorded rather than gated: (d) <= (a) <= (c)-ish, and (b) near four times the weighted forward's traffic.

Every workload is a step of its own: a child process under its own time limit; the run stops at the first step that fails.
The parent never opens the GPU.

  python tools/softmax_aggr_ab.py [--workloads rd_like,reddit] [--dims 32,128] [--runs 3] [--log FILE]
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
    from gat_ab import _symmetric, _times
    dev = torch.device("cuda:0")
    n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
    rp, col = _symmetric(*bench.make_local_block(wl, n_local, e_local, vw, 0))
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=32))
    rows = torch.repeat_interleave(torch.arange(N, device=dev), (rp_d[1:] - rp_d[:-1]).long())
    cols = col_d.long()

    def torch_forward(X, beta):
        src = X.index_select(0, cols)
        s = src * beta
        m = torch.full((N, X.size(1)), -float("inf"), device=dev).scatter_reduce(0, rows[:, None].expand_as(s), s, "amax")
        w = torch.exp(s - m[rows])
        zero = torch.zeros(N, X.size(1), device=dev)
        return zero.index_add(0, rows, w * src) / zero.index_add(0, rows, w).clamp_min(1e-30)

    for D in [int(d) for d in args.dims.split(",") if d]:
        t0 = time.time()
        X = torch.randn(N, D, device=dev)
        G = torch.randn(N, D, device=dev)
        beta = torch.full((D,), 1.0, device=dev)
        Z, M, L, Q = hcspmm.forward_softmax(X, beta, *g)
        with_torch = E * D * 4 <= args.torch_bytes
        diff = float((Z - torch_forward(X, beta)).abs().max()) if with_torch else float("nan")
        fns = [lambda: hcspmm.forward_softmax(X, beta, *g), lambda: hcspmm.forward_softmax(X, beta, *g, return_stats=False),
               lambda: hcspmm.softmax_backward(G, Z, M, L, X, beta, *g), lambda: hcspmm.forward_multi(X, *g),
               lambda: hcspmm.forward(X, *g)]
        if with_torch:
            fns.append(lambda: torch_forward(X, beta))
        runs = [_times(fns, args.steps, args.warmup) for _ in range(args.runs)]
        names = ["(a) forward_softmax", "(a') Z alone", "(b) softmax_backward", "(c) forward_multi", "(d) forward", "(e) torch"]
        cells = []
        for k in range(len(fns)):
            ts = [r[k] for r in runs]
            cells.append("%s %.4f ms [%.4f, %.4f]" % (names[k], sum(ts) / len(ts), min(ts), max(ts)))
        mean = [sum(r[k] for r in runs) / len(runs) for k in range(len(fns))]
        print("%-10s D=%-4d N=%d E=%d | %s | (a)/(d) %.3f (a)/(c) %.3f (b)/(d) %.3f | max |Z - torch| %.1e | %.0f s"
              % (wl, D, N, E, " | ".join(cells), mean[0] / mean[4], mean[0] / mean[3], mean[2] / mean[4], diff, time.time() - t0),
              flush=True)
        del X, G, Z, M, L, Q
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rd_like,reddit")
    ap.add_argument("--dims", default="32,128")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of the whole comparison inside one process")
    ap.add_argument("--torch-bytes", type=int, default=8 << 30, help="largest [E, D] float32 tensor the torch composition may make")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per workload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r17", "softmax_aggr_ab.log"))
    ap.add_argument("--step", default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as log:
        for wl in args.workloads.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", wl, "--dims", args.dims, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--runs", str(args.runs), "--torch-bytes", str(args.torch_bytes)]
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
