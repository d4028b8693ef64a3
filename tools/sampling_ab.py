"""Cost of a per-epoch neighbour sample built on the device (include/hcspmm.h hcspmm_sample_neighbors_device,
hcspmm_transpose_graph_device) on one GPU.  Device work is timed with HIP events (median of --steps
after --warmup, the variants alternated within one process), host work with a host clock around a synchronise (median of
--host-runs); the whole comparison is repeated --runs times in the process so that the spread stands next to the means.
Per workload, fanout K and the workload's width D:
  (a) sample_neighbors with the kept row_pointers_s;          (a0) sample_row_pointers, once per (graph, K);
  (b) transpose_graph_device of the sample;
  (c) forward on the sampled graph, plan-free (plan_free_graph);   (c') the same on its transpose (the backward's aggregation);
  (d) forward on the FULL graph with its plan -- code this feature does not touch;
  (e) what the sample would cost through the host: transpose_graph, and preprocess of the sample;
  (f) forward on the sampled graph with the plan that (e) built: what the plan-free path gives away.
Recorded, not gated: (a) + (b) against (e), and one sampled aggregation pair (a) + (b) + (c) + (c') against the full pair 2 x (d).

Every workload is a step of its own: a child process under its own time limit; the run stops at the first step that fails.
The parent never opens the GPU.

  python tools/sampling_ab.py [--workloads reddit,rd_like] [--fanouts 10,25] [--runs 3] [--log FILE]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel"),
                os.path.join(ROOT, "tools")]


def _host_ms(fn, runs):
    import torch
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def step(args, wl):
    import numpy as np
    import torch
    import bench
    import hcspmm
    from gat_ab import _times
    dev = torch.device("cuda:0")
    n_local, e_local, D, vw, _ = bench.WORKLOADS[wl]
    rp, col = bench.make_local_block(wl, n_local, e_local, vw, 0)
    N, E = len(rp) - 1, len(col)
    deg = np.diff(rp)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=D))
    X = torch.randn(N, D, device=dev)
    for K in [int(k) for k in args.fanouts.split(",") if k]:
        t0 = time.time()
        rp_s = hcspmm.sample_row_pointers(rp_d, K)
        _, col_s, eid_s = hcspmm.sample_neighbors(rp_d, col_d, K, 0, rp_s)
        g_s = hcspmm.plan_free_graph(rp_s, col_s)
        rp_t, col_t, eid_t = hcspmm.transpose_graph_device(rp_s, col_s)
        g_t = hcspmm.plan_free_graph(rp_t, col_t)
        E_s = col_s.numel()
        # the device transpose is the host one, and the plan-free product is the planned one (the 1e-5 bar of the suite)
        host_t = hcspmm.transpose_graph(rp_s, col_s)
        same = all(torch.equal(a, b) for a, b in zip((rp_t, col_t, eid_t), host_t))
        planned = (rp_s, col_s) + tuple(hcspmm.preprocess(col_s, rp_s, N, E_s, (N + 15) // 16, dim=D))
        Z_free, Z_plan = hcspmm.forward(X, *g_s)[0], hcspmm.forward(X, *planned)[0]
        diff = float((Z_free - Z_plan).abs().max() / Z_plan.abs().max())
        seeds = iter(range(1, 1 << 30))
        fns = [lambda: hcspmm.sample_neighbors(rp_d, col_d, K, next(seeds), rp_s), lambda: hcspmm.sample_row_pointers(rp_d, K),
               lambda: hcspmm.transpose_graph_device(rp_s, col_s), lambda: hcspmm.forward(X, *g_s), lambda: hcspmm.forward(X, *g_t),
               lambda: hcspmm.forward(X, *g), lambda: hcspmm.forward(X, *planned)]
        names = ["(a) sample_neighbors", "(a0) sample_row_pointers", "(b) transpose_graph_device", "(c) forward sampled plan-free",
                 "(c') forward sampled^T plan-free", "(d) forward full planned", "(f) forward sampled planned"]
        runs = [_times(fns, args.steps, args.warmup) for _ in range(args.runs)]
        host = [(_host_ms(lambda: hcspmm.transpose_graph(rp_s, col_s), args.host_runs),
                 _host_ms(lambda: hcspmm.preprocess(col_s, rp_s, N, E_s, (N + 15) // 16, dim=D), args.host_runs))
                for _ in range(args.runs)]
        cells = []
        for k in range(len(fns)):
            ts = [r[k] for r in runs]
            cells.append("%s %.4f ms [%.4f, %.4f]" % (names[k], sum(ts) / len(ts), min(ts), max(ts)))
        for k, name in enumerate(("(e) host transpose_graph", "(e) host preprocess")):
            ts = [h[k] for h in host]
            cells.append("%s %.3f ms [%.3f, %.3f]" % (name, sum(ts) / len(ts), min(ts), max(ts)))
        m = [sum(r[k] for r in runs) / len(runs) for k in range(len(fns))]
        e_host = sum(h[0] + h[1] for h in host) / len(host)
        print("%-8s K=%-3d D=%-4d N=%d E=%d E_s=%d rows beyond K: %d, beyond %d: %d, max in-degree of the sample %d | %s | "
              "(a)+(b) %.4f ms vs (e) %.3f ms | sampled pair (a)+(b)+(c)+(c') %.4f ms vs full pair 2(d) %.4f ms | "
              "transpose equals host: %s | plan-free vs planned rel. diff %.1e | %.0f s"
              % (wl, K, D, N, E, E_s, int((deg > K).sum()), hcspmm.SAMPLE_WAVE_ROW_MAX, int((deg > max(K, hcspmm.SAMPLE_WAVE_ROW_MAX)).sum()),
                 int((rp_t[1:] - rp_t[:-1]).max()), " | ".join(cells), m[0] + m[2], e_host, m[0] + m[2] + m[3] + m[4], 2 * m[5],
                 same, diff, time.time() - t0), flush=True)
        if not same:
            raise SystemExit("the device transpose differs from the host transpose")
        del rp_s, col_s, eid_s, g_s, rp_t, col_t, eid_t, g_t, planned, Z_free, Z_plan
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="reddit,rd_like")
    ap.add_argument("--fanouts", default="10,25")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of the whole comparison inside one process")
    ap.add_argument("--host-runs", type=int, default=3, help="repetitions of each host-timed call")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per workload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r19", "sampling_ab.log"))
    ap.add_argument("--step", default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as log:
        for wl in args.workloads.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", wl, "--fanouts", args.fanouts, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--runs", str(args.runs), "--host-runs", str(args.host_runs)]
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
