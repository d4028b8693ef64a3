"""Cost of the gated neighbour aggregation (include/hcspmm.h hcspmm_forward_gated) on one GPU, timed
with HIP events (median of --steps after --warmup), the variants alternated within one process and the whole comparison
repeated --runs times in that process, so that the spread stands next to the means.  Per workload (made pattern-symmetric
where it is not: A + A^T) and width D:
  (g1) forward_gated with Z_gate alone;       (g2) with Z_gate and Z_dgate (what a training step's two passes launch);
  (a)  fp32 forward_weighted on the same plan: ONE gather per entry, the floor for this schedule;
  (b)  today's composition: F = sigmoid(P[rows] + Q[col]) as an [E, D] tensor in torch, then forward_edge_messages(V, F, "mul"):
       (b) with the build of F in the timed region, (b') the launch alone on a prebuilt F.  Skipped where F would exceed
       --torch-bytes.
Nothing here is a merge condition: the figures are recorded.  The expectation is that (b) moves more than twice the bytes of (g1)
and loses.

Every workload is a step of its own: a child process under its own time limit; the run stops at the first step that fails.
The parent never opens the GPU.

  python tools/gated_ab.py [--workloads rd_like,reddit] [--dims 32,128] [--runs 3] [--log FILE]
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
    ones = torch.ones(E, device=dev)

    def build_f(P, Q):
        return torch.sigmoid(P.index_select(0, rows) + Q.index_select(0, cols))

    for D in [int(d) for d in args.dims.split(",") if d]:
        t0 = time.time()
        P, Q = 2.0 * torch.randn(N, D, device=dev), 2.0 * torch.randn(N, D, device=dev)
        V = torch.randn(N, D, device=dev)
        Z = hcspmm.forward_gated(P, Q, V, *g)[0]
        with_torch = E * D * 4 <= args.torch_bytes
        fns = [lambda: hcspmm.forward_gated(P, Q, V, *g), lambda: hcspmm.forward_gated(P, Q, V, *g, outputs=("gate", "dgate")),
               lambda: hcspmm.forward_weighted(V, ones, *g)]
        diff = float("nan")
        if with_torch:
            F = build_f(P, Q)
            diff = float((Z - hcspmm.forward_edge_messages(V, F, *g, "mul")[0]).abs().max())
            fns += [lambda: hcspmm.forward_edge_messages(V, build_f(P, Q), *g, "mul"),
                    lambda: hcspmm.forward_edge_messages(V, F, *g, "mul")]
        runs = [_times(fns, args.steps, args.warmup) for _ in range(args.runs)]
        names = ["(g1) gate", "(g2) gate + dgate", "(a) forward_weighted", "(b) F build + edge_messages", "(b') edge_messages"]
        cells = []
        for k in range(len(fns)):
            ts = [r[k] for r in runs]
            cells.append("%s %.4f ms [%.4f, %.4f]" % (names[k], sum(ts) / len(ts), min(ts), max(ts)))
        mean = [sum(r[k] for r in runs) / len(runs) for k in range(len(fns))]
        ratios = "(g1)/(a) %.3f (g2)/(g1) %.3f" % (mean[0] / mean[2], mean[1] / mean[0])
        if with_torch:
            ratios += " (b)/(g1) %.3f (b')/(g1) %.3f" % (mean[3] / mean[0], mean[4] / mean[0])
        print("%-10s D=%-4d N=%d E=%d | %s | %s | max |Z - composition| %.1e | %.0f s"
              % (wl, D, N, E, " | ".join(cells), ratios, diff, time.time() - t0), flush=True)
        del P, Q, V, Z
        if with_torch:
            del F
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rd_like,reddit")
    ap.add_argument("--dims", default="32,128")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of the whole comparison inside one process")
    ap.add_argument("--torch-bytes", type=int, default=8 << 30, help="largest [E, D] float32 tensor the composition may make")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per workload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r22", "gated_ab.log"))
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
