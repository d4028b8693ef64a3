"""Cost of the edge-feature messages on fp16 / bf16 operands (include/hcspmm.h hcspmm_forward_edge_messages_typed,
hcspmm_edge_messages_grad_typed) against the fp32 launches (section 3.16) on widened copies of the same
inputs, on one GPU, with tools/multi16_ab.py's method: HIP events, median of --steps after --warmup, the variants alternated
within one process and the whole comparison repeated --runs times in that process, so that a ratio can be held against the spread
of the fp32 runs.  Per workload and width: the forward of every op (direct form, F [E, D] read once) and the gradient with
respect to F of every op.  F and grad_F are E x D: from D = 32 on every copy is larger than the 256 MiB Infinity Cache on both
graphs, so no call finds its F rows where the previous one left them; X ([N, D], reused across a row's neighbours) is not rotated.
A width whose fp32 F would pass --max-f-gib is run on the first entries of the graph's rows that fit, and the line says so.
Nothing here is a merge condition: the figures are recorded.  From bytes alone the forward reads 4 instead of 8 bytes per entry
and column, the gradient moves 6 - 8 instead of 12 - 16.

Every workload is a step of its own: a child process under its own time limit; the run stops at the first step that fails.
The parent never opens the GPU.

  python tools/edge16_ab.py [--workloads reddit,rd_like] [--dims 32,128,256] [--runs 3] [--log FILE]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "tools")]
GIB = 1 << 30
OPS = ("mul", "add_relu", "copy")


def step(args, wl):
    import numpy as np
    import torch
    import bench
    import hcspmm
    from gat_ab import _times
    dev = torch.device("cuda:0")
    n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
    rp, col = bench.make_local_block(wl, n_local, e_local, vw, 0)
    for D in [int(d) for d in args.dims.split(",") if d]:
        t0 = time.time()
        n_rows = len(rp) - 1
        if int(rp[-1]) * D * 4 > args.max_f_gib * GIB:  # the leading rows whose entries fit (column ids keep indexing all of X)
            n_rows = int(np.searchsorted(rp, args.max_f_gib * GIB // (4 * D), side="right")) - 1
        rp_k, col_k = rp[:n_rows + 1], col[:rp[n_rows]]
        N, E, x_rows = n_rows, len(col_k), len(rp) - 1
        rp_d, col_d = torch.from_numpy(rp_k.copy()).to(dev), torch.from_numpy(col_k.copy()).to(dev)
        g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=32, num_columns=x_rows))
        ops = {}
        for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            ops[name] = tuple(torch.randn(s, device=dev).to(dt) for s in ((x_rows, D), (E, D), (N, D)))
        ops["f32"] = tuple(t.float() for t in ops["bf16"])
        order = ("f32", "bf16", "fp16")
        for kind in ("forward", "grad_F"):
            for op in OPS:
                if kind == "forward":
                    fns = [lambda X=ops[n][0], F=ops[n][1]: hcspmm.forward_edge_messages(X, F, *g, op=op) for n in order]
                else:
                    fns = [lambda X=ops[n][0], F=ops[n][1], G=ops[n][2]: hcspmm.edge_messages_grad(G, X, F, rp_d, col_d, op) for n in order]
                runs = [_times(fns, args.steps, args.warmup) for _ in range(args.runs)]
                mean = [sum(r[k] for r in runs) / len(runs) for k in range(3)]
                cells = ["(%s) %.4f ms [%.4f, %.4f]" % (order[k], mean[k], min(r[k] for r in runs), max(r[k] for r in runs))
                         for k in range(3)]
                print("%-8s D=%-4d N=%d E=%d%s %-7s %-8s | %s | f32/bf16 %.3f f32/fp16 %.3f | f32 max/min over runs %.3f"
                      % (wl, D, N, E, "" if n_rows == len(rp) - 1 else " (leading rows of %d)" % (len(rp) - 1), kind, op,
                         " | ".join(cells), mean[0] / mean[1], mean[0] / mean[2], max(r[0] for r in runs) / min(r[0] for r in runs)),
                      flush=True)
        print("%-8s D=%-4d %.0f s" % (wl, D, time.time() - t0), flush=True)
        del ops, fns, g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="reddit,rd_like")
    ap.add_argument("--dims", default="32,128,256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of the whole comparison inside one process")
    ap.add_argument("--max-f-gib", type=int, default=24, help="largest fp32 F [E, D] to allocate; beyond it the graph's leading rows are used")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds per workload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r28", "edge16_ab.log"))
    ap.add_argument("--step", default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as log:
        for wl in args.workloads.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", wl, "--dims", args.dims, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--runs", str(args.runs), "--max-f-gib", str(args.max_f_gib)]
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
