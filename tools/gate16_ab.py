"""Cost of the gated neighbour aggregation on fp16 / bf16 operands (include/hcspmm.h hcspmm_forward_gated_typed; DESIGN.md
section 3.21b) against the fp32 call on one GPU, with tools/gated_ab.py's method: HIP events, median of --steps after --warmup,
the variants alternated within one process and the whole comparison repeated --runs times in that process, so that a ratio can
be held against the spread of the fp32 runs.  Per workload (made pattern-symmetric where it is not) and width D, for the gate
alone and for gate + dgate:
  (f32) forward_gated on float32 operands;   (bf16), (fp16) the same call on the operands rounded to that type.
Nothing here is a merge condition: the figures are recorded.  The gathered bytes argue for up to 2 x; the 16-bit builds issue
twice the exponentials and reciprocals per gathered byte and may be bound by those instead.

Every workload is a step of its own: a child process under its own time limit; the run stops at the first step that fails.
The parent never opens the GPU.

  python tools/gate16_ab.py [--workloads rd_like,reddit] [--dims 32,128] [--runs 3] [--log FILE]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel"),
                os.path.join(ROOT, "tools")]
BOTH = ("gate", "dgate")


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
    for D in [int(d) for d in args.dims.split(",") if d]:
        t0 = time.time()
        ops = {torch.float32: (2.0 * torch.randn(N, D, device=dev), 2.0 * torch.randn(N, D, device=dev), torch.randn(N, D, device=dev))}
        for dt in (torch.bfloat16, torch.float16):
            ops[dt] = tuple(o.to(dt) for o in ops[torch.float32])
        Z = hcspmm.forward_gated(*ops[torch.float32], *g)[0]
        diff = [float((hcspmm.forward_gated(*ops[dt], *g)[0] - Z).abs().max()) for dt in (torch.bfloat16, torch.float16)]
        fns = [(lambda o=o, out=out: hcspmm.forward_gated(*o, *g, outputs=out)) for out in (("gate",), BOTH) for o in ops.values()]
        names = ["(%s) %s" % (n, "+".join(out)) for out in (("gate",), BOTH) for n in ("f32", "bf16", "fp16")]
        runs = [_times(fns, args.steps, args.warmup) for _ in range(args.runs)]
        cells = []
        for k in range(len(fns)):
            ts = [r[k] for r in runs]
            cells.append("%s %.4f ms [%.4f, %.4f]" % (names[k], sum(ts) / len(ts), min(ts), max(ts)))
        mean = [sum(r[k] for r in runs) / len(runs) for k in range(len(fns))]
        spread = ["%.3f" % (max(r[k] for r in runs) / min(r[k] for r in runs)) for k in (0, 3)]
        ratios = "gate f32/bf16 %.3f f32/fp16 %.3f | gate+dgate f32/bf16 %.3f f32/fp16 %.3f | f32 max/min over runs %s %s" % (
            mean[0] / mean[1], mean[0] / mean[2], mean[3] / mean[4], mean[3] / mean[5], spread[0], spread[1])
        print("%-10s D=%-4d N=%d E=%d | %s | %s | max |Z16 - Z32| bf16 %.1e fp16 %.1e | %.0f s"
              % (wl, D, N, E, " | ".join(cells), ratios, diff[0], diff[1], time.time() - t0), flush=True)
        del ops, Z
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rd_like,reddit")
    ap.add_argument("--dims", default="32,128")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of the whole comparison inside one process")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per workload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r23", "gate16_ab.log"))
    ap.add_argument("--step", default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as log:
        for wl in args.workloads.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", wl, "--dims", args.dims, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--runs", str(args.runs)]
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
