"""Cost of the softmax aggregation on fp16 / bf16 features (include/hcspmm.h hcspmm_forward_softmax_typed,
hcspmm_softmax_backward_typed) against the fp32 launches on widened copies of the same inputs, on one
GPU, with tools/extremum16_ab.py's method: HIP events, median of --steps after --warmup, the variants alternated within one
process and the whole comparison repeated --runs times in that process.  Every variant rotates through enough copies of its
operands to cover 1 GiB (four times the 256 MiB Infinity Cache), as tools/update16_ab.py does.
  forward   (f32) forward_softmax with M and L;  (bf16), (fp16) forward_softmax16 with LSE -- what each backward needs
  backward  (f32) softmax_backward on G, Z, M, L, X;  (bf16), (fp16) softmax_backward16 on G16, Z16, LSE, X16
The backward walks the workload's own graph: it is a function of its operands on any graph, and the timing does not need the
transpose.  Nothing here is a merge condition: the figures are recorded.

Every workload is a step of its own: a child process under its own time limit; the run stops at the first step that fails.
The parent never opens the GPU.

  python tools/softmax16_ab.py [--workloads reddit,rd_like] [--dims 32,128,256] [--runs 3] [--log FILE]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "tools")]
GIB = 1 << 30


def _rotating(call, operands):
    """call(*one copy of operands) per invocation, over enough copies to cover 1 GiB"""
    n = max(2, -(-GIB // sum(t.numel() * t.element_size() for t in operands)))
    copies = [operands] + [tuple(t.clone() for t in operands) for _ in range(n - 1)]
    state = {"k": 0}

    def fn():
        state["k"] = (state["k"] + 1) % n
        return call(*copies[state["k"]])

    return fn, n


def step(args, wl):
    import torch
    import bench
    import hcspmm
    from gat_ab import _times
    dev = torch.device("cuda:0")
    n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
    rp, col = bench.make_local_block(wl, n_local, e_local, vw, 0)
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=32))
    types = (("bf16", torch.bfloat16), ("fp16", torch.float16))
    for D in [int(d) for d in args.dims.split(",") if d]:
        t0 = time.time()
        X = torch.randn(N, D, device=dev).to(torch.bfloat16).float()  # (bf16 holds it exactly; the fp16 copy rounds once more)
        G = torch.randn(N, D, device=dev)
        Z, M, L, _ = hcspmm.forward_softmax(X, 1.0, *g, return_stats=("M", "L"))
        fwd = [_rotating(lambda x: hcspmm.forward_softmax(x, 1.0, *g, return_stats=("M", "L")), (X,))]
        bwd = [_rotating(lambda a, b, c, d, e: hcspmm.softmax_backward(a, b, c, d, e, 1.0, *g), (G, Z, M, L, X))]
        for _, dt in types:
            x16 = X.to(dt)
            z16, lse, _ = hcspmm.forward_softmax16(x16, 1.0, *g)
            fwd.append(_rotating(lambda x: hcspmm.forward_softmax16(x, 1.0, *g), (x16,)))
            bwd.append(_rotating(lambda a, b, c, d: hcspmm.softmax_backward16(a, b, c, d, 1.0, *g), (G.to(dt), z16, lse, x16)))
        for what, fns in (("forward", fwd), ("backward", bwd)):
            runs = [_times([f for f, _ in fns], args.steps, args.warmup) for _ in range(args.runs)]
            mean = [sum(r[k] for r in runs) / len(runs) for k in range(3)]
            cells = ["(%s x%d) %.4f ms [%.4f, %.4f]" % (name, fns[k][1], mean[k], min(r[k] for r in runs), max(r[k] for r in runs))
                     for k, name in enumerate(("f32", "bf16", "fp16"))]
            print("%-8s %-8s D=%-4d N=%d E=%d | %s | f32/bf16 %.3f f32/fp16 %.3f | f32 max/min over runs %.3f | %.0f s"
                  % (wl, what, D, N, E, " | ".join(cells), mean[0] / mean[1], mean[0] / mean[2],
                     max(r[0] for r in runs) / min(r[0] for r in runs), time.time() - t0), flush=True)
        del fwd, bwd, X, G, Z, M, L
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="reddit,rd_like")
    ap.add_argument("--dims", default="32,128,256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of the whole comparison inside one process")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per workload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r26", "softmax16_ab.log"))
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
