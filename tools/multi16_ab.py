"""Cost of the one-pass sum / sumsq / max / min aggregation on fp16 / bf16 features (include/hcspmm.h hcspmm_forward_multi_typed;
DESIGN.md section 3.17b) against the fp32 launch (hcspmm_forward_multi, section 3.17) on widened copies of the same inputs, on
one GPU, with tools/extremum16_ab.py's method: HIP events, median of --steps after --warmup, the variants alternated within one
process and the whole comparison repeated --runs times in that process, so that a ratio can be held against the spread of the
fp32 runs.  Every variant rotates through enough copies of its X to cover 1 GiB (four times the 256 MiB Infinity Cache), so no
call finds its rows where the previous one left them.  All six outputs are asked of every variant.
  (f32) forward_multi on float32 X;   (bf16), (fp16) forward_multi16 on X rounded to that type (both args checked equal to the
  fp32 args of the widened copy before anything is timed).
Nothing here is a merge condition: the figures are recorded.  From bytes alone the gathers halve and the stores go from 24 to
20 bytes per element.

Every workload is a step of its own: a child process under its own time limit; the run stops at the first step that fails.
The parent never opens the GPU.

  python tools/multi16_ab.py [--workloads reddit,rd_like] [--dims 32,128,256] [--runs 3] [--log FILE]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "tools")]
GIB = 1 << 30


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
    for D in [int(d) for d in args.dims.split(",") if d]:
        t0 = time.time()
        X16 = {dt: torch.randn(N, D, device=dev).to(dt) for dt in (torch.bfloat16, torch.float16)}
        for dt, x in X16.items():  # the winners are the fp32 kernel's on the widened copy
            a, b = hcspmm.forward_multi16(x, *g), hcspmm.forward_multi(x.float(), *g)
            assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]), (wl, D, dt)
            del a, b
        fns, names = [], []
        for name, x in (("f32", X16[torch.bfloat16].float()), ("bf16", X16[torch.bfloat16]), ("fp16", X16[torch.float16])):
            copies = [x] + [x.clone() for _ in range(max(1, -(-GIB // (x.numel() * x.element_size()))) - 1)]
            state = {"k": 0}
            call = hcspmm.forward_multi if name == "f32" else hcspmm.forward_multi16

            def fn(copies=copies, state=state, call=call):
                state["k"] = (state["k"] + 1) % len(copies)
                return call(copies[state["k"]], *g)

            fns.append(fn)
            names.append("(%s x%d)" % (name, len(copies)))
        runs = [_times(fns, args.steps, args.warmup) for _ in range(args.runs)]
        mean = [sum(r[k] for r in runs) / len(runs) for k in range(3)]
        cells = ["%s %.4f ms [%.4f, %.4f]" % (names[k], mean[k], min(r[k] for r in runs), max(r[k] for r in runs)) for k in range(3)]
        print("%-8s D=%-4d N=%d E=%d | %s | f32/bf16 %.3f f32/fp16 %.3f | f32 max/min over runs %.3f | %.0f s"
              % (wl, D, N, E, " | ".join(cells), mean[0] / mean[1], mean[0] / mean[2],
                 max(r[0] for r in runs) / min(r[0] for r in runs), time.time() - t0), flush=True)
        del X16, fns
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="reddit,rd_like")
    ap.add_argument("--dims", default="32,128,256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of the whole comparison inside one process")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per workload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r27", "multi16_ab.log"))
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
