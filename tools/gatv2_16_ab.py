"""Cost of the GATv2 attention on bf16 / fp16 node rows (include/hcspmm.h hcspmm_gatv2_scores_typed,
hcspmm_gatv2_scores_backward_typed) against the fp32 launches (section 3.13) on widened copies of the same
operands, on one GPU, with tools/heads16_ab.py's method: HIP events, median of --steps after --warmup, the sides alternated step by
step within one process.  Per workload (made pattern-symmetric where it is not: A + A^T) and heads x Dh, three comparisons: the
scores launch, the backward (two row launches and the fold) with 16-bit node gradients, and the backward with fp32 node gradients.
Every fp32 yardstick is also run against itself (a second copy of the same call in the alternation): a ratio counts as a gain or a
loss only beyond that self-ratio and the yardstick's spread over --runs repetitions.  Nothing here is a merge condition: the figures
are recorded.

Every workload is a step of its own: a child process under its own time limit; the run stops at the first step that fails.  The
parent never opens the GPU.

  python tools/gatv2_16_ab.py [--workloads reddit,rd_like,community_loi,dense] [--shapes 1x32,4x16,8x8,4x32] [--dtype bf16] [--log FILE]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel"), os.path.join(ROOT, "tools")]
SLOPE = 0.2


def _line(wl, shape, what, names, runs):
    """names[0] and names[1] are the yardstick and its repeat"""
    mean = [sum(r[k] for r in runs) / len(runs) for k in range(len(names))]
    cells = ["(%s) %.4f ms [%.4f, %.4f]" % (names[k], mean[k], min(r[k] for r in runs), max(r[k] for r in runs)) for k in range(len(names))]
    ratios = " ".join("f32/%s %.3f" % (names[k], mean[0] / mean[k]) for k in range(1, len(names)))
    print("%-13s %-5s %-8s | %s | %s | f32 max/min over runs %.3f" % (wl, shape, what, " | ".join(cells), ratios,
                                                                    max(r[0] for r in runs) / min(r[0] for r in runs)), flush=True)


def step(args, wl):
    import torch
    import bench
    import hcspmm
    from gat_ab import _symmetric, _times
    dev = torch.device("cuda:0")
    lo = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
    rp, col = _symmetric(*bench.make_local_block(wl, n_local, e_local, vw, 0))
    N, E = len(rp) - 1, len(col)
    rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
    perm = hcspmm.transpose_permutation(rp_d, col_d).int()
    print("%-13s N %d E %d (symmetrised), %s against fp32" % (wl, N, E, args.dtype), flush=True)
    for shape in args.shapes.split(","):
        heads, dh = (int(v) for v in shape.split("x"))
        D = heads * dh
        h16 = torch.randn(N, 2 * D, device=dev).to(lo)  # [H_src | H_dst]: the halves of one projection, as the layer passes them
        h32 = h16.float()
        s16, d16, s32, d32 = h16[:, :D], h16[:, D:], h32[:, :D], h32[:, D:]
        att, gl = torch.randn(heads, dh, device=dev), torch.randn(heads, E, device=dev)
        f_scores = lambda: hcspmm.gatv2_scores(d32, s32, att, rp_d, col_d, SLOPE)
        f_back = lambda: hcspmm.gatv2_scores_backward(gl, d32, s32, att, rp_d, col_d, perm, SLOPE)
        fns = (("scores", ("f32", "f32'", args.dtype), [f_scores, f_scores, lambda: hcspmm.gatv2_scores16(d16, s16, att, rp_d, col_d, SLOPE)]),
               ("backward", ("f32", "f32'", "g16", "g32"),
                [f_back, f_back, lambda: hcspmm.gatv2_scores_backward16(gl, d16, s16, att, rp_d, col_d, perm, SLOPE),
                 lambda: hcspmm.gatv2_scores_backward16(gl, d16, s16, att, rp_d, col_d, perm, SLOPE, grad_dtype=torch.float32)]))
        for what, names, f in fns:
            _line(wl, shape, what, names, [_times(f, args.steps, args.warmup) for _ in range(args.runs)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="reddit,rd_like,community_loi,dense")
    ap.add_argument("--shapes", default="1x32,4x16,8x8,4x32")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of the whole comparison inside one process")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per workload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r30", "gatv2_16_ab.log"))
    ap.add_argument("--step", default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as log:
        log.write("library: %s\n" % (os.environ.get("HCSPMM_LIB") or "csrc/libhcspmm.so"))
        for wl in args.workloads.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", wl, "--shapes", args.shapes, "--dtype", args.dtype, "--steps",
                   str(args.steps), "--warmup", str(args.warmup), "--runs", str(args.runs)]
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
