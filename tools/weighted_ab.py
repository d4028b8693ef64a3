"""Cost of the edge weights (include/hcspmm.h hcspmm_forward_weighted) on one GPU: per workload the binary
forward, the weighted forward with random values and with values == 1, and torch.sparse.mm on a CSR tensor carrying the same
values (on the fp32 copy of 16-bit X), timed with HIP events (median of --steps launches after --warmup).  The weighted results are checked on the way:
values == 1 against the binary forward bit for bit, random values against torch.sparse.mm within 1e-5 of sum |v x|
(plus one 16-bit rounding).

  python tools/weighted_ab.py [--workloads reddit:128:f32,community_loi:32:f32,dense:32:f32,reddit:128:bf16] [--steps 50]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd")]


def _time(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="reddit:128:f32,community_loi:32:f32,dense:32:f32,reddit:128:bf16")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import hcspmm
    dev = torch.device("cuda:0")
    dtypes = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    for spec in args.workloads.split(","):
        wl, D, dt = spec.split(":")
        D, dt = int(D), dtypes[dt]
        t0 = time.time()
        n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
        rp, col = bench.make_local_block(wl, n_local, e_local, vw, 0)
        N, E = len(rp) - 1, len(col)
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        graph = hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=D)
        X = torch.randn(N, D, device=dev).to(dt)
        vals = torch.rand(E, device=dev) + 0.5
        ones = torch.ones(E, device=dev)
        zb = hcspmm.forward(X, rp_d, col_d, *graph)[0]
        z1 = hcspmm.forward_weighted(X, ones, rp_d, col_d, *graph)[0]
        assert torch.equal(z1, zb), "values == 1 differ from the binary forward"
        zw = hcspmm.forward_weighted(X, vals, rp_d, col_d, *graph)[0]
        A = torch.sparse_csr_tensor(rp_d.long(), col_d.long(), vals, (N, N))
        # 16-bit features: torch.sparse.mm runs on the fp32 copy of X (a bf16 CSR product ended the process with an uncaught
        # host exception on this stack); the weighted result is checked against it to within one 16-bit rounding
        Xs = X if dt == torch.float32 else X.float()
        ref = torch.sparse.mm(A, Xs)
        bound = torch.sparse.mm(A, Xs.abs()) * 1e-5 + (0 if dt == torch.float32 else ref.abs() * 2 ** -7)
        err = ((zw.float() - ref).abs() - bound).max().item()
        assert err <= 0, "weighted forward off torch.sparse.mm by %g beyond the bar" % err
        t_sp = _time(lambda: torch.sparse.mm(A, Xs), args.steps, args.warmup)
        t_b = _time(lambda: hcspmm.forward(X, rp_d, col_d, *graph), args.steps, args.warmup)
        t_w = _time(lambda: hcspmm.forward_weighted(X, vals, rp_d, col_d, *graph), args.steps, args.warmup)
        t_1 = _time(lambda: hcspmm.forward_weighted(X, ones, rp_d, col_d, *graph), args.steps, args.warmup)
        print("%-14s D=%-4d %-5s N=%d E=%d | binary %.4f ms | weighted %.4f ms (%.3fx) | ones %.4f ms (%.3fx) | "
              "torch.sparse.mm%s %.4f ms (weighted %.2fx faster) | check %.3g | %.0f s"
              % (wl, D, str(dt).replace("torch.", ""), N, E, t_b, t_w, t_w / t_b, t_1, t_1 / t_b, "" if dt == torch.float32 else "(fp32 X)", t_sp, t_sp / t_w, err,
                 time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
