"""Cost of the kernels that produce and differentiate edge values (include/hcspmm.h hcspmm_sddmm, hcspmm_edge_softmax*;
DESIGN.md section 3.9) on one GPU, timed with HIP events (median of --steps launches after --warmup).  Per workload:
  * SDDMM, forward_weighted on the same graph and D (it moves about the same bytes per entry), and the torch formulation
    (A[rows] * B[cols]).sum(1) (on fp32 copies of 16-bit operands);
  * edge softmax forward + backward against a torch scatter formulation;
and, on the RD-sized graph, one GAT layer step (forward + backward, GNN_model.GATConv) against the same layer in plain torch.
The SDDMM and softmax results are checked against their torch formulations on the way.

  python tools/sddmm_ab.py [--workloads reddit:128:f32,rd_like:32:f32,...] [--steps 50] [--warmup 10]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel")]

DEFAULT = "reddit:128:f32,rd_like:32:f32,community_loi:32:f32,dense:32:f32,reddit:128:bf16"


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


def _torch_softmax(x, rows, N):
    import torch
    m = torch.full((N,), -float("inf"), device=x.device).scatter_reduce(0, rows, x, "amax")
    ex = torch.exp(x - m[rows])
    return ex / torch.zeros(N, device=x.device).index_add(0, rows, ex)[rows]


def _torch_softmax_bwd(alpha, g, rows, N):
    import torch
    return alpha * (g - torch.zeros(N, device=alpha.device).index_add(0, rows, alpha * g)[rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=DEFAULT)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--gat", default="rd_like", help="workload of the GAT layer comparison ('' skips it)")
    args = ap.parse_args()
    import torch
    import bench
    import hcspmm
    dev = torch.device("cuda:0")
    dtypes = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    cache = {}

    def graph_of(wl, D):
        if wl not in cache:
            cache.clear()
            n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
            rp, col = bench.make_local_block(wl, n_local, e_local, vw, 0)
            N, E = len(rp) - 1, len(col)
            rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
            rows = torch.repeat_interleave(torch.arange(N, device=dev), (rp_d[1:] - rp_d[:-1]).long())
            cache[wl] = (N, E, rp_d, col_d, rows)
        N, E, rp_d, col_d, rows = cache[wl]
        return N, E, rp_d, col_d, rows, hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=D)

    for spec in args.workloads.split(","):
        wl, D, dt = spec.split(":")
        D, dt = int(D), dtypes[dt]
        t0 = time.time()
        N, E, rp_d, col_d, rows, graph = graph_of(wl, D)
        cols = col_d.long()
        A = torch.randn(N, D, device=dev).to(dt)
        B = torch.randn(N, D, device=dev).to(dt)
        vals = torch.rand(E, device=dev)
        got = hcspmm.sddmm(A, B, rp_d, col_d, *graph)
        Af, Bf = A.float(), B.float()
        ref = (Af[rows] * Bf[cols]).sum(1)
        bound = (Af[rows].abs() * Bf[cols].abs()).sum(1) * (D + 1) * 2.0 ** -23
        err = ((got - ref).abs() - bound).max().item()
        assert err <= 0, "sddmm off the torch formulation by %g beyond the bar" % err
        del ref, bound
        t_sd = _time(lambda: hcspmm.sddmm(A, B, rp_d, col_d, *graph), args.steps, args.warmup)
        t_fw = _time(lambda: hcspmm.forward_weighted(A, vals, rp_d, col_d, *graph), args.steps, args.warmup)
        t_ts = _time(lambda: (Af[rows] * Bf[cols]).sum(1), max(5, args.steps // 5), 2)
        line = ("%-14s D=%-4d %-8s N=%d E=%d | sddmm %.4f ms | forward_weighted %.4f ms (sddmm %.3fx) | torch%s %.4f ms "
                "(sddmm %.2fx faster) | check %.3g"
                % (wl, D, str(dt).replace("torch.", ""), N, E, t_sd, t_fw, t_sd / t_fw, "" if dt == torch.float32 else "(fp32)",
                   t_ts, t_ts / t_sd, err))
        if dt == torch.float32:
            logits = torch.rand(E, device=dev) * 160 - 80
            ga = torch.randn(E, device=dev)
            alpha = hcspmm.edge_softmax(logits, rp_d)
            a_ref = _torch_softmax(logits, rows, N)
            sm_err = ((alpha - a_ref).abs() / a_ref.clamp_min(1e-30)).max().item()
            t_sm = _time(lambda: hcspmm.edge_softmax(logits, rp_d), args.steps, args.warmup)
            t_smb = _time(lambda: hcspmm.edge_softmax_backward(alpha, ga, rp_d), args.steps, args.warmup)
            t_tsm = _time(lambda: _torch_softmax(logits, rows, N), max(5, args.steps // 5), 2)
            t_tsmb = _time(lambda: _torch_softmax_bwd(alpha, ga, rows, N), max(5, args.steps // 5), 2)
            line += (" | softmax %.4f ms vs torch %.4f ms (%.2fx faster), backward %.4f ms vs torch %.4f ms (%.2fx faster), "
                     "max rel diff %.2g" % (t_sm, t_tsm, t_tsm / t_sm, t_smb, t_tsmb, t_tsmb / t_smb, sm_err))
        print(line + " | %.0f s" % (time.time() - t0), flush=True)

    if args.gat:
        import GNN_model
        D = 32
        N, E, rp_d, col_d, rows, graph = graph_of(args.gat, D)
        cols = col_d.long()
        g = (rp_d, col_d) + tuple(graph)
        torch.manual_seed(0)
        conv = GNN_model.GATConv(D, D, 0, heads=1).to(dev)
        X = torch.randn(N, D, device=dev, requires_grad=True)
        G = torch.randn(N, D, device=dev)

        def lib_step():
            (conv(X, *g, None) * G).sum().backward()

        W, a_src, a_dst = conv.weights, conv.a_src, conv.a_dst

        def torch_step():
            h = X @ W[0]
            logit = torch.nn.functional.leaky_relu((h @ a_dst[0])[rows] + (h @ a_src[0])[cols], conv.negative_slope)
            alpha = _torch_softmax(logit, rows, N)
            out = torch.zeros(N, D, device=dev).index_add(0, rows, alpha[:, None] * h[cols])
            (out * G).sum().backward()

        t_lib = _time(lib_step, max(5, args.steps // 5), 3)
        t_torch = _time(torch_step, max(5, args.steps // 5), 3)
        print("GAT layer step (forward + backward, heads 1, D %d -> %d) on %s N=%d E=%d | library %.4f ms | plain torch %.4f ms "
              "(library %.2fx faster)" % (D, D, args.gat, N, E, t_lib, t_torch, t_torch / t_lib), flush=True)


if __name__ == "__main__":
    main()
