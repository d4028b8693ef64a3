"""Cost of the GATv2 attention kernels (include/hcspmm.h hcspmm_gatv2_scores / hcspmm_gatv2_scores_backward; DESIGN.md
section 3.13) on one GPU, timed with HIP events (median of --steps after --warmup), the two sides of every comparison
alternated step by step within one process.  Per workload (made pattern-symmetric where it is not: A + A^T) and heads x Dh:
  * the yardsticks against themselves (two alternated series of sddmm_heads, and of forward_weighted_heads): the spread
    within which a ratio counts as "at the yardstick";
  * gatv2_scores against sddmm_heads at the same D and heads (the same gathers and stores, two more VALU operations per
    element), and against the plain-torch formulation (index_select + leaky_relu + sum);
  * gatv2_scores_backward (both row launches and the fold of the att partials) against two forward_weighted_heads
    launches at the same width (per side: the same row walk and gathers), and against torch autograd of the formulation;
  * one GATv2Conv step (forward + backward, 32 input features) against the same layer in plain torch.
The scores are checked against the torch formulation on the way.

  python tools/gatv2_ab.py [--workloads reddit,rd_like,community_loi,dense] [--shapes 1x32,4x16,8x8,4x32]
  python tools/gatv2_ab.py --only layer --workloads rd_like --shapes 4x16   (the layer step alone, for a profiler)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel"),
                os.path.join(ROOT, "tools")]

from gat_ab import _symmetric, _times  # noqa: E402

SLOPE = 0.2


def torch_scores(hd, hs, att, rows, cols):
    import torch
    heads, dh = att.shape
    e = torch.nn.functional.leaky_relu(hd.index_select(0, rows) + hs.index_select(0, cols), SLOPE)
    return (e * att.reshape(1, -1)).view(-1, heads, dh).sum(2).t()


def torch_softmax(x, rows, N):
    """[heads, E] -> per-row softmax with scatter ops"""
    import torch
    idx = rows.expand_as(x)
    m = torch.full((x.size(0), N), -float("inf"), device=x.device).scatter_reduce(1, idx, x, "amax")
    ex = torch.exp(x - m.gather(1, idx))
    return ex / torch.zeros((x.size(0), N), device=x.device).scatter_add(1, idx, ex).gather(1, idx)


def torch_layer(conv, X, rows, cols, N):
    """GATv2Conv(concat=True) in plain torch"""
    import torch
    heads, dh = conv.att.shape
    width = heads * dh
    h = X @ conv.weights
    h_src, h_dst = h[:, :width], h[:, width:]
    alpha = torch_softmax(torch_scores(h_dst, h_src, conv.att, rows, cols), rows, N)
    msg = alpha.t()[:, :, None] * h_src.index_select(0, cols).view(-1, heads, dh)
    return torch.zeros(N, heads, dh, device=X.device).index_add(0, rows, msg).view(N, width)


def _shapes(s):
    return [tuple(int(v) for v in x.split("x")) for x in s.split(",") if x]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="reddit,rd_like,community_loi,dense")
    ap.add_argument("--shapes", default="1x32,4x16,8x8,4x32")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=7, help="steps of the comparisons against plain torch")
    ap.add_argument("--only", choices=["layer"], default=None)
    args = ap.parse_args()
    import torch
    import bench
    import hcspmm
    import GNN_model
    dev = torch.device("cuda:0")
    for wl in args.workloads.split(","):
        t0 = time.time()
        n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
        rp, col = _symmetric(*bench.make_local_block(wl, n_local, e_local, vw, 0))
        N, E = len(rp) - 1, len(col)
        rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        rows = torch.repeat_interleave(torch.arange(N, device=dev), (rp_d[1:] - rp_d[:-1]).long())
        cols = col_d.long()
        g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=32))
        perm32 = GNN_model.transpose_permutation_i32(rp_d, col_d)
        print("%-14s N=%d E=%d longest row %d | graph ready in %.0f s" % (wl, N, E, int((rp_d[1:] - rp_d[:-1]).max()),
                                                                        time.time() - t0), flush=True)
        for heads, dh in _shapes(args.shapes):
            t0 = time.time()
            D = heads * dh
            torch.manual_seed(heads * 100 + dh)
            conv = GNN_model.GATv2Conv(32, dh, 0, heads=heads, concat=True).to(dev)
            X = torch.randn(N, 32, device=dev, requires_grad=True)
            G = torch.randn(N, D, device=dev)
            params = [X, conv.weights, conv.att]

            def step(fwd):
                def run():
                    for p in params:
                        p.grad = None
                    (fwd() * G).sum().backward()
                return run

            lib_step = step(lambda: conv(X, *g, None))
            torch_step = step(lambda: torch_layer(conv, X, rows, cols, N))
            if args.only:
                for _ in range(args.warmup + args.steps):
                    lib_step()
                torch.cuda.synchronize()
                print("layer %s %dx%d: %d steps done" % (wl, heads, dh, args.warmup + args.steps), flush=True)
                continue
            both = torch.randn(N, 2 * D, device=dev)  # the projection's two halves, as the layer passes them
            hs, hd = both[:, :D], both[:, D:]
            att = torch.rand(heads, dh, device=dev) * 2 - 1
            gl = torch.randn(heads, E, device=dev)
            V = torch.rand(heads, E, device=dev)
            hc = hs.contiguous()
            got = hcspmm.gatv2_scores(hd, hs, att, rp_d, col_d, SLOPE)
            ref = torch_scores(hd, hs, att, rows, cols)
            check = float((got - ref).abs().max() / ref.abs().max())
            assert check < 1e-5, check
            del ref

            def scores():
                return hcspmm.gatv2_scores(hd, hs, att, rp_d, col_d, SLOPE)

            def sddmm_heads():
                return hcspmm.sddmm_heads(hd, hs, *g, heads)

            def backward():
                return hcspmm.gatv2_scores_backward(gl, hd, hs, att, rp_d, col_d, perm32, SLOPE)

            def two_fwh():
                hcspmm.forward_weighted_heads(hc, V, *g)
                hcspmm.forward_weighted_heads(hc, V, *g)

            hd_t, hs_t, att_t = (t.detach().clone().requires_grad_(True) for t in (hd, hs, att))

            def torch_backward():
                return torch.autograd.grad(torch_scores(hd_t, hs_t, att_t, rows, cols), (hd_t, hs_t, att_t), gl)

            y1, y2 = _times([sddmm_heads, sddmm_heads], args.steps, args.warmup)
            w1, w2 = _times([two_fwh, two_fwh], args.steps, args.warmup)
            t_sc, t_sd = _times([scores, sddmm_heads], args.steps, args.warmup)
            t_bw, t_fw = _times([backward, two_fwh], args.steps, args.warmup)
            t_sc2, t_tsc = _times([scores, lambda: torch_scores(hd, hs, att, rows, cols)], args.torch_steps, 2)
            t_bw2, t_tbw = _times([backward, torch_backward], args.torch_steps, 2)
            t_lib, t_tl = _times([lib_step, torch_step], args.torch_steps, 2)
            print("%-14s %dx%-3d | yardstick spread: sddmm_heads %.4f / %.4f ms (%.3f), 2 x forward_weighted_heads %.4f / %.4f ms "
                  "(%.3f) | gatv2_scores %.4f ms vs sddmm_heads %.4f ms (ratio %.3f) | backward %.4f ms vs 2 x "
                  "forward_weighted_heads %.4f ms (ratio %.3f) | torch: scores %.3f ms (library %.1fx faster), backward %.3f ms "
                  "(%.1fx faster), GATv2Conv step library %.3f ms vs torch %.3f ms (%.1fx faster) | check %.2g | %.0f s"
                  % (wl, heads, dh, y1, y2, y1 / y2, w1, w2, w1 / w2, t_sc, t_sd, t_sc / t_sd, t_bw, t_fw, t_bw / t_fw,
                     t_tsc, t_tsc / t_sc2, t_tbw, t_tbw / t_bw2, t_lib, t_tl, t_tl / t_lib, check, time.time() - t0), flush=True)
            del conv, X, G, both, hs, hd, hc, gl, V, got, hd_t, hs_t, att_t
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
