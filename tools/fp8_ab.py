"""What does 8-bit (e4m3) feature storage buy the aggregation?  (include/hcspmm.h hcspmm_forward_fp8 / hcspmm_quantize_fp8;
DESIGN.md section 3.15.)  Per case -- a bench.py workload and an embedding width -- three launches on the same graph and
plan parameters, timed with HIP events on one GPU and alternated step by step within one process:
  (a) forward on bf16 features (hcspmm_forward_typed), the baseline: 2 bytes per gathered element, bf16 Z;
  (b) forward_fp8, binary: 1 byte per gathered element, fp32 Z;
  (c) forward_weighted_fp8 with edge values ("sym" normalisation) and the quantiser's per-row scales.
Each of --repeats rounds gives the median of --steps steps (after --warmup) of all three; the spread of (a) is max - min of
its round medians.  fp8 is called faster only when median(a) - median(b) exceeds that spread.

The quantiser itself is timed at the same [N, D] against a device-to-device copy that moves as many bytes as it does
(4 N D read, N D + 4 N written: a copy of half their sum reads and writes that much).

  python tools/fp8_ab.py [--cases reddit:128,reddit:256,rd_like:32,yh_like:32] [--steps 30] [--warmup 10] [--repeats 5]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "tools")]

from gat_ab import _times  # noqa: E402


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="reddit:128,reddit:256,rd_like:32,yh_like:32")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bench
    import hcspmm
    if not torch.cuda.is_available():
        raise SystemExit("fp8_ab.py needs a GPU: it measures, and a CPU has nothing to say about these kernels")
    dev = torch.device("cuda:0")
    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",") if c]
    built = {}
    for wl, D in cases:
        if wl not in built:
            built.clear()
            torch.cuda.empty_cache()
            t0 = time.time()
            n_local, e_local, _, vw, _ = bench.WORKLOADS[wl]
            rp, col = bench.make_local_block(wl, n_local, e_local, vw, 0)
            N, E = len(rp) - 1, len(col)
            rp_d, col_d = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
            built[wl] = (N, E, rp_d, col_d, hcspmm.edge_norm(rp_d, col_d, "sym"))
            print("%-8s N=%d E=%d | graph ready in %.0f s" % (wl, N, E, time.time() - t0), flush=True)
        N, E, rp_d, col_d, values = built[wl]
        g = (rp_d, col_d) + tuple(hcspmm.preprocess(col_d, rp_d, N, E, (N + 15) // 16, dim=D))  # one plan for all three
        X = torch.randn(N, D, device=dev)
        Xb = X.to(torch.bfloat16)
        Xq, scale = hcspmm.quantize_fp8(X)

        def bf16():
            return hcspmm.forward(Xb, *g)[0]

        def fp8_binary():
            return hcspmm.forward_fp8(Xq, None, *g)[0]

        def fp8_scaled():
            return hcspmm.forward_weighted_fp8(Xq, scale, values, *g)[0]

        rounds = [_times([bf16, fp8_binary, fp8_scaled], args.steps, args.warmup) for _ in range(args.repeats)]
        ta, tb, tc = ([r[k] for r in rounds] for k in range(3))
        spread = max(ta) - min(ta)
        gain = _median(ta) - _median(tb)
        print("%-8s D=%-3d | (a) bf16 forward %.4f ms (rounds %s; spread %.4f ms) | (b) forward_fp8 %.4f ms (rounds %s) | "
              "a - b = %+.4f ms, b / a = %.3f -> %s | (c) forward_weighted_fp8 with values and scales %.4f ms (rounds %s), c / b = %.3f"
              % (wl, D, _median(ta), " ".join("%.4f" % t for t in ta), spread, _median(tb), " ".join("%.4f" % t for t in tb), gain,
                 _median(tb) / _median(ta),
                 "fp8 is faster beyond the spread of bf16" if gain > spread else
                 ("fp8 is slower beyond the spread of bf16" if -gain > spread else "within the spread of bf16"),
                 _median(tc), " ".join("%.4f" % t for t in tc), _median(tc) / _median(tb)), flush=True)
        # the quantiser against a copy of as many bytes
        moved = 4 * N * D + N * D + 4 * N
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def quantise():
            return hcspmm.quantize_fp8(X)

        def copy():
            return dst.copy_(src)

        rounds = [_times([quantise, copy], args.steps, args.warmup) for _ in range(args.repeats)]
        tq, tcp = ([r[k] for r in rounds] for k in range(2))
        print("%-8s D=%-3d | quantize_fp8 [%d, %d] %.4f ms (rounds %s) = %.2f TB/s of %.1f MB moved | device-to-device copy of the "
              "same traffic %.4f ms (rounds %s) | quantiser / copy = %.2f"
              % (wl, D, N, D, _median(tq), " ".join("%.4f" % t for t in tq), moved / _median(tq) / 1e9, moved / 1e6, _median(tcp),
                 " ".join("%.4f" % t for t in tcp), _median(tq) / _median(tcp)), flush=True)
        del X, Xb, Xq, scale, src, dst, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
