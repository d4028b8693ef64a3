"""Cost of the multi-head weighted aggregation and SDDMM on bf16 rows (include/hcspmm.h hcspmm_forward_weighted_heads_typed,
hcspmm_sddmm_heads_typed) against the fp32 launches (section 3.11) on widened copies of the same
inputs, on one GPU, with tools/edge16_ab.py's method: HIP events, median of --steps after --warmup, the variants alternated
within one process and the whole comparison repeated --runs times in that process, so that a ratio can be held against the spread
of the fp32 runs.  Per workload and heads x Dh: forward_weighted_heads16 in its four forms (identity / indexed values, fp32 / 16-bit
Z) against forward_weighted_heads and forward_weighted_indexed, and sddmm_heads16 against sddmm_heads.  Then one training epoch of
the driver's --model gat --gat-concat network (forward, loss, backward, Adam) with bf16 and with fp32 activations.
Nothing here is a merge condition: the figures are recorded.  HCSPMM_LIB selects the library, so that two builds can be held
against the same fp32 launches in one run.

Every workload is a step of its own: a child process under its own time limit; the run stops at the first step that fails.
The parent never opens the GPU.

  python tools/heads16_ab.py [--workloads reddit,rd_like] [--shapes 8x8,8x16,4x64] [--runs 3] [--log FILE]
"""
import argparse
import importlib.util
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hc-spmm_amd"), os.path.join(ROOT, "hc-spmm_amd", "hybrid_kernel"), os.path.join(ROOT, "tools")]


def _line(wl, shape, what, names, runs):
    mean = [sum(r[k] for r in runs) / len(runs) for k in range(len(names))]
    cells = ["(%s) %.4f ms [%.4f, %.4f]" % (names[k], mean[k], min(r[k] for r in runs), max(r[k] for r in runs)) for k in range(len(names))]
    ratios = " ".join("f32/%s %.3f" % (names[k], mean[0] / mean[k]) for k in range(1, len(names)))
    print("%-8s %-5s %-9s | %s | %s | f32 max/min over runs %.3f" % (wl, shape, what, " | ".join(cells), ratios,
                                                                    max(r[0] for r in runs) / min(r[0] for r in runs)), flush=True)


def _epoch_ms(main_mod, GNN_model, graph, N, heads, hidden, activation_dtype, steps, warmup):
    """one epoch of the driver's network (HC-SpMM_main.Net: 3 layers, dim 96, 22 classes) as the driver builds it for --model gat --gat-concat"""
    import torch
    dev = graph[0].device
    gen = torch.Generator().manual_seed(0)
    data = types.SimpleNamespace(x=torch.randn(N, 96, generator=gen).to(dev), y=torch.randint(0, 22, (N,), generator=gen).to(dev),
                                 num_features=96, num_classes=22)

    def conv_cls(input_dim, output_dim, fixed):
        if fixed != 2:
            return GNN_model.GATConv(input_dim, output_dim // heads, fixed, heads=heads, concat=True,
                                     activation_dtype=activation_dtype if input_dim % 2 == 0 else None)
        conv = GNN_model.GATConv(input_dim, output_dim, fixed, heads=heads)
        return conv if activation_dtype is None else main_mod._Fp32Input(conv)

    net = main_mod.Net(conv_cls, data, graph, torch.zeros(N, hidden, device=dev), hidden, 3).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=0.01)
    ts, loss = [], None
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad()
        loss = main_mod.nll_loss(net(), data.y)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], float(loss.detach())


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
    idx = torch.randperm(E, device=dev).to(torch.int32)
    for shape in args.shapes.split(","):
        heads, dh = (int(v) for v in shape.split("x"))
        X16 = torch.randn(N, heads * dh, device=dev).to(torch.bfloat16)
        X32, V = X16.float(), torch.rand(heads, E, device=dev)
        fwd = [lambda: hcspmm.forward_weighted_heads(X32, V, *g), lambda: hcspmm.forward_weighted_heads16(X16, V, *g, out_dtype=torch.float32),
               lambda: hcspmm.forward_weighted_heads16(X16, V, *g)]
        ind = [lambda: hcspmm.forward_weighted_indexed(X32, V, idx, *g),
               lambda: hcspmm.forward_weighted_heads16(X16, V, *g, value_index=idx, out_dtype=torch.float32),
               lambda: hcspmm.forward_weighted_heads16(X16, V, *g, value_index=idx)]
        sd = [lambda: hcspmm.sddmm_heads(X32, X32, *g, heads), lambda: hcspmm.sddmm_heads16(X16, X16, *g, heads)]
        for what, names, fns in (("identity", ("f32", "Z32", "Z16"), fwd), ("indexed", ("f32", "Z32", "Z16"), ind), ("sddmm", ("f32", "bf16"), sd)):
            _line(wl, shape, what, names, [_times(fns, args.steps, args.warmup) for _ in range(args.runs)])
    if args.epoch:
        import GNN_model
        spec = importlib.util.spec_from_file_location("hc_spmm_main_ab", os.path.join(ROOT, "hc-spmm_amd", "HC-SpMM_main.py"))
        main_mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(main_mod)
        import HCSPMM
        ge = (rp_d, col_d) + tuple(HCSPMM.preprocess(col_d, rp_d, N, E, (N + 15) // 16, -1))
        for heads, hidden in ((8, 64), (8, 128)):
            for name, dt in (("fp32", None), ("bf16", torch.bfloat16), ("fp32", None)):
                ms, loss = _epoch_ms(main_mod, GNN_model, ge, N, heads, hidden, dt, args.steps, args.warmup)
                print("%-8s epoch gat --gat-concat heads %d hidden %d activations %s: %.2f ms, loss %.4f" % (wl, heads, hidden, name, ms, loss),
                      flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="reddit,rd_like")
    ap.add_argument("--shapes", default="8x8,8x16,4x64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of the whole comparison inside one process")
    ap.add_argument("--epoch", type=int, default=1, help="0: skip the training epochs")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds per workload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r29", "heads16_ab.log"))
    ap.add_argument("--step", default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as log:
        log.write("library: %s\n" % (os.environ.get("HCSPMM_LIB") or "csrc/libhcspmm.so"))
        for wl in args.workloads.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", wl, "--shapes", args.shapes, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--runs", str(args.runs), "--epoch", str(args.epoch)]
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
