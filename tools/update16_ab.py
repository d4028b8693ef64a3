"""A/B of the update GEMM and the weight gradient on fp32 / bf16 / fp16 operands: per-call time of HCSPMM.update and
HCSPMM.weight_grad through the ctypes front-end, the streamed bytes over that time, and torch.mm on the same operands.

    python tools/update16_ab.py > profiles/r24/update16_ab.log

Every variant of a shape rotates through enough copies of its inputs to cover 1 GiB (four times the 256 MiB Infinity Cache), so
each call streams its inputs from HBM also at the 233 K-row shapes; outputs are allocated per call.  A timed window is as many
calls as fill about 50 ms (from a trial call), between device events; the variants of a shape are timed in turn, three rounds,
and the median per variant is reported."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hc-spmm_amd"))
import hcspmm  # noqa: E402

UPDATE = [(4860000, 32, 32), (4860000, 96, 32), (233000, 128, 64), (233000, 602, 64)]
WGRAD = [(4860000, 32, 32), (4860000, 96, 32), (233000, 128, 64)]
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def copies(*tensors):
    """lists of copies of the tensors, enough of them to cover 1 GiB"""
    n = max(1, -(-(1 << 30) // sum(t.numel() * t.element_size() for t in tensors)))
    return [[t.clone() for _ in range(n)] for t in tensors]


def window(fn, n_copies, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for c in range(calls):
        fn(c % n_copies)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def timed(variants, window_ms):
    """variants: {key: (fn(copy index), copies)} -> {key: median us per call, None where fn declines}"""
    live = {k: v for k, v in variants.items() if v[0](0) is not None}
    calls = {k: max(20, int(window_ms * 1e3 / window(fn, n, 5))) for k, (fn, n) in live.items()}  # (the trial warms up as well)
    reps = {k: [] for k in live}
    for _ in range(3):
        for k, (fn, n) in live.items():
            reps[k].append(window(fn, n, calls[k]))
    return {k: (statistics.median(reps[k]) if k in live else None) for k in variants}


def line(op, shape, name, out_name, us, mm_us, nbytes):
    f = lambda v: "   n/a" if v is None else "%8.1f" % v
    print("%-11s %-20s %-5s out=%-5s  kernel %s us  %6s TB/s   torch.mm %s us" % (
        op, shape, name, out_name, f(us), "n/a" if us is None else "%.2f" % (nbytes / us / 1e6), f(mm_us)), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--window-ms", type=float, default=50.0)
    ms = p.parse_args().window_ms
    dev = torch.device("cuda:0")
    print("device:", torch.cuda.get_device_name(0), "| window", ms, "ms")
    for N, D, H in UPDATE:
        x32, w32 = torch.randn(N, D, device=dev), torch.randn(D, H, device=dev)
        variants = {}
        for name, dt in DT.items():
            (xs,), w = copies(x32.to(dt)), w32.to(dt)
            for od in ([dt] if dt == torch.float32 else [dt, torch.float32]):
                variants[(name, od)] = ((lambda c, xs=xs, w=w, od=od: hcspmm.update(xs[c], w, od)), len(xs))
            variants[(name, "mm")] = ((lambda c, xs=xs, w=w: torch.mm(xs[c], w)), len(xs))
        del x32
        us = timed(variants, ms)
        for (name, od), t in us.items():
            if od != "mm":
                line("update", (N, D, H), name, [k for k, v in DT.items() if v == od][0], t, us[(name, "mm")] if od == DT[name] else None,
                     N * (D * DT[name].itemsize + H * od.itemsize))
        del variants
    for N, D, H in WGRAD:
        a32, b32 = torch.randn(N, D, device=dev), torch.randn(N, H, device=dev)
        variants = {}
        for name, dt in DT.items():
            As, Bs = copies(a32.to(dt), b32.to(dt))
            variants[(name, "k")] = ((lambda c, As=As, Bs=Bs: hcspmm.weight_grad(As[c], Bs[c])), len(As))
            variants[(name, "mm")] = ((lambda c, As=As, Bs=Bs: torch.mm(As[c].t(), Bs[c])), len(As))
        del a32, b32
        us = timed(variants, ms)
        for name, dt in DT.items():
            line("weight_grad", (N, D, H), name, "fp32", us[(name, "k")], us[(name, "mm")], N * (D + H) * dt.itemsize)
        del variants


if __name__ == "__main__":
    main()
