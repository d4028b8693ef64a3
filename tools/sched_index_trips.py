"""Dependent memory round trips of the sparse-row path's waves, counted from a built plan: what a wave of the ordinary and of
the sliced region waits for, one after the other, before and with the first-index records of the schedule copies
(include/hcspmm.h off_task_sched_idx / off_slice_sched_idx).  Host-only; next to tools/schedule_slots.py, whose ladder it shares.

A wave life (spmm_impl.h hybrid_plan_kernel, L = 8, 32-column panels: eight descriptors per wave, once per panel):
  before   [slice table, sliced region only] -> descriptor -> first index chunk -> gather batches
  with     descriptor + first index chunk, requested together -> gather batches
           (sliced region: the table of eight slices comes with the kernel arguments)
Later index chunks are requested under the gathers of the chunk before them and cost no trip of their own; a gather batch is
one trip (8, 4, 2 or 1 loads in flight per lane).

Index requests: before, a lane group on the one-index path (waves whose longest task has at most 32 entries) asks for 32
bytes of column_index per chunk of 8 entries, on the four-index path (waves with a longer task) for 32 entries at once.  With
the records every wave takes the four-index path; a task's first 32 entries come from its record -- one aligned 128-byte line,
one request -- and only what lies behind them from column_index.  The lines count says how many 128-byte lines a task's
requests touch (column_index[first ...] starts anywhere in a line, a record at its beginning).

  python tools/sched_index_trips.py [--workload reddit] [--dim 128]
  python tools/sched_index_trips.py --powerlaw 29125,1450000,3 [--slice-threshold 256]
"""
import argparse
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "hc-spmm_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hcspmm  # noqa: E402
from hcspmm import graphs  # noqa: E402


def wave_batches(desc):
    """(gather batches per wave, longest task per wave, lengths [waves][8]) of the descriptors, eight to a wave."""
    lens = np.where(desc[:, 0] >= 0, desc[:, 2], 0).astype(np.int64)  # (slice-list padding: row -1)
    lens = np.concatenate([lens, np.zeros(-len(lens) % 8, np.int64)]).reshape(-1, 8)
    nmax = lens.max(axis=1) if len(lens) else np.zeros(0, np.int64)
    stride = np.where(nmax > 32, 32, 8)
    batches = (nmax // stride) * (stride // 8)
    cnt, j = nmax % stride, np.zeros_like(nmax)
    while np.any(j < cnt):  # the last chunk, batch by batch: 8 while more than 4 remain, then 4 / 2 / 1
        left = cnt - j
        step = np.where(left > 4, 8, np.where(left > 2, 4, np.where(left > 1, 2, np.where(left > 0, 1, 0))))
        batches += step > 0
        j += step
    return batches, nmax, lens


def index_requests(desc):
    """Index requests and 128-byte index lines of the descriptors' tasks, those of at most 32 entries and all of them:
    (short tasks, their requests before, with, their lines before, with, all tasks, requests before, with, lines before, with)."""
    _, nmax, lens = wave_batches(desc)
    first = np.concatenate([desc[:, 1].astype(np.int64), np.zeros(-len(desc) % 8, np.int64)]).reshape(-1, 8)
    real = lens > 0
    four = np.broadcast_to((nmax > 32)[:, None], lens.shape)[real]  # the wave's index path before
    n, e0 = lens[real], first[real]
    lines = lambda a, b: np.where(b > a, (4 * b - 1) // 128 - (4 * a) // 128 + 1, 0)  # lines of column_index[a, b)
    req_before = np.where(four, (n + 31) // 32, (n + 7) // 8)
    req_with = 1 + (np.maximum(n - 32, 0) + 31) // 32
    lines_before = lines(e0, e0 + n)
    lines_with = 1 + lines(e0 + 32, e0 + n)
    short = n <= 32
    return np.array([short.sum(), req_before[short].sum(), req_with[short].sum(), lines_before[short].sum(), lines_with[short].sum(),
                     len(n), req_before.sum(), req_with.sum(), lines_before.sum(), lines_with.sum()], np.int64)


def trip_table(plan, n_wide):
    h = hcspmm.capi.Header.from_buffer_copy(plan[:hcspmm.capi.Header.WORDS].tobytes())
    n_nt = h.n_tasks - h.n_tiny
    off_t = h.off_task_sched or h.off_tasks
    off_s = h.off_slice_sched or h.off_slice_tasks
    regions = [("ordinary", [plan[off_t:off_t + 4 * n_nt].reshape(-1, 4)[n_wide:]], 0)]
    if h.n_slices:
        table = plan[h.off_slice_table:h.off_slice_table + h.n_slices + 1]
        d = plan[off_s:off_s + 4 * h.n_slice_tasks].reshape(-1, 4)
        regions.append(("sliced", [d[table[s]:table[s + 1]] for s in range(h.n_slices)], 1))
    rows, short = [], np.zeros(10, np.int64)
    for name, lists, table_hop in regions:
        lives = idle = batches = 0
        for d in lists:
            b, nmax, _ = wave_batches(d)
            lives += int((nmax > 0).sum())
            idle += int((nmax == 0).sum())  # waves of nothing but padding: they read their descriptors and end
            batches += int(b.sum())
            short += index_requests(d)
        table_arg = table_hop and h.n_slices == 8
        before = lives * (2 + table_hop) + batches
        with_ = lives * (1 + (table_hop and not table_arg)) + batches
        rows.append((name, lives, idle, batches, before, with_))
    return h, rows, short


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="reddit", help="a bench.py workload")
    ap.add_argument("--powerlaw", default="", help="nodes,entries,seed: graphs.powerlaw_graph instead of a workload")
    ap.add_argument("--dim", type=int, default=128, help="embedding width: sets the launch's wide-task prefix")
    ap.add_argument("--slice-threshold", type=int, default=0, help="hcspmm_plan_params.slice_threshold (0: automatic)")
    args = ap.parse_args()
    if args.powerlaw:
        n, e, seed = (int(x) for x in args.powerlaw.split(","))
        rp, col = graphs.powerlaw_graph(n, e, seed=seed)
        name = "powerlaw_graph(%d, %d, seed=%d)" % (n, e, seed)
        n_cols = n
    else:
        import bench
        n_local, e_local, _, vw, _ = bench.WORKLOADS[args.workload]
        rp, col = bench.make_local_block(args.workload, n_local, e_local, vw, 0)
        name = args.workload
        n_cols = n_local * vw
    N, E = len(rp) - 1, len(col)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    bp, e2c, e2r, ht, plan, _ = hcspmm.preprocess(t(col), t(rp), N, E, (N + 15) // 16, num_columns=n_cols)
    if args.slice_threshold:
        plan = hcspmm.build_plan(t(rp), t(col), bp, e2c, ht, slice_threshold=args.slice_threshold, num_columns=n_cols)
    thr = hcspmm.wide_threshold(plan, args.dim)
    plan = plan.numpy()
    h = hcspmm.capi.Header.from_buffer_copy(plan[:hcspmm.capi.Header.WORDS].tobytes())
    n_wide = h.n_len_gt[(16, 32, 64, 128, 256).index(thr)] if thr in (16, 32, 64, 128, 256) else 0
    h, rows, short = trip_table(plan, n_wide)
    rec_words = h.total_words - h.off_task_sched_idx if h.off_task_sched_idx else 0
    print("%s: N=%d E=%d; D=%d: %d wide tasks; %d non-tiny tasks, %d slice descriptors in %d lists"
          % (name, N, E, args.dim, n_wide, h.n_tasks - h.n_tiny, h.n_slice_tasks, h.n_slices))
    print("plan: %d words (%.1f MB), of them first-index records %d words (%.1f MB, %d records)"
          % (h.total_words, h.total_words * 4 / 1e6, rec_words, rec_words * 4 / 1e6, rec_words // 32))
    print("%-10s %10s %10s %14s %16s %16s %14s %12s" % ("per panel", "wave lives", "idle waves", "gather batches", "trips before", "trips with",
                                                       "per life", "removed"))
    tb = tw = 0
    for name, lives, idle, batches, before, with_ in rows:
        print("%-10s %10d %10d %14d %16d %16d %6.2f -> %-5.2f %11.1f%%" % (name, lives, idle, batches, before, with_, before / max(lives, 1),
                                                                         with_ / max(lives, 1), 100.0 * (before - with_) / max(before, 1)))
        tb, tw = tb + before, tw + with_
    print("%-10s %10s %10s %14s %16d %16d %14s %11.1f%%" % ("total", "", "", "", tb, tw, "", 100.0 * (tb - tw) / max(tb, 1)))
    print("per panel, lane-group index requests and 128-byte index lines touched (before -> with the records):")
    print("  tasks of at most 32 entries: %8d  requests %8d -> %-8d lines %8d -> %d" % tuple(short[:5]))
    print("  all ordinary + sliced tasks: %8d  requests %8d -> %-8d lines %8d -> %d" % tuple(short[5:]))


if __name__ == "__main__":
    main()
