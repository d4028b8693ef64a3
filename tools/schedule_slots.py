"""Gather slots of the sparse-row path's lane groups, counted from a built plan: what the eight 8-lane groups of a wave
issue against what the result needs, for the plan's lists (descending power-of-two length class, rows ascending) and for
their schedule copies (exact descending length; include/hcspmm.h off_task_sched / off_slice_sched).  Host-only.

The count is the kernel's own ladder (spmm_impl.h sparse_task_body with 32-column panels, L = 8): a wave holds eight
consecutive descriptors and loops to the longest of them, nmax, in chunks of 8 entries (32 where nmax > 32); inside a chunk,
batches of 8 gathers while more than 4 entries remain, then 4 / 2 / 1.  Every lane group issues every batch; a group whose
task has ended re-reads row 0 and discards it.  Figures are per 32-column panel; a wave-level load instruction serves the
eight lane groups at once.

  python tools/schedule_slots.py [--workload reddit] [--dim 128]
  python tools/schedule_slots.py --powerlaw 29125,1450000,3 [--slice-threshold 256]
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


def gather_slots(desc):
    """(lane-group gathers issued, useful ones, wave-level gather instructions) of the descriptors, eight to a wave."""
    lens = np.where(desc[:, 0] >= 0, desc[:, 2], 0).astype(np.int64)  # (slice-list padding: row -1)
    if len(lens) == 0:
        return np.zeros(3, np.int64)
    nmax = np.concatenate([lens, np.zeros(-len(lens) % 8, np.int64)]).reshape(-1, 8).max(axis=1)
    stride = np.where(nmax > 32, 32, 8)
    per_group = (nmax // stride) * stride  # whole chunks: stride / 8 batches of 8
    cnt, j = nmax % stride, np.zeros_like(nmax)
    while np.any(j < cnt):  # the last chunk, batch by batch
        left = cnt - j
        j += np.where(left > 4, 8, np.where(left > 2, 4, np.where(left > 1, 2, np.where(left > 0, 1, 0))))
    per_group += j
    return np.array([8 * per_group.sum(), lens.sum(), per_group.sum()], np.int64)


def slot_table(plan, n_wide):
    """rows (name, issued, useful, instructions) for the ordinary tasks behind the n_wide wide ones and for the slice lists, from
    the lists and from the schedule copies."""
    h = hcspmm.capi.Header.from_buffer_copy(plan[:hcspmm.capi.Header.WORDS].tobytes())
    n_nt = h.n_tasks - h.n_tiny
    rows = []
    for name, off_t, off_s in (("lists", h.off_tasks, h.off_slice_tasks), ("schedule", h.off_task_sched, h.off_slice_sched)):
        if name == "schedule" and h.off_task_sched == 0:
            continue
        ordinary = gather_slots(plan[off_t:off_t + 4 * n_nt].reshape(-1, 4)[n_wide:])
        sliced = np.zeros(3, np.int64)
        if h.n_slices:
            table = plan[h.off_slice_table:h.off_slice_table + h.n_slices + 1]
            d = plan[off_s:off_s + 4 * h.n_slice_tasks].reshape(-1, 4)
            for s in range(h.n_slices):
                sliced += gather_slots(d[table[s]:table[s + 1]])
        rows += [(name + ", ordinary tasks", ordinary), (name + ", slice lists", sliced), (name + ", total", ordinary + sliced)]
    return h, rows


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
        n_cols = n_local * vw  # (a row block of a larger matrix gathers from all its columns)
    N, E = len(rp) - 1, len(col)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    bp, e2c, e2r, ht, plan, _ = hcspmm.preprocess(t(col), t(rp), N, E, (N + 15) // 16, num_columns=n_cols)
    if args.slice_threshold:
        plan = hcspmm.build_plan(t(rp), t(col), bp, e2c, ht, slice_threshold=args.slice_threshold, num_columns=n_cols)
    thr = hcspmm.wide_threshold(plan, args.dim)
    plan = plan.numpy()
    h = hcspmm.capi.Header.from_buffer_copy(plan[:hcspmm.capi.Header.WORDS].tobytes())
    n_wide = h.n_len_gt[(16, 32, 64, 128, 256).index(thr)] if thr in (16, 32, 64, 128, 256) else 0
    h, rows = slot_table(plan, n_wide)
    print("%s: N=%d E=%d; D=%d: tasks above %s entries are wide (%d); %d non-tiny tasks, %d slice descriptors in %d lists, %d dense windows"
          % (name, N, E, args.dim, thr if n_wide else "-", n_wide, h.n_tasks - h.n_tiny, h.n_slice_tasks, h.n_slices, h.n_dense))
    print("plan: %d words (%.1f MB), schedule sections %d words" % (h.total_words, h.total_words * 4 / 1e6,
                                                                   h.total_words - h.off_task_sched if h.off_task_sched else 0))
    print("%-26s %14s %12s %12s %16s" % ("per 32-column panel", "issued", "useful", "dummy/useful", "wave-level loads"))
    for label, (issued, useful, instr) in rows:
        print("%-26s %14d %12d %11.1f%% %16d" % (label, issued, useful, 100.0 * (issued - useful) / max(useful, 1), instr))


if __name__ == "__main__":
    main()
