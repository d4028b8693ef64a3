"""Host tests of the plan's schedule sections (include/hcspmm.h off_task_sched / off_slice_sched): copies of the non-tiny
tasks and of the slice lists in exact descending length order, which the binary product's launch reads so that the eight lane
groups of a wave end together.  The lists themselves keep the order that test_host_cpu.py pins.

The slot count below is the kernel's own ladder (spmm_impl.h sparse_task_body, 8-lane groups, 32-column panels): a wave
holds eight consecutive descriptors and loops to the longest of them, nmax, in chunks of 8 entries (32 where nmax > 32);
inside a chunk, batches of 8 gathers while more than 4 remain, then 4 / 2 / 1.  Every lane group issues every batch."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hcspmm
from hcspmm import graphs
from hcspmm.capi import Header

import test_host_cpu as host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import schedule_slots  # noqa: E402
PAD = np.array([-1, 0, 0, -1])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _graph_with_lengths(lengths, n_cols, seed):
    """One row per entry of `lengths`, in shuffled row order, ascending unique column ids below n_cols."""
    rng = np.random.default_rng(seed)
    deg = np.array(lengths, np.int64)
    rng.shuffle(deg)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(n_cols, size=d, replace=False)) for d in deg]).astype(np.int32)
    return rp, col


def _every_length():
    """Every length 3 ... 600 twice (so that ties exist), among 1 300 rows that index 1 300 columns."""
    return _graph_with_lengths(list(range(3, 601)) * 2 + [0, 1, 2] * 35, 1301, seed=21)


def _plan(rp, col, rule=0, **params):
    bp, e2c, e2r, ht, plan, _ = host._pre(rp, col, rule)
    if params:
        plan = hcspmm.build_plan(_t(rp), _t(col), bp, e2c, ht, **params)
    return plan.numpy(), (bp, e2c, ht)


_CASES = [(name, gen, {}) for name, gen in host._PLAN_GRAPHS] + [
    ("every_length", _every_length, {}),
    ("forced_slices", lambda: graphs.powerlaw_graph(3000, 90000, seed=5, max_degree_frac=0.3), {"slice_threshold": 64, "n_slices": 8}),
]
_built = {}


def _case(name):
    """(rp, col, plan words, header) of a case, built once and shared read-only."""
    if name not in _built:
        gen, params = next((g, p) for n, g, p in _CASES if n == name)
        rp, col = gen()
        plan, _ = _plan(rp, col, 2 if params else 0, **params)
        plan.setflags(write=False)
        _built[name] = (rp, col, plan, Header.from_buffer_copy(plan[:Header.WORDS].tobytes()))
    return _built[name]


def _sections(plan, h):
    """-> (non-tiny tasks, task schedule, [(slice list, its schedule)] with the padding)."""
    n_nt = h.n_tasks - h.n_tiny
    tasks = plan[h.off_tasks:h.off_tasks + 4 * n_nt].reshape(-1, 4)
    sched = plan[h.off_task_sched:h.off_task_sched + 4 * n_nt].reshape(-1, 4)
    lists = []
    if h.n_slices:
        table = plan[h.off_slice_table:h.off_slice_table + h.n_slices + 1].astype(np.int64)
        a = plan[h.off_slice_tasks:h.off_slice_tasks + 4 * h.n_slice_tasks].reshape(-1, 4)
        b = plan[h.off_slice_sched:h.off_slice_sched + 4 * h.n_slice_tasks].reshape(-1, 4)
        lists = [(a[table[s]:table[s + 1]], b[table[s]:table[s + 1]]) for s in range(h.n_slices)]
    return tasks, sched, lists


def _stable_by_length(d):
    """d's rows by descending length, equal lengths in d's order."""
    return d[np.argsort(-d[:, 2].astype(np.int64), kind="stable")]


def gather_slots(desc, first=0):
    """(issued, useful, wave-level gather instructions) per 32-column panel of the descriptors desc[first:], eight to a wave:
    tools/schedule_slots.py's count, the one DESIGN's table is printed from."""
    return tuple(int(x) for x in schedule_slots.gather_slots(desc[first:]))


def plan_slots(plan, h, schedule, n_wide=0):
    """The same over the ordinary tasks (behind the n_wide wide ones) and the slice lists of a plan, from the lists (schedule
    False) or from their schedule copies."""
    tasks, sched, lists = _sections(plan, h)
    tot = np.array(gather_slots(sched if schedule else tasks, n_wide))
    for a, b in lists:
        tot += np.array(gather_slots(b if schedule else a))
    return tuple(int(x) for x in tot)


@pytest.mark.parametrize("name", [c[0] for c in _CASES])
def test_schedule_is_the_lists_in_exact_length_order(name, capi):
    rp, col, plan, h = _case(name)
    N, E = len(rp) - 1, len(col)
    assert h.version == 8 and h.total_words == len(plan)
    assert capi.lib().hcspmm_plan_check(ctypes.byref(h), N, E, len(plan)) == 0
    tasks, sched, lists = _sections(plan, h)
    n_nt = h.n_tasks - h.n_tiny
    assert h.off_task_sched > 0 and h.off_task_sched % 4 == 0 and h.off_task_sched + 4 * n_nt <= h.total_words
    # a permutation of the non-tiny prefix ...
    assert set(map(tuple, sched.tolist())) == set(map(tuple, tasks.tolist())) and len(sched) == len(tasks)
    # ... lengths non-increasing, equal lengths in their original relative order
    assert np.all(np.diff(sched[:, 2]) <= 0)
    assert np.array_equal(sched, _stable_by_length(tasks))
    # the wide-task prefixes hold on the schedule
    for b in range(5):
        n = h.n_len_gt[b]
        assert np.all(sched[:n, 2] > (16 << b)) and np.all(sched[n:, 2] <= (16 << b))
    if name == "every_length":
        assert set(range(3, 513)) <= set(sched[:, 2].tolist()) and h.n_split_rows == 2 * (600 - 512)
    # slice lists: same multiset per slice, sorted the same way, padding at the end, table untouched
    assert (h.off_slice_sched > 0) == (h.n_slices > 0)
    if name == "forced_slices":
        assert h.n_slices == 8 and h.slice_threshold == 64 and h.n_slice_tasks > 0
        assert h.off_slice_sched % 4 == 0 and h.off_slice_sched >= h.off_task_sched + 4 * n_nt
        assert h.off_slice_sched + 4 * h.n_slice_tasks <= h.total_words  # (the section is sized by an upper bound)
        host._decode_slices(plan, h)  # the lists and their table as test_host_cpu.py pins them
    for a, b in lists:
        real = int((a[:, 0] >= 0).sum())
        assert np.array_equal(b[:real], _stable_by_length(a[:real])) and np.all(b[real:] == PAD) and np.all(a[real:] == PAD)
        assert sorted(map(tuple, a.tolist())) == sorted(map(tuple, b.tolist()))
    # the schedule never issues more gather slots than the lists, whatever the wide-task prefix of the launch
    for n_wide in [0] + list(h.n_len_gt):
        was, now = plan_slots(plan, h, False, n_wide), plan_slots(plan, h, True, n_wide)
        assert now[1] == was[1] and now[0] <= was[0] and now[2] <= was[2], (n_wide, was, now)


@pytest.mark.parametrize("name,params", [("powerlaw_10k", {"slice_threshold": -1}), ("forced_slices", {"slice_threshold": 64, "n_slices": 8}),
                                         ("powerlaw_10k", {})], ids=["slices_off", "slices_forced", "either"])
def test_plan_words_sizes_the_schedule(name, params, capi):
    rp, col = _case(name)[:2]
    plan, (bp, e2c, ht) = _plan(rp, col, 2 if name == "forced_slices" else 0, **params)
    h = Header.from_buffer_copy(plan[:Header.WORDS].tobytes())
    pp = hcspmm.capi.PlanParams()
    for k, v in params.items():
        setattr(pp, k, v)
    words = ctypes.c_int64(0)
    assert capi.lib().hcspmm_plan_words(rp.ctypes.data, len(rp) - 1, len(col), bp.numpy().ctypes.data, ht.numpy().ctypes.data,
                                       ctypes.byref(pp), ctypes.byref(words)) == 0
    assert h.off_task_sched > 0 and h.total_words == len(plan)
    if params:
        assert words.value == h.total_words
    else:  # the parameters leave the slices to the build, which knows the column ids: sized for either outcome
        assert words.value >= h.total_words


def test_schedule_switch_leaves_both_sections_out(monkeypatch, capi):
    """HCSPMM_TASK_SCHEDULE=0 at plan build (read per build, not latched): offsets 0, a blob shorter by exactly the two sections,
    everything behind the header byte for byte the default build's."""
    for name in ("powerlaw_ragged", "forced_slices"):
        rp, col, plan, h = _case(name)
        params = next(p for n, g, p in _CASES if n == name)
        monkeypatch.setenv("HCSPMM_TASK_SCHEDULE", "0")
        off, _ = _plan(rp, col, 2 if params else 0, **params)
        monkeypatch.delenv("HCSPMM_TASK_SCHEDULE")
        again, _ = _plan(rp, col, 2 if params else 0, **params)
        assert np.array_equal(again, plan)  # the switch is read per build
        ho = Header.from_buffer_copy(off[:Header.WORDS].tobytes())
        assert ho.off_task_sched == 0 and ho.off_slice_sched == 0 and ho.total_words == len(off) == h.off_task_sched
        assert capi.lib().hcspmm_plan_check(ctypes.byref(ho), len(rp) - 1, len(col), len(off)) == 0
        assert np.array_equal(off[Header.WORDS:], plan[Header.WORDS:h.off_task_sched])
        for f, _ in Header._fields_:
            if f not in ("total_words", "off_task_sched", "off_slice_sched", "n_len_gt", "reserved"):
                assert getattr(ho, f) == getattr(h, f), f
        assert list(ho.n_len_gt) == list(h.n_len_gt)


def test_plan_check_rejects_corrupted_schedule_fields(capi):
    rp, col, plan, _ = _case("forced_slices")
    N, E = len(rp) - 1, len(col)
    L = capi.lib()
    h = Header.from_buffer_copy(plan[:Header.WORDS].tobytes())
    n_nt = h.n_tasks - h.n_tiny
    assert n_nt > 0 and L.hcspmm_plan_check(ctypes.byref(h), N, E, len(plan)) == 0
    bad = [("off_task_sched", h.off_task_sched + 1),                   # unaligned
           ("off_task_sched", h.off_slice_tasks),                      # on top of the slice lists
           ("off_task_sched", h.off_tasks),                            # on top of the task list
           ("off_task_sched", h.total_words - 4 * n_nt + 4),           # runs beyond the blob
           ("off_task_sched", -4),
           ("off_task_sched", 0),                                      # a slice schedule without a task schedule
           ("off_slice_sched", h.off_slice_sched + 2),                 # unaligned
           ("off_slice_sched", h.off_task_sched),                      # on top of the task schedule
           ("off_slice_sched", h.off_slice_tasks),                     # on top of the lists it copies
           ("off_slice_sched", h.total_words - 4 * h.n_slice_tasks + 4),  # runs beyond the blob
           ("off_slice_sched", -8),
           ("total_words", h.off_slice_sched)]
    for field, value in bad:
        keep = getattr(h, field)
        setattr(h, field, value)
        assert L.hcspmm_plan_check(ctypes.byref(h), N, E, 0) == capi.EPLAN, (field, value)
        setattr(h, field, keep)
    # a plan without slices has no slice schedule
    rp, col, plan, _ = _case("powerlaw_10k")
    h = Header.from_buffer_copy(plan[:Header.WORDS].tobytes())
    assert h.n_slices == 0 and h.off_slice_sched == 0
    h.off_slice_sched = h.off_task_sched + 4 * (h.n_tasks - h.n_tiny)
    assert L.hcspmm_plan_check(ctypes.byref(h), len(rp) - 1, len(col), 0) == capi.EPLAN
    h.off_slice_sched = 0
    assert L.hcspmm_plan_check(ctypes.byref(h), len(rp) - 1, len(col), 0) == 0


def _threaded_sort_graph():
    """A power-law graph of 100 000 rows (6 250 row windows: the multi-threaded plan build) whose non-tiny tasks -- more than
    65 536 -- take the multi-threaded path of the schedule's counting sort."""
    return graphs.powerlaw_graph(100000, 1500000, seed=9)


def _digests():
    """sha256 of that graph's default plan and of one with forced slices, after checking the schedule sections themselves."""
    rp, col = _threaded_sort_graph()
    out = []
    for params in ({}, {"slice_threshold": 64, "n_slices": 8}):
        plan, _ = _plan(rp, col, 2, **params)
        h = Header.from_buffer_copy(plan[:Header.WORDS].tobytes())
        assert h.off_task_sched > 0 and (h.off_slice_sched > 0) == bool(params)
        assert h.num_windows >= 4096 and h.n_tasks - h.n_tiny >= 65536
        tasks, sched, lists = _sections(plan, h)
        assert np.array_equal(sched, _stable_by_length(tasks))
        for a, b in lists:
            real = int((a[:, 0] >= 0).sum())
            assert np.array_equal(b[:real], _stable_by_length(a[:real])) and np.all(b[real:] == PAD)
        out.append(hashlib.sha256(plan.tobytes()).hexdigest())
    return out


def test_blob_is_byte_identical_for_1_and_16_host_threads():
    """(The thread count is latched per process -- HCSPMM_THREADS -- so each count builds in a process of its own.)"""
    code = ("import sys; sys.path[:0] = %r; import test_task_schedule_cpu as t; print('digests', *t._digests())"
            % [os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "hc-spmm_amd")])
    procs = [subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, HCSPMM_THREADS=str(n)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for n in (1, 16)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    lines = [[l for l in o.splitlines() if l.startswith("digests ")][-1] for o in outs]
    assert lines[0] == lines[1] and len(lines[0].split()) == 3


def test_schedule_is_built_only_for_cache_resident_column_counts(monkeypatch, capi):
    """The copies are built when one 128-byte line per X row fits 256 MiB (num_columns <= 2 097 152); beyond that the plan is
    the one HCSPMM_TASK_SCHEDULE=0 builds, HCSPMM_TASK_SCHEDULE=1 restores the copies, and hcspmm_plan_words -- which does not
    know the column count -- stays an upper bound."""
    rp, col, small, hs = _case("forced_slices")
    N, E = len(rp) - 1, len(col)
    bp, e2c, e2r, ht, _, _ = host._pre(rp, col, 2)
    params = {"slice_threshold": 64, "n_slices": 8}
    build = lambda m: hcspmm.build_plan(_t(rp), _t(col), bp, e2c, ht, num_columns=m, **params).numpy()
    pp = hcspmm.capi.PlanParams()
    for k, v in params.items():
        setattr(pp, k, v)
    words = ctypes.c_int64(0)
    assert capi.lib().hcspmm_plan_words(rp.ctypes.data, N, E, bp.numpy().ctypes.data, ht.numpy().ctypes.data, ctypes.byref(pp),
                                       ctypes.byref(words)) == 0
    monkeypatch.delenv("HCSPMM_TASK_SCHEDULE", raising=False)
    for m, built in ((2097152, True), (2097153, False), (3000000, False)):
        plan = build(m)
        h = Header.from_buffer_copy(plan[:Header.WORDS].tobytes())
        assert h.num_columns == m and (h.off_task_sched > 0) == built and (h.off_slice_sched > 0) == built, m
        assert h.total_words == len(plan) <= words.value
        assert capi.lib().hcspmm_plan_check(ctypes.byref(h), N, E, len(plan)) == 0
        # the lists do not depend on the gate (the slice boundaries on the column count: compare among equal counts below)
        assert h.total_words == (hs.total_words if built else hs.off_task_sched)
    gated = build(3000000)
    monkeypatch.setenv("HCSPMM_TASK_SCHEDULE", "1")
    forced = build(3000000)
    monkeypatch.setenv("HCSPMM_TASK_SCHEDULE", "0")
    off = build(3000000)
    hf = Header.from_buffer_copy(forced[:Header.WORDS].tobytes())
    assert hf.off_task_sched > 0 and hf.off_slice_sched > 0 and hf.total_words == len(forced) <= words.value
    assert np.array_equal(off, gated)
    assert np.array_equal(forced[Header.WORDS:hf.off_task_sched], gated[Header.WORDS:])
    tasks, sched, lists = _sections(forced, hf)
    assert np.array_equal(sched, _stable_by_length(tasks))


@pytest.fixture(scope="module")
def eighth_scale():
    rp, col = graphs.powerlaw_graph(29125, 1450000, seed=3)
    return rp, col, host._pre(rp, col, 2)


@pytest.mark.parametrize("slices", [True, False], ids=["sliced_as_at_full_scale", "library_default"])
def test_dummy_share_on_the_headline_graph_at_one_eighth_scale(eighth_scale, slices):
    """powerlaw_graph(29125, 1450000, seed=3) with the wide-task prefix of the full-scale launch (tasks above 256 entries), with
    the column slices of the full-scale plan (threshold 256, 8 slices) and with the plan the library builds at this size (no
    slices: 29 125 columns).  The lists issue 28.5 % more gathers than the result needs, the schedule 2.4 %; the bar is 5 % of
    the useful slots."""
    rp, col, (bp, e2c, e2r, ht, plan, _) = eighth_scale
    if slices:
        plan = hcspmm.build_plan(_t(rp), _t(col), bp, e2c, ht, slice_threshold=256, n_slices=8)
    plan = plan.numpy()
    h = Header.from_buffer_copy(plan[:Header.WORDS].tobytes())
    assert h.n_slices == (8 if slices else 0) and h.n_dense == 0
    n_wide = h.n_len_gt[4]
    was, now = plan_slots(plan, h, False, n_wide), plan_slots(plan, h, True, n_wide)
    print("issued / useful / wave instructions per panel: lists %s, schedule %s" % (was, now))
    deg = np.diff(rp)
    if slices:
        assert n_wide == 0 and was[1] == now[1] == int(deg[deg > 2].sum())
    assert was[1] == now[1] > 0.8 * len(col)
    assert (was[0] - was[1]) > 0.20 * was[1]  # the lists' share: this test cannot pass by accident
    assert (now[0] - now[1]) <= 0.05 * now[1]
