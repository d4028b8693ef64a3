"""Host tests of the first-index records of the plan's schedule copies (include/hcspmm.h off_task_sched_idx /
off_slice_sched_idx): one 128-byte record of 32 int32 per descriptor of a schedule copy, in the copy's order, holding
column_index[first : first + min(length, 32)] and -1 behind it; padding descriptors get all -1.  The binary product's launch
asks for a wave's records together with its descriptors, so what the records hold is what its lane groups gather first.

With HCSPMM_SCHED_INDEX=0 at plan build the plan is the one from before the records existed, byte for byte, and
hcspmm_plan_check treats the new header words like the other section offsets."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hcspmm
from hcspmm import graphs
from hcspmm.capi import Header

import test_host_cpu as host
import test_task_schedule_cpu as sched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = 32  # HCSPMM_SCHED_INDEX_WORDS

_CASES = {
    # (graph, classifier rule, plan parameters)
    "forced_slices": (lambda: graphs.powerlaw_graph(3000, 90000, seed=5, max_degree_frac=0.3), 2, {"slice_threshold": 64, "n_slices": 8}),
    "sixteen_slices": (lambda: graphs.powerlaw_graph(3000, 90000, seed=5, max_degree_frac=0.3), 2, {"slice_threshold": 64, "n_slices": 16}),
    "slices_off": (lambda: graphs.powerlaw_graph(3000, 90000, seed=5, max_degree_frac=0.3), 2, {"slice_threshold": -1}),
    "every_length": (sched._every_length, 0, {}),
}
_built = {}


def _case(name):
    """(rp, col, plan words, header), built once and shared read-only."""
    if name not in _built:
        gen, rule, params = _CASES[name]
        rp, col = gen()
        plan, _ = sched._plan(rp, col, rule, **params)
        plan.setflags(write=False)
        _built[name] = (rp, col, plan, Header.from_buffer_copy(plan[:Header.WORDS].tobytes()))
    return _built[name]


def _expected_records(desc, col):
    """The records of the descriptors desc [n][4] (row, first, length, slot), straight from the definition."""
    out = np.full((len(desc), REC), -1, np.int32)
    for i, (row, first, length, _) in enumerate(desc.tolist()):
        if row >= 0:
            k = min(length, REC)
            out[i, :k] = col[first:first + k]
    return out


@pytest.mark.parametrize("name", sorted(_CASES))
def test_records_hold_the_first_indices_in_schedule_order(name, capi):
    rp, col, plan, h = _case(name)
    N, E = len(rp) - 1, len(col)
    assert capi.lib().hcspmm_plan_check(ctypes.byref(h), N, E, len(plan)) == 0
    n_nt = h.n_tasks - h.n_tiny
    assert n_nt > 0 and h.off_task_sched > 0
    sliced = name in ("forced_slices", "sixteen_slices")
    assert (h.n_slices > 0) == sliced
    # behind the schedule copies, on 128-byte boundaries, inside the blob
    sched_end = h.off_slice_sched + 4 * h.n_slice_tasks if sliced else h.off_task_sched + 4 * n_nt
    assert h.off_task_sched_idx >= sched_end and h.off_task_sched_idx % REC == 0
    assert h.off_task_sched_idx + REC * n_nt <= h.total_words == len(plan)
    desc = plan[h.off_task_sched:h.off_task_sched + 4 * n_nt].reshape(-1, 4)
    rec = plan[h.off_task_sched_idx:h.off_task_sched_idx + REC * n_nt].reshape(-1, REC)
    assert np.all(desc[:, 0] >= 0) and desc[:, 2].max() > REC and desc[:, 2].min() <= 8  # both sides of one record's length
    assert np.array_equal(rec, _expected_records(desc, col))
    if not sliced:
        assert h.off_slice_sched_idx == 0 and h.slice_table_copy == [0] * 9
        return
    assert h.off_slice_sched_idx == h.off_task_sched_idx + REC * n_nt and h.off_slice_sched_idx % REC == 0
    assert h.off_slice_sched_idx + REC * h.n_slice_tasks <= h.total_words
    sdesc = plan[h.off_slice_sched:h.off_slice_sched + 4 * h.n_slice_tasks].reshape(-1, 4)
    srec = plan[h.off_slice_sched_idx:h.off_slice_sched_idx + REC * h.n_slice_tasks].reshape(-1, REC)
    pad = sdesc[:, 0] < 0
    assert pad.any() and not pad.all() and np.all(sdesc[pad] == sched.PAD)
    assert np.all(srec[pad] == -1)  # padding descriptors: nothing to gather
    assert np.array_equal(srec, _expected_records(sdesc, col))
    # the section is sized by the slice lists' upper bound: what lies behind the last list is -1 as well
    assert np.all(plan[h.off_slice_sched_idx + REC * h.n_slice_tasks:] == -1)
    # the launcher passes the table of eight slices as kernel arguments: the header holds it once more
    table = plan[h.off_slice_table:h.off_slice_table + h.n_slices + 1].tolist()
    assert h.slice_table_copy == (table if h.n_slices == 8 else [0] * 9)


@pytest.mark.parametrize("name", ["forced_slices", "slices_off", "every_length"])
def test_switch_off_gives_the_plan_from_before_the_records(name, monkeypatch, capi):
    """HCSPMM_SCHED_INDEX=0 at plan build (read per build): both offsets and the table's copy zero, the blob the default
    build's up to the end of the schedule copies -- the layout of the plans built before the records existed."""
    rp, col, plan, h = _case(name)
    _, rule, params = _CASES[name]
    monkeypatch.setenv("HCSPMM_SCHED_INDEX", "0")
    off, _ = sched._plan(rp, col, rule, **params)
    monkeypatch.delenv("HCSPMM_SCHED_INDEX")
    again, _ = sched._plan(rp, col, rule, **params)
    assert np.array_equal(again, plan)  # the switch is read per build
    ho = Header.from_buffer_copy(off[:Header.WORDS].tobytes())
    n_nt = h.n_tasks - h.n_tiny
    sched_words = 4 * n_nt + (h.total_words - h.off_slice_sched_idx) // REC * 4 if h.n_slices else 4 * n_nt
    assert ho.off_task_sched_idx == 0 and ho.off_slice_sched_idx == 0 and ho.slice_table_copy == [0] * 9
    assert ho.total_words == len(off) == h.off_task_sched + sched_words <= h.off_task_sched_idx
    assert capi.lib().hcspmm_plan_check(ctypes.byref(ho), len(rp) - 1, len(col), len(off)) == 0
    assert np.array_equal(off[Header.WORDS:], plan[Header.WORDS:len(off)])
    assert list(ho.reserved) == [0] * 16
    for f, _ in Header._fields_:
        if f not in ("total_words", "reserved", "n_len_gt"):
            assert getattr(ho, f) == getattr(h, f), f
    # without the schedule copies there is nothing the records could belong to
    monkeypatch.setenv("HCSPMM_TASK_SCHEDULE", "0")
    bare, _ = sched._plan(rp, col, rule, **params)
    hb = Header.from_buffer_copy(bare[:Header.WORDS].tobytes())
    assert hb.off_task_sched == 0 and hb.off_task_sched_idx == 0 and hb.off_slice_sched_idx == 0 and list(hb.reserved) == [0] * 16
    assert len(bare) == hb.total_words == h.off_task_sched


def _malformed(h):
    """(field or index into the table's copy, value) of headers hcspmm_plan_check must refuse; h: a plan with eight slices."""
    n_nt = h.n_tasks - h.n_tiny
    return [("off_task_sched_idx", h.off_task_sched_idx + 1),                      # misaligned
            ("off_task_sched_idx", h.off_task_sched_idx + 4),                      # on the dword grid, off the 128-byte one
            ("off_task_sched_idx", (h.off_slice_sched + 4 * h.n_slice_tasks - 1) // REC * REC),  # on top of the slice schedule's end
            ("off_task_sched_idx", h.off_task_sched // REC * REC),                 # on top of the task schedule
            ("off_task_sched_idx", h.off_task_sched_idx + REC),                    # overlaps the slice records
            ("off_task_sched_idx", (h.total_words - REC * n_nt) // REC * REC + REC),  # runs beyond the blob
            ("off_task_sched_idx", -REC),
            ("off_task_sched_idx", 0),                                             # slice records without task records
            ("off_slice_sched_idx", h.off_slice_sched_idx + 2),
            ("off_slice_sched_idx", h.off_slice_sched_idx - REC),                  # overlaps the task records
            ("off_slice_sched_idx", h.off_task_sched_idx),
            ("off_slice_sched_idx", (h.total_words - REC * h.n_slice_tasks) // REC * REC + REC),  # runs beyond the blob
            ("off_slice_sched_idx", -REC),
            ("total_words", h.off_slice_sched_idx),
            ("total_words", h.off_slice_sched_idx + REC * h.n_slice_tasks - 1),
            ("off_task_sched", 0),                                                 # records without the copy they belong to
            (0, 64), (8, h.n_slice_tasks - 64), (3, h.slice_table_copy[3] + 1), (4, h.slice_table_copy[8] + 64)]


def _set(h, field, value):
    if isinstance(field, int):
        keep = h.reserved[2 + field]
        h.reserved[2 + field] = value
    else:
        keep = getattr(h, field)
        setattr(h, field, value)
    return keep


def test_plan_check_rejects_malformed_record_offsets(capi):
    rp, col, plan, _ = _case("forced_slices")
    N, E = len(rp) - 1, len(col)
    L = capi.lib()
    h = Header.from_buffer_copy(plan[:Header.WORDS].tobytes())
    assert L.hcspmm_plan_check(ctypes.byref(h), N, E, len(plan)) == 0
    for field, value in _malformed(h):
        keep = _set(h, field, value)
        assert L.hcspmm_plan_check(ctypes.byref(h), N, E, 0) == capi.EPLAN, (field, value)
        _set(h, field, keep)
    assert L.hcspmm_plan_check(ctypes.byref(h), N, E, len(plan)) == 0
    # a plan without slices has neither slice records nor a copy of the table
    rp, col, plan, _ = _case("slices_off")
    h = Header.from_buffer_copy(plan[:Header.WORDS].tobytes())
    n_nt = h.n_tasks - h.n_tiny
    for field, value in (("off_slice_sched_idx", h.off_task_sched_idx + REC * n_nt), (8, 64)):
        keep = _set(h, field, value)
        assert L.hcspmm_plan_check(ctypes.byref(h), len(rp) - 1, len(col), 0) == capi.EPLAN, (field, value)
        _set(h, field, keep)
    # the task records alone may be absent: the plan of HCSPMM_SCHED_INDEX=0
    h.off_task_sched_idx = 0
    assert L.hcspmm_plan_check(ctypes.byref(h), len(rp) - 1, len(col), 0) == 0


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("c++") is None, reason="no host C++ compiler")
def test_malformed_headers_through_the_c_header(tmp_path):
    """The same cases from C (tests/capi/sched_index_check.cpp against include/hcspmm.h and libhcspmm.so): the struct's own
    field names and offsets, no ctypes mirror in between."""
    cxx = shutil.which("g++") or shutil.which("c++")
    lib_dir = os.path.join(ROOT, "hc-spmm_amd", "csrc")
    exe = str(tmp_path / "sched_index_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "capi", "sched_index_check.cpp"),
                    "-o", exe, "-L" + lib_dir, "-lhcspmm", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "sched_index_check ok" in r.stdout, r.stdout[-2000:]
