"""The neighbour sampler without a GPU: the properties of its key that the definition (include/hcspmm.h) relies on, checked on
the numpy restatement tests/sampling_reference.py, and the argument errors of the C entry points that build graphs on the
device, which return before any launch."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sampling_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hc-spmm_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345])
def test_keys_are_distinct(seed):
    """for one seed, key is a bijection of e: no ties, so the selection needs no tie rule"""
    k = ref.keys(np.arange(10 ** 6), seed)
    assert k.max() < 2 ** 32
    assert len(np.unique(k)) == 10 ** 6


def test_key_follows_the_definition_on_a_scalar():
    def fmix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)

    for e, seed in ((0, 0), (7, 1), (123456, 2 ** 32 + 5), (2 ** 31 - 1, 2 ** 63 + 12345), (99, 2 ** 64 - 1)):
        want = fmix((fmix(((e * 0x9E3779B1) + (seed & 0xFFFFFFFF)) & 0xFFFFFFFF) + (seed >> 32)) & 0xFFFFFFFF)
        assert int(ref.keys(np.array([e]), seed)[0]) == want, (e, seed)


def _chi2(e0, seeds):
    """one row of 20 entries starting at CSR position e0, fanout 5: chi-square of the 20 selection counts against uniform"""
    rp = np.array([0, 20], dtype=np.int64)
    counts = np.zeros(20)
    for s in seeds:
        # the row's entries sit at positions e0 ... e0 + 19 of a longer graph: select on their keys directly
        k = ref.keys(np.arange(e0, e0 + 20), s)
        counts[np.argsort(k)[:5]] += 1
    assert counts.sum() == 5 * len(seeds)
    want = 5 * len(seeds) / 20
    # the restatement's own selection on a graph that IS this row (e0 = 0) agrees with the direct one
    if e0 == 0:
        again = np.zeros(20)
        for s in seeds:
            again[ref.sample_neighbors(rp, np.arange(20), 5, s)[2]] += 1
        assert np.array_equal(again, counts)
    return float(((counts - want) ** 2 / want).sum())


@pytest.mark.parametrize("e0", [0, 7, 1000, 123456, 2 ** 31 - 40])
def test_selection_is_uniform_over_seeds(e0):
    """seeds 0 ... 399 (consecutive epochs): chi-square below 43.8, the 0.1 % point for 19 degrees of freedom (the
    restatement gives 9.7 - 16.9)"""
    chi2 = _chi2(e0, range(400))
    print("e0 = %d: chi2 = %.1f" % (e0, chi2))
    assert chi2 < 43.8


def test_selection_is_uniform_over_multiplied_64_bit_seeds():
    """seeds s * 0x9E3779B97F4A7C15 mod 2^64: both halves of the seed vary (the restatement gives 13.1)"""
    chi2 = _chi2(0, [(s * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF for s in range(400)])
    print("chi2 = %.1f" % chi2)
    assert chi2 < 43.8


def test_restatement_on_a_small_graph():
    rp = np.array([0, 0, 3, 4, 10, 10], dtype=np.int32)
    col = np.array([1, 2, 4, 0, 0, 1, 2, 3, 4, 5], dtype=np.int32)
    rp_s, col_s, eid_s = ref.sample_neighbors(rp, col, 3, 9)
    assert rp_s.tolist() == [0, 0, 3, 4, 7, 7]
    assert eid_s[:4].tolist() == [0, 1, 2, 3] and col_s[:4].tolist() == [1, 2, 4, 0]
    k = ref.keys(np.arange(4, 10), 9)
    assert eid_s[4:].tolist() == sorted((4 + np.argsort(k)[:3]).tolist())
    assert np.array_equal(col_s, col[eid_s]) and np.all(np.diff(eid_s) > 0)
    # fanout >= the maximum degree gives the graph back
    rp_f, col_f, eid_f = ref.sample_neighbors(rp, col, 6, 1)
    assert np.array_equal(rp_f, rp) and np.array_equal(col_f, col) and np.array_equal(eid_f, np.arange(10))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_argument_errors_return_before_any_launch(tmp_path):
    """tests/capi/sampling_arg_codes.cpp: a program of its own, run with no GPU visible"""
    assert os.path.exists(os.path.join(CSRC, "libhcspmm.so")), "libhcspmm.so is not built"
    exe = str(tmp_path / "sampling_arg_codes")
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "capi", "sampling_arg_codes.cpp"), "-L", CSRC, "-lhcspmm",
                           "-Wl,-rpath," + CSRC, "-o", exe])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-2000:], r.stderr[-2000:])


def test_front_end_names_and_constants():
    import re
    import hcspmm
    from hcspmm import capi
    for name in ("sample_row_pointers", "sample_neighbors", "transpose_graph_device", "plan_free_graph"):
        assert callable(getattr(hcspmm, name)) and name in hcspmm.__all__
    with open(os.path.join(ROOT, "include", "hcspmm.h")) as f:
        header = f.read()
    assert int(re.search(r"#define HCSPMM_SAMPLE_WAVE_ROW_MAX (\d+)", header).group(1)) == hcspmm.SAMPLE_WAVE_ROW_MAX
    assert re.search(r"#define HCSPMM_ABI_VERSION 3\b", header)  # additions: the ABI version stays
    L = capi.lib()
    assert L.hcspmm_sample_workspace_bytes(-1) == 0 and L.hcspmm_sample_workspace_bytes(300) >= 4
    assert L.hcspmm_transpose_graph_device_workspace_bytes(10, 10, 0) == 0
    assert L.hcspmm_transpose_graph_device_workspace_bytes(10, 10, 5000) >= 2 * 5000 * 4
