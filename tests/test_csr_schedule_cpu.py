"""The schedule of the CSR-served aggregation launches is written once (csrc/csr_schedule.h): no other
unit decodes the plan's slice table or its two-word dense records, or searches the fix-up list, on its own.  A new family
that starts as a copy of an old one fails here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hc-spmm_amd", "csrc")

# who may name the plan's regions: the boundary, the plan's builder, the argument structs, the hybrid launch and its weighted
# and multi-head forms (MFMA dense paths, a fused form and a tiny launch of their own), and the shared walk
DECODERS = {"capi.hip", "plan_host.cpp", "spmm_kernels.h", "spmm_impl.h", "spmm_weighted_impl.h", "spmm_weighted_heads_impl.h",
            "csr_schedule.h"}
# fused_rows.hip multiplies the two-word dense records on MFMA (the fused aggregate + update): it reads them, never the slices
DENSE_RECORD_READERS = DECODERS | {"fused_rows.hip"}

# the binary search from a partial slot to its fix-up record: a `while (hi - lo > 1)` in a function that opened the fix-up list
SLOT_SEARCH = re.compile(r"off_fixups[^}]*?while \(hi - lo > 1\)")


def _sources():
    for unit in sorted(os.listdir(CSRC)):
        if unit.endswith((".hip", ".h", ".cpp")):
            yield unit, open(os.path.join(CSRC, unit)).read()


def test_the_schedule_header_exists():
    text = open(os.path.join(CSRC, "csr_schedule.h")).read()
    for name in ("csr_plan_walk", "csr_window_walk", "fixup_of_slot", "csr_launch", "csr_dispatch"):
        assert name in text, name


def test_only_the_listed_units_decode_the_plans_regions():
    for unit, text in _sources():
        if unit not in DECODERS:
            assert "off_slice_table" not in text, unit
        if unit not in DENSE_RECORD_READERS:
            assert "off_dense_compact2" not in text, unit


def test_the_five_families_walk_through_the_header():
    for unit in ("spmm_extremum.hip", "spmm_multi.hip", "spmm_softmax.hip", "softmax_aggr_grad.hip", "spmm_edge_messages.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "csr_plan_walk<" in text and "csr_window_walk<" in text and "csr_launch(" in text and "csr_dispatch(" in text, unit
        assert "plan_launch_layout" not in text and "pick_L" not in text, unit


def test_one_search_over_the_fixup_list():
    holders = [unit for unit, text in _sources() if SLOT_SEARCH.search(text)]
    assert holders == ["csr_schedule.h"], holders
    # the pattern does find the search it guards against: the copy each family used to carry
    copy = ("const int4* fix = reinterpret_cast<const int4*>(a.plan + a.off_fixups);\n  int lo = 0, hi = a.n_split_rows;\n"
            "  while (hi - lo > 1) {")
    assert SLOT_SEARCH.search(copy)
