// Host-only check of the first-index records of the schedule copies (include/hcspmm.h off_task_sched_idx / off_slice_sched_idx)
// through the C header itself: builds a column-sliced plan on the host, compares every record with column_index, and hands
// hcspmm_plan_check malformed headers.  No GPU, no HIP call; compiled and run by tests/test_sched_index_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hcspmm.h"

#define REQUIRE(cond)                                               \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);        \
      return 1;                                                     \
    }                                                               \
  } while (0)

static int check_records(const int32_t* desc, const int32_t* rec, int64_t n, const std::vector<int32_t>& col) {
  for (int64_t i = 0; i < n; ++i) {
    const int32_t* d = desc + 4 * i;
    const int32_t* r = rec + HCSPMM_SCHED_INDEX_WORDS * i;
    const int k = d[0] < 0 ? 0 : (d[2] < HCSPMM_SCHED_INDEX_WORDS ? d[2] : HCSPMM_SCHED_INDEX_WORDS);
    for (int j = 0; j < HCSPMM_SCHED_INDEX_WORDS; ++j) REQUIRE(r[j] == (j < k ? col[(size_t)d[1] + j] : -1));
  }
  return 0;
}

int main() {
  // 600 rows over 600 columns: row r holds (r * 37) % 131 entries, every 7th row 150-400 of them (sliced above 64 entries)
  const int64_t N = 600;
  std::vector<int32_t> rowptr(N + 1, 0), col;
  uint32_t seed = 12345;
  for (int64_t r = 0; r < N; ++r) {
    const int64_t d = r % 7 == 0 ? 150 + (r * 13) % 251 : (r * 37) % 131;
    int64_t left = d;  // d ascending column ids out of N: selection sampling
    for (int64_t c = 0; c < N && left > 0; ++c) {
      seed = seed * 1664525u + 1013904223u;
      if ((uint64_t)(seed >> 8) % (uint64_t)(N - c) < (uint64_t)left) col.push_back((int32_t)c), --left;
    }
    rowptr[r + 1] = (int32_t)col.size();
  }
  const int64_t E = (int64_t)col.size(), W = (N + 15) / 16;
  std::vector<int32_t> bp(W), ht(W), e2c(E), e2r(E);
  REQUIRE(hcspmm_preprocess_host(rowptr.data(), col.data(), N, E, N, HCSPMM_RULE_AS_SHIPPED, 1, bp.data(), e2c.data(), e2r.data(),
                                 ht.data()) == HCSPMM_OK);
  hcspmm_plan_params pp;
  std::memset(&pp, 0, sizeof(pp));
  pp.slice_threshold = 64;
  pp.n_slices = 8;
  int64_t words = 0;
  REQUIRE(hcspmm_plan_words(rowptr.data(), N, E, bp.data(), ht.data(), &pp, &words) == HCSPMM_OK);
  std::vector<int32_t> plan((size_t)words, 0x5a5a5a5a);
  REQUIRE(hcspmm_plan_build(rowptr.data(), col.data(), N, E, N, bp.data(), e2c.data(), ht.data(), &pp, plan.data(), words) == HCSPMM_OK);
  hcspmm_plan_header h;
  std::memcpy(&h, plan.data(), sizeof(h));
  REQUIRE(hcspmm_plan_check(&h, N, E, words) == HCSPMM_OK);
  const int32_t n_nt = h.n_tasks - h.n_tiny;
  REQUIRE(h.n_slices == 8 && h.n_slice_tasks > 0 && n_nt > 0);
  REQUIRE(h.off_task_sched > 0 && h.off_slice_sched > 0 && h.off_task_sched_idx > 0 && h.off_slice_sched_idx > 0);
  REQUIRE(h.off_task_sched_idx % HCSPMM_SCHED_INDEX_WORDS == 0 && h.off_slice_sched_idx % HCSPMM_SCHED_INDEX_WORDS == 0);
  REQUIRE(h.off_task_sched_idx >= h.off_slice_sched + 4 * h.n_slice_tasks);
  REQUIRE(h.off_slice_sched_idx == h.off_task_sched_idx + HCSPMM_SCHED_INDEX_WORDS * n_nt);
  REQUIRE((int64_t)h.off_slice_sched_idx + (int64_t)HCSPMM_SCHED_INDEX_WORDS * h.n_slice_tasks <= h.total_words && h.total_words <= words);
  if (check_records(plan.data() + h.off_task_sched, plan.data() + h.off_task_sched_idx, n_nt, col)) return 1;
  if (check_records(plan.data() + h.off_slice_sched, plan.data() + h.off_slice_sched_idx, h.n_slice_tasks, col)) return 1;
  for (int64_t i = h.off_slice_sched_idx + (int64_t)HCSPMM_SCHED_INDEX_WORDS * h.n_slice_tasks; i < h.total_words; ++i) REQUIRE(plan[(size_t)i] == -1);
  for (int s = 0; s <= 8; ++s) REQUIRE(h.slice_table_copy[s] == plan[(size_t)h.off_slice_table + s]);

  // malformed headers
  int cases = 0;
#define REJECTED(stmt)                                                   \
  do {                                                                   \
    hcspmm_plan_header b = h;                                            \
    stmt;                                                                \
    REQUIRE(hcspmm_plan_check(&b, N, E, 0) == HCSPMM_EPLAN);             \
    ++cases;                                                             \
  } while (0)
  const int R = HCSPMM_SCHED_INDEX_WORDS;
  REJECTED(b.off_task_sched_idx += 1);
  REJECTED(b.off_task_sched_idx += 4);
  REJECTED(b.off_task_sched_idx = (h.off_slice_sched + 4 * h.n_slice_tasks - 1) / R * R);  // on top of the slice schedule's end
  REJECTED(b.off_task_sched_idx += R);
  REJECTED(b.off_task_sched_idx = h.off_task_sched / R * R);
  REJECTED(b.off_task_sched_idx = (h.total_words - R * n_nt) / R * R + R);
  REJECTED(b.off_task_sched_idx = -R);
  REJECTED(b.off_task_sched_idx = 0);
  REJECTED(b.off_slice_sched_idx += 2);
  REJECTED(b.off_slice_sched_idx -= R);
  REJECTED(b.off_slice_sched_idx = h.off_task_sched_idx);
  REJECTED(b.off_slice_sched_idx = (h.total_words - R * h.n_slice_tasks) / R * R + R);
  REJECTED(b.off_slice_sched_idx = -R);
  REJECTED(b.total_words = h.off_slice_sched_idx);
  REJECTED(b.total_words = h.off_slice_sched_idx + R * h.n_slice_tasks - 1);
  REJECTED(b.off_task_sched = 0);
  REJECTED(b.off_slice_sched = 0);
  REJECTED(b.slice_table_copy[0] = 64);
  REJECTED(b.slice_table_copy[8] -= 64);
  REJECTED(b.slice_table_copy[3] += 1);
  REJECTED(b.slice_table_copy[4] = h.slice_table_copy[8] + 64);
  // a header from before the records: the words they took are zero, and the plan passes
  hcspmm_plan_header old = h;
  old.off_task_sched_idx = old.off_slice_sched_idx = 0;
  std::memset(old.slice_table_copy, 0, sizeof(old.slice_table_copy));
  old.total_words = h.off_slice_sched + 4 * (h.total_words - h.off_slice_sched_idx) / R;
  REQUIRE(hcspmm_plan_check(&old, N, E, 0) == HCSPMM_OK);
  std::printf("sched_index_check ok: %d + %d records, %d malformed headers\n", n_nt, h.n_slice_tasks, cases);
  return 0;
}
