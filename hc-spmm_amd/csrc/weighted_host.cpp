// weighted_host.cpp -- host side of the edge-weighted product's backward (include/hcspmm.h hcspmm_transpose_permutation,
// hcspmm_transpose_graph).
#include <stdint.h>

#include <vector>

#include "hcspmm.h"

// For a pattern-symmetric CSR graph, the transpose A_w^T has A's pattern, and its entry (r, c) is A_w's entry (c, r).  Row c's
// entries are visited in CSR order (columns ascending), so for every row r the entries (c, r) arrive in ascending c -- the
// order of row r's own entries: a cursor per row pairs them up in one pass.  Any mismatch means the pattern is not
// symmetric (or a row is not strictly ascending).
extern "C" int hcspmm_transpose_permutation(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t E, int32_t* perm) {
  if (N < 0 || E < 0 || !rowptr || (E > 0 && (!col || !perm))) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  if (rowptr[0] != 0 || rowptr[N] != E) return HCSPMM_EINVAL;
  for (int64_t r = 0; r < N; ++r)
    if (rowptr[r + 1] < rowptr[r]) return HCSPMM_EINVAL;
  std::vector<int32_t> cursor(rowptr, rowptr + N);
  for (int64_t c = 0; c < N; ++c) {
    for (int32_t e = rowptr[c]; e < rowptr[c + 1]; ++e) {
      const int32_t r = col[e];
      if (r < 0 || r >= N) return HCSPMM_EINVAL;
      const int32_t q = cursor[(size_t)r];
      if (q >= rowptr[r + 1] || col[q] != (int32_t)c) return HCSPMM_EINVAL;  // (c, r) stored but not (r, c) -- or not in order
      perm[q] = e;  // A^T(r, c) = A(c, r): entry q of row r takes the value of entry e
      cursor[(size_t)r] = q + 1;
    }
  }
  for (int64_t r = 0; r < N; ++r)
    if (cursor[(size_t)r] != rowptr[r + 1]) return HCSPMM_EINVAL;  // (r, c) stored but not (c, r)
  return HCSPMM_OK;
}

// The general transpose (hcspmm_transpose_graph): a counting sort by column.  Rows are visited in ascending order, so row j of
// A^T receives its entries (i, j) in ascending i: A^T's columns are strictly ascending whenever A's are.  Everything is
// validated in the counting pass, before the outputs are written.
extern "C" int hcspmm_transpose_graph(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t M, int64_t E,
                                      int32_t* rowptr_t, int32_t* col_t, int32_t* entry_t) {
  if (N < 0 || M < 0 || E < 0 || !rowptr || !rowptr_t || (E > 0 && (!col || !col_t || !entry_t))) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || M > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  if (rowptr[0] != 0 || rowptr[N] != E) return HCSPMM_EINVAL;
  std::vector<int32_t> cursor((size_t)M + 1, 0);  // cursor[j + 1] = entries of column j, then the running row starts
  for (int64_t r = 0; r < N; ++r) {
    if (rowptr[r + 1] < rowptr[r] || rowptr[r + 1] > E) return HCSPMM_EINVAL;
    int32_t prev = -1;
    for (int32_t e = rowptr[r]; e < rowptr[r + 1]; ++e) {
      const int32_t c = col[e];
      if (c <= prev || c >= M) return HCSPMM_EINVAL;  // outside [0, num_cols), or not strictly ascending
      prev = c;
      ++cursor[(size_t)c + 1];
    }
  }
  rowptr_t[0] = 0;
  for (int64_t j = 0; j < M; ++j) {
    cursor[(size_t)j + 1] += cursor[(size_t)j];
    rowptr_t[j + 1] = cursor[(size_t)j + 1];
  }
  for (int64_t r = 0; r < N; ++r) {
    for (int32_t e = rowptr[r]; e < rowptr[r + 1]; ++e) {
      const int32_t q = cursor[(size_t)col[e]]++;
      col_t[q] = (int32_t)r;
      entry_t[q] = e;
    }
  }
  return HCSPMM_OK;
}
