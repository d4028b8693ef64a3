// sampling_arg_codes.cpp -- the argument errors of the entry points that build graphs on the device
// (hcspmm_sample_row_pointers_device, hcspmm_sample_neighbors_device, hcspmm_transpose_graph_device and their workspace
// queries): every failing call returns before a launch, so the pointers -- host arrays here -- are never read and no GPU is
// needed.  Exits 0 when every code is the expected one; prints the ones that are not.
//   hipcc sampling_arg_codes.cpp -I include -L csrc -lhcspmm   (host code only)
#include <climits>
#include <cstdint>
#include <cstdio>

#include "hcspmm.h"

static int g_failures = 0;

static void expect(const char* what, long long got, long long want) {
  if (got != want) {
    std::printf("%s: got %lld, want %lld\n", what, got, want);
    ++g_failures;
  }
}

int main() {
  static int32_t rp[4] = {0, 1, 2, 3}, col[3] = {0, 1, 2}, rp_s[4], col_s[3], eid_s[3], ws[1024];
  const int64_t N = 3, E = 3;
  const int64_t big_n = INT32_MAX, big_e = (int64_t)INT32_MAX + 1;

  // the workspace queries: host arithmetic
  expect("sample ws(N<0)", (long long)hcspmm_sample_workspace_bytes(-1), 0);
  expect("sample ws(3) > 0", hcspmm_sample_workspace_bytes(N) >= sizeof(int32_t), 1);
  expect("sample ws(5000) >= ws(3)", hcspmm_sample_workspace_bytes(5000) >= hcspmm_sample_workspace_bytes(N), 1);
  expect("transpose ws(E=0)", (long long)hcspmm_transpose_graph_device_workspace_bytes(N, N, 0), 0);
  expect("transpose ws(E<0)", (long long)hcspmm_transpose_graph_device_workspace_bytes(N, N, -1), 0);
  expect("transpose ws(M<0)", (long long)hcspmm_transpose_graph_device_workspace_bytes(N, -1, E), 0);
  expect("transpose ws(3) >= two arrays", hcspmm_transpose_graph_device_workspace_bytes(N, N, E) >= 2 * E * sizeof(int32_t), 1);
  const size_t t_need = hcspmm_transpose_graph_device_workspace_bytes(N, N, E);
  expect("transpose ws fits the test buffer", t_need <= sizeof(ws), 1);

  // hcspmm_sample_row_pointers_device
  expect("scan fanout=0", hcspmm_sample_row_pointers_device(rp, N, 0, rp_s, ws, sizeof(ws), nullptr), HCSPMM_EINVAL);
  expect("scan fanout<0", hcspmm_sample_row_pointers_device(rp, N, -3, rp_s, ws, sizeof(ws), nullptr), HCSPMM_EINVAL);
  expect("scan N<0", hcspmm_sample_row_pointers_device(rp, -1, 2, rp_s, ws, sizeof(ws), nullptr), HCSPMM_EINVAL);
  expect("scan rowptr=0", hcspmm_sample_row_pointers_device(nullptr, N, 2, rp_s, ws, sizeof(ws), nullptr), HCSPMM_EINVAL);
  expect("scan out=0", hcspmm_sample_row_pointers_device(rp, N, 2, nullptr, ws, sizeof(ws), nullptr), HCSPMM_EINVAL);
  expect("scan N>range", hcspmm_sample_row_pointers_device(rp, big_n, 2, rp_s, ws, sizeof(ws), nullptr), HCSPMM_ERANGE);
  expect("scan workspace=0", hcspmm_sample_row_pointers_device(rp, N, 2, rp_s, nullptr, sizeof(ws), nullptr), HCSPMM_EWORKSPACE);
  expect("scan short workspace", hcspmm_sample_row_pointers_device(rp, N, 2, rp_s, ws, hcspmm_sample_workspace_bytes(N) - 1, nullptr),
         HCSPMM_EWORKSPACE);

  // hcspmm_sample_neighbors_device
  expect("sample fanout=0", hcspmm_sample_neighbors_device(rp, col, rp_s, N, E, 0, 1, col_s, eid_s, nullptr), HCSPMM_EINVAL);
  expect("sample N<0", hcspmm_sample_neighbors_device(rp, col, rp_s, -1, E, 2, 1, col_s, eid_s, nullptr), HCSPMM_EINVAL);
  expect("sample E<0", hcspmm_sample_neighbors_device(rp, col, rp_s, N, -1, 2, 1, col_s, eid_s, nullptr), HCSPMM_EINVAL);
  expect("sample rowptr=0", hcspmm_sample_neighbors_device(nullptr, col, rp_s, N, E, 2, 1, col_s, eid_s, nullptr), HCSPMM_EINVAL);
  expect("sample col=0", hcspmm_sample_neighbors_device(rp, nullptr, rp_s, N, E, 2, 1, col_s, eid_s, nullptr), HCSPMM_EINVAL);
  expect("sample rowptr_s=0", hcspmm_sample_neighbors_device(rp, col, nullptr, N, E, 2, 1, col_s, eid_s, nullptr), HCSPMM_EINVAL);
  expect("sample col_s=0", hcspmm_sample_neighbors_device(rp, col, rp_s, N, E, 2, 1, nullptr, eid_s, nullptr), HCSPMM_EINVAL);
  expect("sample eid_s=0", hcspmm_sample_neighbors_device(rp, col, rp_s, N, E, 2, 1, col_s, nullptr, nullptr), HCSPMM_EINVAL);
  expect("sample N>range", hcspmm_sample_neighbors_device(rp, col, rp_s, big_n, E, 2, 1, col_s, eid_s, nullptr), HCSPMM_ERANGE);
  expect("sample E>range", hcspmm_sample_neighbors_device(rp, col, rp_s, N, big_e, 2, 1, col_s, eid_s, nullptr), HCSPMM_ERANGE);
  // nothing to sample: OK without a launch (and without the entry arrays)
  expect("sample E=0", hcspmm_sample_neighbors_device(rp, nullptr, rp_s, N, 0, 2, 1, nullptr, nullptr, nullptr), HCSPMM_OK);
  expect("sample N=0", hcspmm_sample_neighbors_device(rp, col, rp_s, 0, E, 2, 1, col_s, eid_s, nullptr), HCSPMM_OK);

  // hcspmm_transpose_graph_device
  expect("transpose N<0", hcspmm_transpose_graph_device(rp, col, -1, N, E, rp_s, col_s, eid_s, ws, sizeof(ws), nullptr), HCSPMM_EINVAL);
  expect("transpose M<0", hcspmm_transpose_graph_device(rp, col, N, -1, E, rp_s, col_s, eid_s, ws, sizeof(ws), nullptr), HCSPMM_EINVAL);
  expect("transpose E<0", hcspmm_transpose_graph_device(rp, col, N, N, -1, rp_s, col_s, eid_s, ws, sizeof(ws), nullptr), HCSPMM_EINVAL);
  expect("transpose rowptr=0", hcspmm_transpose_graph_device(nullptr, col, N, N, E, rp_s, col_s, eid_s, ws, sizeof(ws), nullptr),
         HCSPMM_EINVAL);
  expect("transpose col=0", hcspmm_transpose_graph_device(rp, nullptr, N, N, E, rp_s, col_s, eid_s, ws, sizeof(ws), nullptr),
         HCSPMM_EINVAL);
  expect("transpose rowptr_t=0", hcspmm_transpose_graph_device(rp, col, N, N, E, nullptr, col_s, eid_s, ws, sizeof(ws), nullptr),
         HCSPMM_EINVAL);
  expect("transpose col_t=0", hcspmm_transpose_graph_device(rp, col, N, N, E, rp_s, nullptr, eid_s, ws, sizeof(ws), nullptr),
         HCSPMM_EINVAL);
  expect("transpose eid_t=0", hcspmm_transpose_graph_device(rp, col, N, N, E, rp_s, col_s, nullptr, ws, sizeof(ws), nullptr),
         HCSPMM_EINVAL);
  expect("transpose M>range", hcspmm_transpose_graph_device(rp, col, N, big_n, E, rp_s, col_s, eid_s, ws, sizeof(ws), nullptr),
         HCSPMM_ERANGE);
  expect("transpose E>range", hcspmm_transpose_graph_device(rp, col, N, N, big_e, rp_s, col_s, eid_s, ws, sizeof(ws), nullptr),
         HCSPMM_ERANGE);
  expect("transpose workspace=0", hcspmm_transpose_graph_device(rp, col, N, N, E, rp_s, col_s, eid_s, nullptr, sizeof(ws), nullptr),
         HCSPMM_EWORKSPACE);
  expect("transpose short workspace", hcspmm_transpose_graph_device(rp, col, N, N, E, rp_s, col_s, eid_s, ws, t_need - 1, nullptr),
         HCSPMM_EWORKSPACE);

  if (g_failures == 0) std::printf("ok\n");
  return g_failures == 0 ? 0 : 1;
}
