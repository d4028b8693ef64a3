// spmm_weighted.hip -- fp32 instantiations of the edge-weighted hybrid SpMM (spmm_weighted_impl.h holds the device code),
// and the device-side edge normalisations the weighted GCN layers use.
#include "spmm_weighted_impl.h"

namespace hcspmm {

hipError_t launch_plan_w_f32(const WPlanArgs& a, int vec, hipStream_t stream) {
  if (vec == 4) { HCSPMM_DISPATCH_L(launch_plan_w_LV, F32, 4, a.p.panel_cols, a, stream) }
  if (a.p.D > 4 * vec) return hipErrorInvalidValue;
  if (vec == 2) return launch_plan_w_LV<F32, 4, 2>(a, stream);
  return launch_plan_w_LV<F32, 4, 1>(a, stream);
}

hipError_t launch_window_w_f32(const WWindowArgs& a, int vec, hipStream_t stream) {
  if (vec == 4) { HCSPMM_DISPATCH_L(launch_window_w_LV, F32, 4, a.w.D, a, stream) }
  if (a.w.D > 4 * vec) return hipErrorInvalidValue;
  if (vec == 2) return launch_window_w_LV<F32, 4, 2>(a, stream);
  return launch_window_w_LV<F32, 4, 1>(a, stream);
}

namespace {
// one thread per entry: its row by binary search in rowptr (as edge_to_row_kernel in capi.hip), the degrees are row lengths
__global__ __launch_bounds__(256) void edge_norm_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, int N,
                                                        long long E, int kind, float* __restrict__ values) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
    int lo = 0, hi = N;  // invariant: rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if ((long long)rowptr[mid] <= e) lo = mid;
      else hi = mid;
    }
    const float dr = (float)(rowptr[lo + 1] - rowptr[lo]);
    if (kind == 0) {
      const int c = col[e];
      const float dc = (float)(rowptr[c + 1] - rowptr[c]);
      values[e] = 1.0f / sqrtf(dr * dc);  // correctly rounded sqrt and division (no fast-math here)
    } else {
      values[e] = 1.0f / dr;
    }
  }
}
}  // namespace

hipError_t launch_edge_norm(const int* rowptr, const int* col, int N, long long E, int kind, float* values, hipStream_t stream) {
  if (E == 0) return hipSuccess;
  long long blocks = (E + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(edge_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, rowptr, col, N, E, kind, values);
  return hipGetLastError();
}

}  // namespace hcspmm
