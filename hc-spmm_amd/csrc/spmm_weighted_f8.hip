// spmm_weighted_f8.hip -- 8-bit (OCP e4m3fn) feature instantiations of the edge-weighted hybrid SpMM (spmm_weighted_impl.h):
// the weighted / scaled product of hcspmm_forward_fp8.  Entry e of column c weighs values[e] * row_scale[c] (WPlanArgs::row_scale), every
// step is acc = fmaf(w, widen(code), acc) in the fp32 path's order, the sums are stored as fp32.
#include "spmm_weighted_impl.h"

namespace hcspmm {

hipError_t launch_plan_w_f8(const WPlanArgs& a, int vec, hipStream_t stream) {
  if (vec == 8) { HCSPMM_DISPATCH_L(launch_plan_w_LV, F8, 8, a.p.panel_cols, a, stream) }
  HCSPMM_DISPATCH_L(launch_plan_w_LV, F8, 4, a.p.panel_cols, a, stream)
}

hipError_t launch_window_w_f8(const WWindowArgs& a, int vec, hipStream_t stream) {
  if (vec == 8) { HCSPMM_DISPATCH_L(launch_window_w_LV, F8, 8, a.w.D, a, stream) }
  HCSPMM_DISPATCH_L(launch_window_w_LV, F8, 4, a.w.D, a, stream)
}

}  // namespace hcspmm
