// spmm_weighted_h16.hip -- fp16 / bf16 feature instantiations of the edge-weighted hybrid SpMM (spmm_weighted_impl.h): 16-bit X
// and Z, fp32 values, fp32 fma accumulation in the fp32 path's order, one rounding (RNE) per output element.
#include "spmm_weighted_impl.h"

namespace hcspmm {

template <typename E>
static hipError_t plan16_w(const WPlanArgs& a, int vec, hipStream_t stream) {
  if (vec == 8) { HCSPMM_DISPATCH_L(launch_plan_w_LV, E, 8, a.p.panel_cols, a, stream) }
  if (vec == 4) { HCSPMM_DISPATCH_L(launch_plan_w_LV, E, 4, a.p.panel_cols, a, stream) }
  HCSPMM_DISPATCH_L(launch_plan_w_LV, E, 1, a.p.panel_cols, a, stream)
}

template <typename E>
static hipError_t window16_w(const WWindowArgs& a, int vec, hipStream_t stream) {
  if (vec == 8) { HCSPMM_DISPATCH_L(launch_window_w_LV, E, 8, a.w.D, a, stream) }
  if (vec == 4) { HCSPMM_DISPATCH_L(launch_window_w_LV, E, 4, a.w.D, a, stream) }
  HCSPMM_DISPATCH_L(launch_window_w_LV, E, 1, a.w.D, a, stream)
}

hipError_t launch_plan_w_f16(const WPlanArgs& a, int vec, hipStream_t stream) { return plan16_w<F16>(a, vec, stream); }
hipError_t launch_plan_w_bf16(const WPlanArgs& a, int vec, hipStream_t stream) { return plan16_w<BF16>(a, vec, stream); }
hipError_t launch_window_w_f16(const WWindowArgs& a, int vec, hipStream_t stream) { return window16_w<F16>(a, vec, stream); }
hipError_t launch_window_w_bf16(const WWindowArgs& a, int vec, hipStream_t stream) { return window16_w<BF16>(a, vec, stream); }

}  // namespace hcspmm
