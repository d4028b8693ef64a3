// spmm_kernels_f8.hip -- 8-bit (OCP e4m3fn) feature instantiations of the hybrid SpMM kernels (spmm_impl.h): the binary
// product of hcspmm_forward_fp8 (no values, no row scales).  Codes are gathered as stored (a quarter of the fp32 bytes),
// widened in registers with v_cvt_pk_f32_fp8 (exact), summed in fp32 in the fp32 path's order and stored as fp32.
// vec = codes per lane access: 8 (8-byte loads, D >= 32) or 4; D, the strides and the bases are on the dword grid.
#include "spmm_impl.h"

namespace hcspmm {

hipError_t launch_plan_f8(const PlanArgs& a, int vec, hipStream_t stream) {
  if (vec == 8) { HCSPMM_DISPATCH_L(launch_plan_LV, F8, 8, a.panel_cols, a, stream) }
  HCSPMM_DISPATCH_L(launch_plan_LV, F8, 4, a.panel_cols, a, stream)
}

hipError_t launch_window_f8(const WindowArgs& a, int vec, hipStream_t stream) {
  if (vec == 8) { HCSPMM_DISPATCH_L(launch_window_LV, F8, 8, a.D, a, stream) }
  HCSPMM_DISPATCH_L(launch_window_LV, F8, 4, a.D, a, stream)
}

}  // namespace hcspmm
