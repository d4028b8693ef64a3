// spmm_weighted_heads.hip -- multi-head edge-weighted hybrid SpMM (hcspmm_forward_weighted_heads):
//   Z[r][h*Dh + j] = sum over the entries e of row r of values[h*E + e] * X[col(e)][h*Dh + j],   D = heads * Dh, fp32.
// The direct form of spmm_weighted_heads_impl.h (values aligned with column_index): its shape check and its builds.
#include "spmm_weighted_heads_impl.h"

namespace hcspmm {
namespace {
template <typename E, int L, int VEC> hipError_t plan_LV(const WHPlanArgs& a, hipStream_t s) { return launch_plan_wh_LV<E, L, VEC, false>(a, s); }
template <typename E, int L, int VEC> hipError_t window_LV(const WHWindowArgs& a, hipStream_t s) { return launch_window_wh_LV<E, L, VEC, false>(a, s); }

// fp32 only, 16-byte lanes: D = heads * Dh with Dh % 4 == 0 is always at least 4 columns (pick_vec's vec 4)
bool wh_shape_ok(int vec, int D, int dh) { return vec == 4 && dh > 0 && dh % 4 == 0 && D % dh == 0; }
}  // namespace

hipError_t launch_plan_wh_f32(const WHPlanArgs& a, int vec, hipStream_t stream) {
  if (!wh_shape_ok(vec, a.w.p.D, a.dh)) return hipErrorInvalidValue;
  HCSPMM_DISPATCH_L(plan_LV, F32, 4, a.w.p.panel_cols, a, stream)
}

hipError_t launch_window_wh_f32(const WHWindowArgs& a, int vec, hipStream_t stream) {
  if (!wh_shape_ok(vec, a.w.w.D, a.dh)) return hipErrorInvalidValue;
  HCSPMM_DISPATCH_L(window_LV, F32, 4, a.w.w.D, a, stream)
}

}  // namespace hcspmm
