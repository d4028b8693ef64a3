// spmm_weighted_indexed.hip -- multi-head edge-weighted hybrid SpMM with indexed values (hcspmm_forward_weighted_indexed;
// DESIGN.md section 3.14):
//   Z[r][h*Dh + j] = sum over the entries e of row r of values[h*nV + vindex[e]] * X[col(e)][h*Dh + j],   D = heads * Dh, fp32.
// The indexed form of spmm_weighted_heads_impl.h (vindex = the transposed graph's entry_index_t, or
// hcspmm_transpose_permutation's perm): its shape check and its builds.
#include "spmm_weighted_heads_impl.h"

namespace hcspmm {
namespace {
template <typename E, int L, int VEC> hipError_t plan_LV(const WHPlanArgs& a, hipStream_t s) { return launch_plan_wh_LV<E, L, VEC, true>(a, s); }
template <typename E, int L, int VEC> hipError_t window_LV(const WHWindowArgs& a, hipStream_t s) { return launch_window_wh_LV<E, L, VEC, true>(a, s); }

// fp32 only.  16-byte lanes: D = heads * Dh with Dh % 4 == 0, or one head of any D >= 4 (lane_col moves the last lane back,
// as in the weighted kernels: with one head there is nothing to span); one head of D < 4 takes the 8 / 4-byte lanes.
bool wi_shape_ok(int vec, int D, int dh) {
  if (dh <= 0 || D % dh != 0) return false;
  return dh == D ? (vec == 4 || vec == 2 || vec == 1) : (vec == 4 && dh % 4 == 0);
}
}  // namespace

hipError_t launch_plan_wi_f32(const WHPlanArgs& a, int vec, hipStream_t stream) {
  if (!wi_shape_ok(vec, a.w.p.D, a.dh)) return hipErrorInvalidValue;
  if (vec == 4) { HCSPMM_DISPATCH_L(plan_LV, F32, 4, a.w.p.panel_cols, a, stream) }
  if (a.w.p.D > 4 * vec) return hipErrorInvalidValue;
  if (vec == 2) return plan_LV<F32, 4, 2>(a, stream);
  return plan_LV<F32, 4, 1>(a, stream);
}

hipError_t launch_window_wi_f32(const WHWindowArgs& a, int vec, hipStream_t stream) {
  if (!wi_shape_ok(vec, a.w.w.D, a.dh)) return hipErrorInvalidValue;
  if (vec == 4) { HCSPMM_DISPATCH_L(window_LV, F32, 4, a.w.w.D, a, stream) }
  if (a.w.w.D > 4 * vec) return hipErrorInvalidValue;
  if (vec == 2) return window_LV<F32, 4, 2>(a, stream);
  return window_LV<F32, 4, 1>(a, stream);
}

}  // namespace hcspmm
