// plan_layout.h -- the grid layout of the planned hybrid launch, computed in ONE place for every launcher that shares it:
// launch_plan_LV (spmm_impl.h), launch_plan_w_LV (spmm_weighted_impl.h), launch_plan_wh_LV (spmm_weighted_heads_impl.h,
// direct and indexed) and csr_launch (csr_schedule.h).  Their device decodes all read the fields filled here, so
// the fields must mean the same thing everywhere.  Plain host code: no templates, nothing of HIP beyond PlanArgs.
#pragma once
#include "spmm_kernels.h"

namespace hcspmm {

constexpr int kWaves = 4;  // waves per workgroup (256 threads)
constexpr int kThreads = kWaves * 64;
#ifndef HCSPMM_TINY_KERNEL_T
#define HCSPMM_TINY_KERNEL_T 2  // tiny tasks per lane group in the tiny tasks' own launch (spmm_impl.h tiny_kernel)
#endif

// Fills the launcher-owned fields of b from its plan fields, D and panel_cols; returns the number of column panels of the
// sparse region.  The grid is [sparse region: n_col_panels panels of sparse_wgs_pp workgroups][dense units, kWaves per
// workgroup]; a panel is [slice_wgs XCD-bound workgroups][wide_wgs][ordinary][tiny_wgs][idle padding].
//   L           lanes per task (64 / L tasks per wave)
//   vec         elements per lane of the build; vec_mid the second-widest dense-tile vector (DenseV<vec>::mid).  vec = 0: the
//               launch has no dense-tile lanes of its own and walks the dense windows once per column panel (extremum)
//   tiny_T      tiny tasks per lane group in the launch's own tiny region (TinyT<L> / XTinyT<L>)
//   own_tiny    the tiny tasks run as a launch of their own behind this one (own_tiny_launch; never for the extremum form)
//   fused       PlanArgs::fused of the call.  Bit 1: the ordinary and tiny tasks and the dense windows run in the row-tile
//               fused launch (fused_rows.hip); this launch keeps the sliced region and the wide tasks
inline int plan_launch_layout(PlanArgs& b, int L, int vec, int vec_mid, int tiny_T, bool own_tiny, int fused) {
  const int R = 64 / L;               // tasks per wave
  const int per_wg = kWaves * R;      // ordinary tasks per workgroup
  if (R == 1) b.n_wide = 0;           // with one lane group per wave a wide task is an ordinary one
  if (fused & 2) {
    b.n_tasks = b.n_wide;
    b.n_tiny = 0;
    b.n_dense = b.n_dense_compact = b.n_dense_compact2 = 0;  // (dense windows are tiles of that launch as well)
  }
  b.wide_wgs = (b.n_wide + kWaves - 1) / kWaves;
  // tiny tasks: a region of the hybrid launch, or -- when there are enough of them -- a launch of their own behind it
  b.tiny_kernel_wgs = own_tiny ? (b.n_tiny + per_wg * HCSPMM_TINY_KERNEL_T - 1) / (per_wg * HCSPMM_TINY_KERNEL_T) : 0;
  b.tiny_wgs = own_tiny ? 0 : (b.n_tiny + per_wg * tiny_T - 1) / (per_wg * tiny_T);
  b.free_wgs_pp = b.wide_wgs + (b.n_tasks - b.n_tiny - b.n_wide + per_wg - 1) / per_wg + b.tiny_wgs;
  // the sliced region: per XCD ceil(slice_xcd_tasks / tasks per workgroup) workgroups, interleaved b = x (mod 8); a panel is
  // padded to a multiple of 8 workgroups so that b mod 8 == blockIdx mod 8 in every panel.  The idle ones return at once:
  // the kernels check bf >= free_wgs_pp, because with tiny_wgs = 0 they would otherwise fall into the tiny region
  b.slice_wgs = b.n_slices > 0 ? 8 * ((b.slice_xcd_tasks + per_wg - 1) / per_wg) : 0;
  b.sparse_wgs_pp = b.slice_wgs + b.free_wgs_pp;
  if (b.slice_wgs > 0) b.sparse_wgs_pp = (b.sparse_wgs_pp + 7) & ~7;
  const int n_col_panels = (b.D + b.panel_cols - 1) / b.panel_cols;
  b.sparse_wgs = b.sparse_wgs_pp * n_col_panels;
  if (b.sparse_wgs_pp == 0) b.sparse_wgs_pp = 1;  // divisor in the kernels (sparse_wgs stays 0: no workgroup divides by it)
  // dense-tile panel width: 16*dense_vec columns -- the narrowest of the three lane widths that covers the embedding in ONE panel
  // (a second panel walks the window's column list and gathers its rows again: D = 48 as 32 + 16 columns took 382 us on the
  // YeastH-sized graph where D = 50 in one 64-column panel takes 279, profiles/r04/ab_dense_panels.log), else the widest.  A 16-bit
  // build wider than one element per lane is only launched on even widths (capi.hip pick_vec), so its narrower lanes, the last one
  // moved back, stay on the dword grid.
  if (vec > 0) {
    b.dense_vec = b.D <= 16 ? 1 : (b.D <= 16 * vec_mid ? vec_mid : vec);
    b.n_panels = (b.D + 16 * b.dense_vec - 1) / (16 * b.dense_vec);
  } else {
    b.dense_vec = 0;
    b.n_panels = n_col_panels;
  }
  return n_col_panels;
}

}  // namespace hcspmm
