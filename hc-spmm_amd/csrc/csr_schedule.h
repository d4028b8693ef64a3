// csr_schedule.h -- the schedule of the launches that serve EVERY row from CSR on the binary product's plan, written once
// (DESIGN.md section 3.20): spmm_extremum.hip, spmm_multi.hip, spmm_softmax.hip, softmax_aggr_grad.hip and the edge-feature
// message unit.  Their reductions cannot go through MFMA, so a dense-tile window's rows are sparse-row tasks too, and what is
// left of the hybrid launch (spmm_impl.h hybrid_plan_kernel) is a walk that hands tasks to a body:
//   csr_plan_walk    planned kernel: sliced | wide | ordinary | tiny regions per column panel, then one wave per (dense-tile
//                    window, column panel) serving the window's 16 rows
//   csr_window_walk  plan-free kernel: one workgroup per 16-row window
//   fixup_of_slot    the split row that owns a partial slot (the weighted launches' tiny tasks use it as well)
//   csr_launch       host: plan-free, or planned + fix-up
//   csr_dispatch     host: lanes per task and elements per lane, from the width
// A family supplies a body
//   Dst dst(int row, int slot) const;
//   template <bool WIDE> void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const;
//   void tiny(int first, int c0, int cend, int lane) const;
// dst: where a task's result goes, Z[row] (slot < 0) or partial slot `slot`, in the form the family's task body takes (RowSlot,
// or pointers); it is called where the descriptor is decoded, under the lanes' own condition, and a value-initialised Dst is a
// lane group without a task (slice padding included).  That group still runs task: the task bodies shuffle across the wave.
// task: entries [e0, e0 + n) over columns [c0, cend).  WIDE: the whole wave owns the task, e0 and n are wave-uniform.
// tiny: the T tasks per lane group from descriptor `first` on, T the family's tiny-task count (it sizes the region in
// plan_launch_layout as well).
#pragma once
#include <type_traits>

#include "spmm_impl.h"

namespace hcspmm {

// the fix-up record (row, first slot, slot count, -) of the split row that owns partial slot s: the list is ascending in its
// first slot, and segment k of a row covers entries rowptr[row] + k * segment_len ... (plan_host.cpp)
__device__ __forceinline__ int4 fixup_of_slot(const PlanArgs& a, int s) {
  const int4* fix = reinterpret_cast<const int4*>(a.plan + a.off_fixups);
  int lo = 0, hi = a.n_split_rows;  // largest i with fix[i].y <= s
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (fix[mid].y <= s) lo = mid;
    else hi = mid;
  }
  return fix[lo];
}
// first CSR entry of the split-row segment that owns partial slot s
__device__ __forceinline__ int segment_entry(const PlanArgs& a, const int* rowptr, int segment_len, int s) {
  const int4 f = fixup_of_slot(a, s);
  return rowptr[f.x] + (s - f.y) * segment_len;
}

// the destination of the families whose store takes (row, slot) as they are
struct RowSlot {
  int row = -1, slot = -1;
};

// the 16 rows of a window from CSR, R = 64 / L at a time
template <int L, typename Body>
__device__ __forceinline__ void csr_window_rows(const PlanArgs& a, const int* rowptr, const Body& body, int window, int c0,
                                                int cend, int lane) {
  constexpr int R = 64 / L;
  const int g = lane / L;
  for (int rb = 0; rb < 16; rb += R) {
    const int r = window * 16 + rb + g;
    int e0 = 0, n = 0;
    typename Body::Dst o{};
    if (rb + g < 16 && r < a.N) {
      e0 = rowptr[r];
      n = rowptr[r + 1] - e0;
      o = body.dst(r, -1);
    }
    body.template task<false>(o, e0, n, c0, cend, lane);
  }
}

// Planned kernel: hybrid_plan_kernel's regions (sliced | wide | ordinary | tiny per column panel), then one wave per
// (dense-tile window, column panel) serving the window's rows from CSR.  Tiny tasks always run in their region here.
template <int L, int T, typename Body>
__device__ __forceinline__ void csr_plan_walk(const PlanArgs& a, const int* rowptr, const Body& body) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if ((int)blockIdx.x < a.sparse_wgs) {
    const int p = (int)blockIdx.x / a.sparse_wgs_pp;
    const int b = (int)blockIdx.x - p * a.sparse_wgs_pp;
    const int c0 = p * a.panel_cols;
    const int cend = min(a.D, c0 + a.panel_cols);
    const int bf = b - a.slice_wgs;
    if (bf >= 0 && bf < a.wide_wgs) {
      const int tid = bf * kWaves + wave;
      if (tid >= a.n_wide) return;
      const int4 t = reinterpret_cast<const int4*>(a.plan + a.off_tasks)[tid];
      body.template task<true>(body.dst(t.x, t.w), __builtin_amdgcn_readfirstlane(t.y), __builtin_amdgcn_readfirstlane(t.z), c0, cend,
                               lane);
    } else if (bf >= sparse_wgs_pp_ordinary_end(a)) {
      if (bf >= a.free_wgs_pp) return;
      constexpr int R = 64 / L;
      const int first = a.n_tasks - a.n_tiny + ((bf - sparse_wgs_pp_ordinary_end(a)) * kWaves + wave) * (R * T);
      if (first >= a.n_tasks) return;
      body.tiny(first, c0, cend, lane);
    } else {
      constexpr int R = 64 / L;
      const int g = lane / L;
      const int4* tp = nullptr;
      if (bf < 0) {
        cint_p tbl = (cint_p)(a.plan + a.off_slice_table);
        int j = ((b >> 3) * kWaves + wave) * R;
        for (int sl = b & 7; sl < a.n_slices; sl += 8) {
          const int lo = tbl[sl], cnt = tbl[sl + 1] - lo;
          if (j < cnt) {
            tp = reinterpret_cast<const int4*>(a.plan + a.off_slice_tasks) + lo + j + g;
            break;
          }
          j -= cnt;
        }
      } else {
        const int tid = a.n_wide + ((bf - a.wide_wgs) * kWaves + wave) * R + g;
        if (tid < a.n_tasks - a.n_tiny) tp = reinterpret_cast<const int4*>(a.plan + a.off_tasks) + tid;
      }
      int e0 = 0, n = 0;
      typename Body::Dst o{};
      if (tp != nullptr) {
        const int4 t = *tp;
        if (t.x >= 0) {  // (slice padding: row -1)
          e0 = t.y;
          n = t.z;
          o = body.dst(t.x, t.w);
        }
      }
      body.template task<false>(o, e0, n, c0, cend, lane);
    }
  } else {
    const int n_col_panels = (a.D + a.panel_cols - 1) / a.panel_cols;
    const int unit = ((int)blockIdx.x - a.sparse_wgs) * kWaves + wave;
    if (unit >= a.n_dense * n_col_panels) return;
    const int p = unit / a.n_dense, di = unit - p * a.n_dense;
    const int n_reg = a.n_dense - a.n_dense_compact - a.n_dense_compact2;
    int window;  // the first word of the window's record, whatever its kind
    if (di < n_reg) window = ((cint_p)(a.plan + a.off_dense_index))[4 * di];
    else if (di < n_reg + a.n_dense_compact2) window = ((cint_p)(a.plan + a.off_dense_compact2))[(di - n_reg) * HCSPMM_COMPACT2_WORDS];
    else window = ((cint_p)(a.plan + a.off_dense_compact))[(di - n_reg - a.n_dense_compact2) * HCSPMM_COMPACT_WORDS];
    const int c0 = p * a.panel_cols;
    csr_window_rows<L>(a, rowptr, body, window, c0, min(a.D, c0 + a.panel_cols), lane);
  }
}

// Plan-free kernel: one workgroup per 16-row window, every window (dense-tile or not) served from CSR: rows up to
// kPlanFreeWide entries by one lane group each, longer ones by whole waves (hybrid_window_kernel's sparse branch)
template <int L, typename Body>
__device__ __forceinline__ void csr_window_walk(const PlanArgs& a, const int* rowptr, const Body& body) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = (int)blockDim.x >> 6;
  const int r0 = (int)blockIdx.x * 16, r1 = min(r0 + 16, a.N);
  constexpr int R = 64 / L;
  const int G = R * nwaves;
  const int gi = wave * R + lane / L;
  for (int rb = r0; rb < r1; rb += G) {
    const int r = rb + gi;
    int e0 = 0, n = 0;
    typename Body::Dst o{};
    if (r < r1) {
      e0 = rowptr[r];
      n = rowptr[r + 1] - e0;
      if (R == 1 || n <= kPlanFreeWide) o = body.dst(r, -1);
      else n = 0;  // left to the whole-wave pass below
    }
    body.template task<false>(o, e0, n, 0, a.D, lane);
  }
  if (R > 1) {
    int k = 0;
    for (int r = r0; r < r1; ++r) {
      const int e0 = rowptr[r];
      const int n = rowptr[r + 1] - e0;
      if (n > kPlanFreeWide) {
        if (k % nwaves == wave) body.template task<true>(body.dst(r, -1), e0, n, 0, a.D, lane);
        ++k;
      }
    }
  }
}

// Host: the plan-free launch (args.p.plan == nullptr), or the planned launch on the shared layout (plan_layout.h: T tiny
// tasks per lane group in their region, no launch of their own; dense windows once per column panel) and, with split rows,
// the fix-up launch behind it.  The fix-up kernel takes the family's arguments or, for plain fp32 sums, the PlanArgs alone.
template <typename Args, typename FArgs>
hipError_t csr_launch(const Args& args, int L, int T, void (*window_kernel)(Args), void (*plan_kernel)(Args),
                      void (*fixup)(FArgs), hipStream_t stream) {
  Args b = args;
  PlanArgs& p = b.p;
  if (p.plan == nullptr) {
    const int W = (p.N + 15) / 16;
    int waves = (16 * L + 63) / 64;
    if (waves > kWaves) waves = kWaves;
    if (W > 0) hipLaunchKernelGGL(window_kernel, dim3(W), dim3(waves * 64), 0, stream, b);
    return hipGetLastError();
  }
  p.fused = 0;
  const int n_col_panels = plan_launch_layout(p, L, 0, 0, T, false, 0);
  const long long dense_wgs = ((long long)p.n_dense * n_col_panels + kWaves - 1) / kWaves;
  const long long grid = (long long)p.sparse_wgs + dense_wgs;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (grid > 0) hipLaunchKernelGGL(plan_kernel, dim3((unsigned)grid), dim3(kThreads), 0, stream, b);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || p.n_split_rows == 0) return e;
  const int fg = (p.n_split_rows + kWaves - 1) / kWaves;
  if constexpr (std::is_same<FArgs, PlanArgs>::value) hipLaunchKernelGGL(fixup, dim3(fg), dim3(kThreads), 0, stream, p);
  else hipLaunchKernelGGL(fixup, dim3(fg), dim3(kThreads), 0, stream, b);
  return hipGetLastError();
}

// Host: f(LanesVec<L, VEC>{}) for the build that serves the width: 16-byte lanes and L = pick_L of the panel (planned) or of D
// (plan-free) at vec == 4, four lanes of 2 or 1 elements for D = 2, 3 / 1
template <int L_, int VEC_> struct LanesVec {
  static constexpr int L = L_, VEC = VEC_;
};
template <typename F>
hipError_t csr_dispatch(const PlanArgs& p, int vec, F&& f) {
  if (vec == 4) {
    switch (pick_L(p.plan != nullptr ? p.panel_cols : p.D, 4)) {
      case 4: return f(LanesVec<4, 4>{});
      case 8: return f(LanesVec<8, 4>{});
      case 16: return f(LanesVec<16, 4>{});
      case 32: return f(LanesVec<32, 4>{});
      default: return f(LanesVec<64, 4>{});
    }
  }
  if (p.D > 4 * vec) return hipErrorInvalidValue;
  if (vec == 2) return f(LanesVec<4, 2>{});
  return f(LanesVec<4, 1>{});
}

}  // namespace hcspmm
