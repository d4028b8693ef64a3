// softmax_aggr_grad.hip -- gradient of the softmax aggregation with respect to X (hcspmm_softmax_backward, DESIGN.md section
// 3.18), fp32 on the plan of the graph the backward walks (A^T's, or A's own for a symmetric pattern):
//   dX[j][d] = sum over the entries (j, i) of row j of  exp(s_j - M[i][d]) / L[i][d] * G[i][d] * (1 + beta[d] (x_j - Z[i][d])),
//   x_j = X[j][d], s_j = fl(beta[d] * x_j)
// The softmax weight of entry (i, j) of A is recomputed from the forward's M and L: no [E, D] tensor, no transpose
// permutation.  On the true transpose s_j <= M[i] (j is among row i's entries), so the exponent is <= 0, and L >= 1.
//
// A plain-sum sparse-row launch on the weighted launches' schedule (spmm_weighted_impl.h: sliced | wide | ordinary | tiny
// regions per column panel), with the dense-tile windows served from CSR by the task body as in spmm_multi.hip, fixup_kernel's
// pass over split rows and a plan-free window kernel.
//  * Every entry issues FOUR 16-byte loads per lane (G, Z, M, L rows of one stride through col[e]); two entries are in flight
//    per lane, the binary gather's eight loads.
//  * The task's own row of X and beta are per-lane constants of a column chunk.  A tiny task that carries a partial slot
//    instead of its row finds the row through the fix-up list.
//  * Sums run in hcspmm_forward_weighted's order: CSR order on ordinary and tiny tasks, the wide tasks' xor-shuffle tree, fp32
//    partials of sliced and segmented rows added by the fix-up pass in fixup_kernel's order.  No atomics.
#include "spmm_impl.h"

namespace hcspmm {
namespace {

constexpr int kGradU = 2;  // entries in flight per lane: eight 16-byte loads
constexpr float kLog2e = 1.44269504088896340736f;

// per-lane constants of a column chunk: the task's own x, beta and s = fl(beta x)
template <int VEC> struct GOwn {
  typename AccT<VEC>::type x, b, s;
};

template <int VEC>
__device__ __forceinline__ GOwn<VEC> gown(const SGradArgs& ga, int row, int c) {
  typedef Lane<F32, VEC> Ln;
  GOwn<VEC> o;
  o.b = Ln::load(ga.beta + c);
  o.x = row >= 0 ? Ln::load(reinterpret_cast<const float*>(ga.p.X) + (size_t)row * ga.p.ldx + c) : azero<VEC>();
#pragma unroll
  for (int q = 0; q < VEC; ++q) aset(o.s, q, __fmul_rn(aget(o.b, q), aget(o.x, q)));
  return o;
}

// one entry: VEC columns of the gathered G, Z, M, L rows
template <int VEC>
__device__ __forceinline__ void gstep(typename AccT<VEC>::type& acc, const GOwn<VEC>& o, const typename AccT<VEC>::type& g,
                                      const typename AccT<VEC>::type& z, const typename AccT<VEC>::type& m,
                                      const typename AccT<VEC>::type& l) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    const float p = __builtin_amdgcn_exp2f(__fsub_rn(aget(o.s, q), aget(m, q)) * kLog2e) * __builtin_amdgcn_rcpf(aget(l, q));
    const float k = __builtin_fmaf(aget(o.b, q), __fsub_rn(aget(o.x, q), aget(z, q)), 1.0f);
    aset(acc, q, __builtin_fmaf(p * aget(g, q), k, aget(acc, q)));
  }
}

// One branch-free batch of UB entries (spmm_impl.h gather_batch): lanes past a task's end hold idx -1, re-read row 0 and take
// nothing
template <int VEC, int UB>
__device__ __forceinline__ void gbatch(const SGradArgs& ga, int csafe, bool cok, int myidx, int src0, const GOwn<VEC>& o,
                                       typename AccT<VEC>::type& acc) {
  typedef Lane<F32, VEC> Ln;
  int idx[UB];
  typename AccT<VEC>::type g[UB], z[UB], m[UB], l[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = __shfl(myidx, src0 + u, 64);
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const size_t off = (size_t)max(idx[u], 0) * ga.ld_in + csafe;
    g[u] = Ln::load(ga.G + off);
    z[u] = Ln::load(ga.Zf + off);
    m[u] = Ln::load(ga.M + off);
    l[u] = Ln::load(ga.L + off);
  }
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && idx[u] >= 0) gstep<VEC>(acc, o, g[u], z[u], m[u], l[u]);
}

// sparse_task_w (spmm_weighted_impl.h) with the gradient step: L lanes own the task = entries [e0, e0 + n) of row `row` (< 0: a
// lane group without a task); WIDE: the whole wave owns it and the 64/L lane-group sums are combined by the fixed tree
template <int L, int VEC, bool WIDE>
__device__ __forceinline__ void gtask(const SGradArgs& ga, int row, float* dz, float* dp, int e0, int n, int c0, int cend, int lane) {
  typedef Lane<F32, VEC> Ln;
  constexpr int U = (L < kGradU) ? L : kGradU;
  constexpr int STRIDE = WIDE ? 64 : L;
  const int* __restrict__ col = ga.p.col;
  const int s = lane & (L - 1);
  const int pos = WIDE ? lane : s;
  const int gbase = lane & ~(L - 1);
  int nmax = n;
  if (!WIDE) {
#pragma unroll
    for (int off = L; off < 64; off <<= 1) nmax = max(nmax, __shfl_xor(nmax, off, 64));
  }
  nmax = __builtin_amdgcn_readfirstlane(nmax);

  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const bool cok = pbase + s * VEC < cend;
    const int c = cok ? lane_col<VEC>(pbase + s * VEC, cend) : 0;
    const GOwn<VEC> o = gown<VEC>(ga, row, c);
    typename AccT<VEC>::type acc = azero<VEC>();
    int next = pos < n ? col[e0 + pos] : -1;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      next = base + STRIDE + pos < n ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      const int cnt = min(L, nmax - base);
      for (int j = 0; j < cnt;) {
        if (U >= 2 && cnt - j > 1) {
          gbatch<VEC, U>(ga, c, cok, myidx, gbase + j, o, acc);
          j += U;
        } else {
          gbatch<VEC, 1>(ga, c, cok, myidx, gbase + j, o, acc);
          j += 1;
        }
      }
    }
    if (WIDE) {
#pragma unroll
      for (int off = L; off < 64; off <<= 1) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) aset(acc, q, aget(acc, q) + __shfl_xor(aget(acc, q), off, 64));
      }
    }
    if (cok && (!WIDE || lane < L)) {
      if (dz != nullptr) Ln::store(dz + c, acc);
      else if (dp != nullptr) Ln::store_partial(dp + c, acc);
    }
  }
}

// destinations of a task descriptor (row | first entry | length | partial slot or -1)
struct GDst {
  float* z;
  float* p;
};
__device__ __forceinline__ GDst task_dst(const SGradArgs& ga, int row, int slot) {
  const PlanArgs& a = ga.p;
  GDst d{nullptr, nullptr};
  if (slot < 0) d.z = reinterpret_cast<float*>(a.Z) + (size_t)row * a.ldz;
  else d.p = a.partial + (size_t)slot * (size_t)a.D;
  return d;
}

// the split row that owns partial slot s (the search of spmm_multi.hip msegment_entry)
__device__ __forceinline__ int gsegment_row(const SGradArgs& ga, int s) {
  const int4* fix = reinterpret_cast<const int4*>(ga.p.plan + ga.p.off_fixups);
  int lo = 0, hi = ga.p.n_split_rows;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (fix[mid].y <= s) lo = mid;
    else hi = mid;
  }
  return fix[lo].x;
}

// tiny_tasks_w (spmm_weighted_impl.h), one task of at most two entries per lane group (eight loads), column ids inline in the
// descriptor; the own row comes from the descriptor (a whole row) or the fix-up list (the last segment of a split row)
template <int L, int VEC>
__device__ __forceinline__ void gtiny(const SGradArgs& ga, int first, int c0, int cend, int lane) {
  typedef Lane<F32, VEC> Ln;
  typedef typename AccT<VEC>::type acc_t;
  const PlanArgs& a = ga.p;
  const int g = lane / L, s = lane & (L - 1);
  const int tid = first + g;
  const int4 d = (tid < a.n_tasks) ? reinterpret_cast<const int4*>(a.plan + a.off_tasks)[tid] : int4{0, -1, -1, -1};
  const bool any1 = __builtin_amdgcn_ballot_w64(d.y >= 0) != 0, any2 = __builtin_amdgcn_ballot_w64(d.w >= 0) != 0;
  int row = -1;
  if (d.z >= 0) row = d.x >= 0 ? d.x : gsegment_row(ga, -(d.x + 1));
  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const bool cok = pbase + s * VEC < cend;
    const int c = cok ? lane_col<VEC>(pbase + s * VEC, cend) : 0;
    const GOwn<VEC> o = gown<VEC>(ga, row, c);
    acc_t g0 = azero<VEC>(), z0 = g0, m0 = g0, l0 = g0, g1 = g0, z1 = g0, m1 = g0, l1 = g0;
    if (any1) {
      const size_t off = (size_t)max(d.y, 0) * ga.ld_in + c;
      g0 = Ln::load(ga.G + off);
      z0 = Ln::load(ga.Zf + off);
      m0 = Ln::load(ga.M + off);
      l0 = Ln::load(ga.L + off);
    }
    if (any2) {
      const size_t off = (size_t)max(d.w, 0) * ga.ld_in + c;
      g1 = Ln::load(ga.G + off);
      z1 = Ln::load(ga.Zf + off);
      m1 = Ln::load(ga.M + off);
      l1 = Ln::load(ga.L + off);
    }
    acc_t acc = azero<VEC>();
    if (d.y >= 0) gstep<VEC>(acc, o, g0, z0, m0, l0);
    if (d.w >= 0) gstep<VEC>(acc, o, g1, z1, m1, l1);
    if (cok && d.z >= 0) {
      const GDst t = d.x >= 0 ? task_dst(ga, d.x, -1) : task_dst(ga, 0, -(d.x + 1));
      if (t.z != nullptr) Ln::store(t.z + c, acc);
      else Ln::store_partial(t.p + c, acc);
    }
  }
}

// the 16 rows of a window from CSR, R = 64 / L at a time (dense-tile windows of the plan)
template <int L, int VEC>
__device__ __forceinline__ void gwindow_rows(const SGradArgs& ga, int window, int c0, int cend, int lane) {
  constexpr int R = 64 / L;
  const int g = lane / L;
  for (int rb = 0; rb < 16; rb += R) {
    const int r = window * 16 + rb + g;
    int e0 = 0, n = 0, row = -1;
    GDst o{nullptr, nullptr};
    if (rb + g < 16 && r < ga.p.N) {
      e0 = ga.rowptr[r];
      n = ga.rowptr[r + 1] - e0;
      row = r;
      o = task_dst(ga, r, -1);
    }
    gtask<L, VEC, false>(ga, row, o.z, o.p, e0, n, c0, cend, lane);
  }
}

// ------------------------------------------------------------------------------------------
// Planned kernel: the weighted planned kernel's decode (spmm_weighted_impl.h).  Tiny tasks always run in their region here, one per lane group.
// ------------------------------------------------------------------------------------------
template <int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void softmax_grad_plan_kernel(SGradArgs ga) {
  const PlanArgs& a = ga.p;
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
      const GDst o = task_dst(ga, t.x, t.w);
      gtask<L, VEC, true>(ga, t.x, o.z, o.p, __builtin_amdgcn_readfirstlane(t.y), __builtin_amdgcn_readfirstlane(t.z), c0, cend, lane);
    } else if (bf >= sparse_wgs_pp_ordinary_end(a)) {
      if (bf >= a.free_wgs_pp) return;
      constexpr int R = 64 / L;
      const int first = a.n_tasks - a.n_tiny + ((bf - sparse_wgs_pp_ordinary_end(a)) * kWaves + wave) * R;
      if (first >= a.n_tasks) return;
      gtiny<L, VEC>(ga, first, c0, cend, lane);
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
      int e0 = 0, n = 0, row = -1;
      GDst o{nullptr, nullptr};
      if (tp != nullptr) {
        const int4 t = *tp;
        if (t.x >= 0) {  // (slice padding: row -1)
          e0 = t.y;
          n = t.z;
          row = t.x;
          o = task_dst(ga, t.x, t.w);
        }
      }
      gtask<L, VEC, false>(ga, row, o.z, o.p, e0, n, c0, cend, lane);
    }
  } else {
    const int n_col_panels = (a.D + a.panel_cols - 1) / a.panel_cols;
    const int unit = ((int)blockIdx.x - a.sparse_wgs) * kWaves + wave;
    if (unit >= a.n_dense * n_col_panels) return;
    const int p = unit / a.n_dense, di = unit - p * a.n_dense;
    const int n_reg = a.n_dense - a.n_dense_compact - a.n_dense_compact2;
    int window;
    if (di < n_reg) window = ((cint_p)(a.plan + a.off_dense_index))[4 * di];
    else if (di < n_reg + a.n_dense_compact2) window = ((cint_p)(a.plan + a.off_dense_compact2))[(di - n_reg) * HCSPMM_COMPACT2_WORDS];
    else window = ((cint_p)(a.plan + a.off_dense_compact))[(di - n_reg - a.n_dense_compact2) * HCSPMM_COMPACT_WORDS];
    const int c0 = p * a.panel_cols;
    gwindow_rows<L, VEC>(ga, window, c0, min(a.D, c0 + a.panel_cols), lane);
  }
}

// Plan-free kernel: one workgroup per 16-row window, every window served from CSR: rows up to kPlanFreeWide entries by one
// lane group each, longer ones by whole waves (hybrid_window_w_kernel's sparse branch)
template <int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void softmax_grad_window_kernel(SGradArgs ga) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = (int)blockDim.x >> 6;
  const int r0 = (int)blockIdx.x * 16, r1 = min(r0 + 16, ga.p.N);
  constexpr int R = 64 / L;
  const int G = R * nwaves;
  const int gi = wave * R + lane / L;
  for (int rb = r0; rb < r1; rb += G) {
    const int r = rb + gi;
    int e0 = 0, n = 0, row = -1;
    GDst o{nullptr, nullptr};
    if (r < r1) {
      e0 = ga.rowptr[r];
      n = ga.rowptr[r + 1] - e0;
      if (R == 1 || n <= kPlanFreeWide) {
        row = r;
        o = task_dst(ga, r, -1);
      } else {
        n = 0;  // left to the whole-wave pass below
      }
    }
    gtask<L, VEC, false>(ga, row, o.z, o.p, e0, n, 0, ga.p.D, lane);
  }
  if (R > 1) {
    int k = 0;
    for (int r = r0; r < r1; ++r) {
      const int e0 = ga.rowptr[r];
      const int n = ga.rowptr[r + 1] - e0;
      if (n > kPlanFreeWide) {
        if (k % nwaves == wave) {
          const GDst o = task_dst(ga, r, -1);
          gtask<L, VEC, true>(ga, r, o.z, o.p, e0, n, 0, ga.p.D, lane);
        }
        ++k;
      }
    }
  }
}

constexpr int kGradMinWaves = 4;  // 128 registers per lane

template <int L, int VEC>
hipError_t launch_softmax_grad_LV(const SGradArgs& ga, hipStream_t stream) {
  SGradArgs gb = ga;
  PlanArgs& b = gb.p;
  if (ga.p.plan == nullptr) {  // plan-free
    const int W = (b.N + 15) / 16;
    int waves = (16 * L + 63) / 64;
    if (waves > kWaves) waves = kWaves;
    if (W > 0) hipLaunchKernelGGL((softmax_grad_window_kernel<L, VEC, kGradMinWaves>), dim3(W), dim3(waves * 64), 0, stream, gb);
    return hipGetLastError();
  }
  b.fused = 0;
  // the shared layout (plan_layout.h): no launch of their own for the tiny tasks (one per lane group), dense windows once per
  // column panel
  const int n_col_panels = plan_launch_layout(b, L, 0, 0, 1, false, 0);
  const long long dense_wgs = ((long long)b.n_dense * n_col_panels + kWaves - 1) / kWaves;
  const long long grid = (long long)b.sparse_wgs + dense_wgs;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (grid > 0)
    hipLaunchKernelGGL((softmax_grad_plan_kernel<L, VEC, kGradMinWaves>), dim3((unsigned)grid), dim3(kThreads), 0, stream, gb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || b.n_split_rows == 0) return e;
  const int fg = (b.n_split_rows + kWaves - 1) / kWaves;
  hipLaunchKernelGGL((fixup_kernel<F32, VEC>), dim3(fg), dim3(kThreads), 0, stream, b);  // fp32 sums: the binary pass
  return hipGetLastError();
}

}  // namespace

hipError_t launch_softmax_backward_f32(const SGradArgs& a, int vec, hipStream_t stream) {
  if (vec == 4) {
    switch (pick_L(a.p.plan != nullptr ? a.p.panel_cols : a.p.D, 4)) {
      case 4: return launch_softmax_grad_LV<4, 4>(a, stream);
      case 8: return launch_softmax_grad_LV<8, 4>(a, stream);
      case 16: return launch_softmax_grad_LV<16, 4>(a, stream);
      case 32: return launch_softmax_grad_LV<32, 4>(a, stream);
      default: return launch_softmax_grad_LV<64, 4>(a, stream);
    }
  }
  if (a.p.D > 4 * vec) return hipErrorInvalidValue;
  if (vec == 2) return launch_softmax_grad_LV<4, 2>(a, stream);
  return launch_softmax_grad_LV<4, 1>(a, stream);
}

}  // namespace hcspmm
