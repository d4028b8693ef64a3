// spmm_edge_messages.hip -- edge-feature messages (hcspmm_forward_edge_messages), fp32 on the binary
// product's plan: a neighbour's row combined with a feature VECTOR of the edge,
//   Z[r][d] = sum over the entries e of row r of m(X[col(e)][d], F[fi(e)][d]),  fi(e) = findex ? findex[e] : e
//   mul: fmaf(f, x, acc)    add_relu: acc + ((x + f) < 0 ? +0 : x + f)    copy: acc + f (X is not read)
//
// The schedule is the hybrid launch's (spmm_impl.h): sliced | wide | ordinary | tiny regions per column panel, then the
// dense-tile windows, then the fix-up pass over split rows.  Only the per-entry step differs.
//  * Every entry issues two 16-byte loads per lane, the X row through col[e] and the F row through fi(e), both through the
//    element-aligned lanes (Lane / lane_col), F in 64-bit addressing.  The lane that loads col[e] loads findex[e] behind it
//    (or takes e itself) and both travel to the gathering lanes through ds_bpermute; a lane past its task's end holds
//    fi = -1 and takes nothing.  HCSPMM_EDGE_U entries are in flight per lane (copy, one load per entry: HCSPMM_SPARSE_U).
//  * MFMA cannot take a per-column value: the rows of a dense-tile window are served from CSR by the sparse-row task body,
//    one lane group per row (spmm_extremum.hip does the same).
//  * Sums run in hcspmm_forward_weighted's order: CSR order on ordinary and tiny tasks, the wide tasks' xor-shuffle tree, fp32
//    partials of sliced and segmented rows added by the fix-up pass in fixup_kernel's order.  No atomics.
//  * Gradient with respect to X: this launch on A^T's graph with findex = entry_index_t (hcspmm.h).
#include "spmm_impl.h"

#include "hcspmm.h"

namespace hcspmm {
namespace {

#ifndef HCSPMM_EDGE_U
#define HCSPMM_EDGE_U 4  // entries in flight per lane for the two-load ops (eight 16-byte loads, the binary gather's count)
#endif

// tiny tasks per lane group: TinyT's, but two at L = 32 (four tasks hold sixteen loaded vectors per lane)
template <int L> struct ETinyT {
  static constexpr int value = L >= 32 ? 2 : TinyT<L>::value;
};

// one entry: VEC columns of the gathered X row and of the edge's F row
template <int OP, int VEC>
__device__ __forceinline__ void estep(typename AccT<VEC>::type& acc, const typename AccT<VEC>::type& x,
                                      const typename AccT<VEC>::type& f) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    if constexpr (OP == HCSPMM_EDGE_OP_MUL) {
      aset(acc, q, __builtin_fmaf(aget(f, q), aget(x, q), aget(acc, q)));
    } else if constexpr (OP == HCSPMM_EDGE_OP_ADD_RELU) {
      const float t = aget(x, q) + aget(f, q);
      aset(acc, q, aget(acc, q) + (t < 0.0f ? 0.0f : t));  // (written out: v_max_f32 drops a NaN in IEEE mode)
    } else {
      aset(acc, q, aget(acc, q) + aget(f, q));
    }
  }
}

// One branch-free batch of UB entries (spmm_impl.h gather_batch): lanes past a task's end hold fi -1, re-read row 0 and take
// nothing
template <int OP, int VEC, int UB>
__device__ __forceinline__ void ebatch(const EdgeMsgArgs& ea, int csafe, bool cok, int myidx, int myfi, int src0,
                                       typename AccT<VEC>::type& acc) {
  typedef Lane<F32, VEC> Ln;
  const float* X = reinterpret_cast<const float*>(ea.p.X);
  int idx[UB], fi[UB];
  typename AccT<VEC>::type x[UB], f[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    idx[u] = OP == HCSPMM_EDGE_OP_COPY ? 0 : __shfl(myidx, src0 + u, 64);
    fi[u] = __shfl(myfi, src0 + u, 64);
  }
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    if constexpr (OP != HCSPMM_EDGE_OP_COPY) x[u] = Ln::load(X + (size_t)max(idx[u], 0) * ea.p.ldx + csafe);
    else x[u] = azero<VEC>();
    f[u] = Ln::load(ea.F + (size_t)max(fi[u], 0) * ea.ldf + csafe);
  }
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && fi[u] >= 0) estep<OP, VEC>(acc, x[u], f[u]);
}

// sparse_task_w (spmm_weighted_impl.h) with the edge-message step: L lanes own the task = entries [e0, e0 + n); WIDE: the
// whole wave owns it and the 64/L lane-group sums are combined by the fixed xor-shuffle tree
template <int OP, int L, int VEC, bool WIDE>
__device__ __forceinline__ void etask(const EdgeMsgArgs& ea, float* dz, float* dp, int e0, int n, int c0, int cend, int lane) {
  typedef Lane<F32, VEC> Ln;
  constexpr int UMAX = OP == HCSPMM_EDGE_OP_COPY ? HCSPMM_SPARSE_U : HCSPMM_EDGE_U;
  constexpr int U = (L < UMAX) ? L : UMAX;
  constexpr int STRIDE = WIDE ? 64 : L;
  const int* __restrict__ col = ea.p.col;
  const int* __restrict__ findex = ea.findex;
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
    typename AccT<VEC>::type acc = azero<VEC>();
    int next = 0, nextf = -1;
    if (pos < n) {
      if (OP != HCSPMM_EDGE_OP_COPY) next = col[e0 + pos];
      nextf = findex != nullptr ? findex[e0 + pos] : e0 + pos;
    }
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next, myfi = nextf;
      const int en = e0 + base + STRIDE + pos;  // the next chunk's indices arrive under this chunk's gathers
      next = 0;
      nextf = -1;
      if (base + STRIDE + pos < n) {
        if (OP != HCSPMM_EDGE_OP_COPY) next = col[en];
        nextf = findex != nullptr ? findex[en] : en;
      }
      const int cnt = min(L, nmax - base);
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
        if (left > U / 2) {
          ebatch<OP, VEC, U>(ea, c, cok, myidx, myfi, gbase + j, acc);
          j += U;
        } else if (U >= 8 && left > U / 4) {
          ebatch<OP, VEC, (U >= 8 ? U / 2 : 1)>(ea, c, cok, myidx, myfi, gbase + j, acc);
          j += U / 2;
        } else if (U >= 4 && left > 1) {
          ebatch<OP, VEC, (U >= 8 ? U / 4 : 2)>(ea, c, cok, myidx, myfi, gbase + j, acc);
          j += (U >= 8 ? U / 4 : 2);
        } else {
          ebatch<OP, VEC, 1>(ea, c, cok, myidx, myfi, gbase + j, acc);
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
struct EDst {
  float* z;
  float* p;
};
__device__ __forceinline__ EDst task_dst(const EdgeMsgArgs& ea, int row, int slot) {
  const PlanArgs& a = ea.p;
  EDst d{nullptr, nullptr};
  if (slot < 0) d.z = reinterpret_cast<float*>(a.Z) + (size_t)row * a.ldz;
  else d.p = a.partial + (size_t)slot * (size_t)a.D;
  return d;
}

// first CSR entry of the split-row segment that owns partial slot s (spmm_weighted_impl.h segment_entry)
__device__ __forceinline__ int esegment_entry(const EdgeMsgArgs& ea, int s) {
  const int4* fix = reinterpret_cast<const int4*>(ea.p.plan + ea.p.off_fixups);
  int lo = 0, hi = ea.p.n_split_rows;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (fix[mid].y <= s) lo = mid;
    else hi = mid;
  }
  const int4 f = fix[lo];
  return ea.rowptr[f.x] + (s - f.y) * ea.segment_len;
}

// tiny_tasks_w (spmm_weighted_impl.h): T tasks of at most two entries per lane group, column ids inline in the descriptor;
// the entry position (the F row, or the place in findex) comes from rowptr (a whole row) or the fix-up list (the last
// segment of a split row)
template <int OP, int L, int VEC, int T>
__device__ __forceinline__ void etiny(const EdgeMsgArgs& ea, int first, int c0, int cend, int lane) {
  typedef Lane<F32, VEC> Ln;
  typedef typename AccT<VEC>::type acc_t;
  const PlanArgs& a = ea.p;
  const float* X = reinterpret_cast<const float*>(a.X);
  constexpr int R = 64 / L;
  const int g = lane / L, s = lane & (L - 1);
  const int4* tasks = reinterpret_cast<const int4*>(a.plan + a.off_tasks);
  int4 d[T];
  int f0[T], f1[T];
  bool any1 = false, any2 = false;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int tid = first + t * R + g;
    d[t] = (tid < a.n_tasks) ? tasks[tid] : int4{0, -1, -1, -1};
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    any1 |= d[t].y >= 0;
    any2 |= d[t].w >= 0;
  }
  any1 = __builtin_amdgcn_ballot_w64(any1) != 0;
  any2 = __builtin_amdgcn_ballot_w64(any2) != 0;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    int e = 0;
    if (d[t].y >= 0) e = d[t].x >= 0 ? ea.rowptr[d[t].x] : esegment_entry(ea, -(d[t].x + 1));
    f0[t] = f1[t] = 0;
    if (d[t].y >= 0) f0[t] = ea.findex != nullptr ? ea.findex[e] : e;
    if (d[t].w >= 0) f1[t] = ea.findex != nullptr ? ea.findex[e + 1] : e + 1;
  }
  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const bool cok = pbase + s * VEC < cend;
    const int c = cok ? lane_col<VEC>(pbase + s * VEC, cend) : 0;
    acc_t x0[T], x1[T], v0[T], v1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) x0[t] = x1[t] = v0[t] = v1[t] = azero<VEC>();
    if (any1) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if constexpr (OP != HCSPMM_EDGE_OP_COPY) x0[t] = Ln::load(X + (size_t)max(d[t].y, 0) * a.ldx + c);
        v0[t] = Ln::load(ea.F + (size_t)f0[t] * ea.ldf + c);
      }
    }
    if (any2) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if constexpr (OP != HCSPMM_EDGE_OP_COPY) x1[t] = Ln::load(X + (size_t)max(d[t].w, 0) * a.ldx + c);
        v1[t] = Ln::load(ea.F + (size_t)f1[t] * ea.ldf + c);
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      acc_t acc = azero<VEC>();
      if (d[t].y >= 0) estep<OP, VEC>(acc, x0[t], v0[t]);
      if (d[t].w >= 0) estep<OP, VEC>(acc, x1[t], v1[t]);
      if (cok && d[t].z >= 0) {
        const EDst o = d[t].x >= 0 ? task_dst(ea, d[t].x, -1) : task_dst(ea, 0, -(d[t].x + 1));
        if (o.z != nullptr) Ln::store(o.z + c, acc);
        else Ln::store_partial(o.p + c, acc);
      }
    }
  }
}

// the 16 rows of a window from CSR, R = 64 / L at a time (dense-tile windows of the plan)
template <int OP, int L, int VEC>
__device__ __forceinline__ void ewindow_rows(const EdgeMsgArgs& ea, int window, int c0, int cend, int lane) {
  constexpr int R = 64 / L;
  const int g = lane / L;
  for (int rb = 0; rb < 16; rb += R) {
    const int r = window * 16 + rb + g;
    int e0 = 0, n = 0;
    EDst o{nullptr, nullptr};
    if (rb + g < 16 && r < ea.p.N) {
      e0 = ea.rowptr[r];
      n = ea.rowptr[r + 1] - e0;
      o = task_dst(ea, r, -1);
    }
    etask<OP, L, VEC, false>(ea, o.z, o.p, e0, n, c0, cend, lane);
  }
}

// ------------------------------------------------------------------------------------------
// Planned kernel: hybrid_plan_kernel's regions (sliced | wide | ordinary | tiny per column panel), then one wave per
// (dense-tile window, column panel) serving the window's rows from CSR.  Tiny tasks always run in their region here.
// ------------------------------------------------------------------------------------------
template <int OP, int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void edge_messages_plan_kernel(EdgeMsgArgs ea) {
  const PlanArgs& a = ea.p;
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
      const EDst o = task_dst(ea, t.x, t.w);
      etask<OP, L, VEC, true>(ea, o.z, o.p, __builtin_amdgcn_readfirstlane(t.y), __builtin_amdgcn_readfirstlane(t.z), c0, cend, lane);
    } else if (bf >= sparse_wgs_pp_ordinary_end(a)) {
      if (bf >= a.free_wgs_pp) return;
      constexpr int R = 64 / L;
      const int first = a.n_tasks - a.n_tiny + ((bf - sparse_wgs_pp_ordinary_end(a)) * kWaves + wave) * (R * ETinyT<L>::value);
      if (first >= a.n_tasks) return;
      etiny<OP, L, VEC, ETinyT<L>::value>(ea, first, c0, cend, lane);
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
      EDst o{nullptr, nullptr};
      if (tp != nullptr) {
        const int4 t = *tp;
        if (t.x >= 0) {  // (slice padding: row -1)
          e0 = t.y;
          n = t.z;
          o = task_dst(ea, t.x, t.w);
        }
      }
      etask<OP, L, VEC, false>(ea, o.z, o.p, e0, n, c0, cend, lane);
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
    ewindow_rows<OP, L, VEC>(ea, window, c0, min(a.D, c0 + a.panel_cols), lane);
  }
}

// Fix-up: Z[row] of a split row = the sum of its fp32 partial rows, in fixup_kernel's order (spmm_impl.h): one wave per row,
// its 64/L lane groups taking every (64/L)-th slot, eight loads in flight, combined by the wide tasks' xor-shuffle tree
template <int VEC>
__global__ __launch_bounds__(kThreads) void edge_messages_fixup_kernel(PlanArgs a) {
  typedef typename AccT<VEC>::type acc_t;
  float* Z = reinterpret_cast<float*>(a.Z);
  const int lane = threadIdx.x & 63;
  const int fi = (int)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (fi >= a.n_split_rows) return;
  const int4 f = reinterpret_cast<const int4*>(a.plan + a.off_fixups)[fi];
  const int row = f.x, s0 = f.y, ns = f.z;
  const int slots = (a.D + VEC - 1) / VEC;
  int L = 1;
  while (L < slots && L < 64) L <<= 1;
  const int R = 64 / L, g = lane / L, sl = lane & (L - 1);
  for (int c0 = 0; c0 < a.D; c0 += L * VEC) {
    const bool cok = c0 + sl * VEC < a.D;
    const int c = cok ? lane_col<VEC>(c0 + sl * VEC, a.D) : 0;
    const float* p = a.partial + (size_t)s0 * (size_t)a.D + c;
    acc_t acc = azero<VEC>();
    int s = g;
    for (; s + 7 * R < ns; s += 8 * R) {
      acc_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = Lane<F32, VEC>::load_partial(p + (size_t)(s + u * R) * (size_t)a.D);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; s < ns; s += R) acc += Lane<F32, VEC>::load_partial(p + (size_t)s * (size_t)a.D);
    for (int off = L; off < 64; off <<= 1) {
#pragma unroll
      for (int q = 0; q < VEC; ++q) aset(acc, q, aget(acc, q) + __shfl_xor(aget(acc, q), off, 64));
    }
    if (cok && g == 0) Lane<F32, VEC>::store(Z + (size_t)row * a.ldz + c, acc);
  }
}

// Plan-free kernel: one workgroup per 16-row window, every window (dense-tile or not) served from CSR: rows up to
// kPlanFreeWide entries by one lane group each, longer ones by whole waves (hybrid_window_w_kernel's sparse branch)
template <int OP, int L, int VEC>
__global__ __launch_bounds__(kThreads) void edge_messages_window_kernel(EdgeMsgArgs ea) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = (int)blockDim.x >> 6;
  const int r0 = (int)blockIdx.x * 16, r1 = min(r0 + 16, ea.p.N);
  constexpr int R = 64 / L;
  const int G = R * nwaves;
  const int gi = wave * R + lane / L;
  for (int rb = r0; rb < r1; rb += G) {
    const int r = rb + gi;
    int e0 = 0, n = 0;
    EDst o{nullptr, nullptr};
    if (r < r1) {
      e0 = ea.rowptr[r];
      n = ea.rowptr[r + 1] - e0;
      if (R == 1 || n <= kPlanFreeWide) o = task_dst(ea, r, -1);
      else n = 0;  // left to the whole-wave pass below
    }
    etask<OP, L, VEC, false>(ea, o.z, o.p, e0, n, 0, ea.p.D, lane);
  }
  if (R > 1) {
    int k = 0;
    for (int r = r0; r < r1; ++r) {
      const int e0 = ea.rowptr[r];
      const int n = ea.rowptr[r + 1] - e0;
      if (n > kPlanFreeWide) {
        if (k % nwaves == wave) {
          const EDst o = task_dst(ea, r, -1);
          etask<OP, L, VEC, true>(ea, o.z, o.p, e0, n, 0, ea.p.D, lane);
        }
        ++k;
      }
    }
  }
}

template <int OP, int L, int VEC>
hipError_t launch_edge_messages_LV(const EdgeMsgArgs& ea, hipStream_t stream) {
  EdgeMsgArgs eb = ea;
  PlanArgs& b = eb.p;
  if (ea.p.plan == nullptr) {  // plan-free
    const int W = (b.N + 15) / 16;
    int waves = (16 * L + 63) / 64;
    if (waves > kWaves) waves = kWaves;
    if (W > 0) hipLaunchKernelGGL((edge_messages_window_kernel<OP, L, VEC>), dim3(W), dim3(waves * 64), 0, stream, eb);
    return hipGetLastError();
  }
  b.fused = 0;
  // the shared layout (plan_layout.h): no launch of their own for the tiny tasks, dense windows once per column panel
  const int n_col_panels = plan_launch_layout(b, L, 0, 0, ETinyT<L>::value, false, 0);
  const long long dense_wgs = ((long long)b.n_dense * n_col_panels + kWaves - 1) / kWaves;
  const long long grid = (long long)b.sparse_wgs + dense_wgs;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (grid > 0)
    hipLaunchKernelGGL((edge_messages_plan_kernel<OP, L, VEC, HCSPMM_MIN_WAVES_PER_SIMD>), dim3((unsigned)grid), dim3(kThreads), 0,
                       stream, eb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || b.n_split_rows == 0) return e;
  const int fg = (b.n_split_rows + kWaves - 1) / kWaves;
  hipLaunchKernelGGL((edge_messages_fixup_kernel<VEC>), dim3(fg), dim3(kThreads), 0, stream, b);
  return hipGetLastError();
}

template <int OP>
hipError_t launch_edge_messages_op(const EdgeMsgArgs& a, int vec, hipStream_t stream) {
  if (vec == 4) {
    switch (pick_L(a.p.plan != nullptr ? a.p.panel_cols : a.p.D, 4)) {
      case 4: return launch_edge_messages_LV<OP, 4, 4>(a, stream);
      case 8: return launch_edge_messages_LV<OP, 8, 4>(a, stream);
      case 16: return launch_edge_messages_LV<OP, 16, 4>(a, stream);
      case 32: return launch_edge_messages_LV<OP, 32, 4>(a, stream);
      default: return launch_edge_messages_LV<OP, 64, 4>(a, stream);
    }
  }
  if (a.p.D > 4 * vec) return hipErrorInvalidValue;
  if (vec == 2) return launch_edge_messages_LV<OP, 4, 2>(a, stream);
  return launch_edge_messages_LV<OP, 4, 1>(a, stream);
}

}  // namespace

hipError_t launch_edge_messages_f32(const EdgeMsgArgs& a, int vec, hipStream_t stream) {
  switch (a.op) {
    case HCSPMM_EDGE_OP_MUL: return launch_edge_messages_op<HCSPMM_EDGE_OP_MUL>(a, vec, stream);
    case HCSPMM_EDGE_OP_ADD_RELU: return launch_edge_messages_op<HCSPMM_EDGE_OP_ADD_RELU>(a, vec, stream);
    case HCSPMM_EDGE_OP_COPY: return launch_edge_messages_op<HCSPMM_EDGE_OP_COPY>(a, vec, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace hcspmm
