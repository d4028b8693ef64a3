// spmm_extremum.hip -- max / min neighbour aggregation with its argmax, and the backward of it (hcspmm_forward_extremum*,
// DESIGN.md section 3.12), fp32 on the binary product's plan:
//   forward   Z[r][d] = max (min) over the entries e of row r of X[col(e)][d],  arg[r][d] = the winning e
//   backward  grad_X[j][d] = sum of grad_Z[i][d] over the entries e = (i, j) with arg[i][d] == e
//
// The schedule is the hybrid launch's (spmm_impl.h): sliced | wide | ordinary | tiny regions per column panel, then the
// dense-tile windows, then a fix-up pass over split rows.  Only the reduction differs.
//  * The winner is a (value, position) pair under one strict order: NaN above every number, then the larger value, ties
//    (-0 == +0, NaN against NaN) to the lower position.  The order is total on distinct positions, so every combine --
//    a lane's CSR scan, the wide tasks' shuffle tree, the fix-up over slices and segments -- gives the bits of a
//    sequential scan, whatever the split.  The compares are written out: v_max_f32 drops a NaN in IEEE mode.
//  * min is max over the negated values: the sign bit of every loaded element is flipped, and flipped back on the way
//    out, so the output is the winning entry's own bits (a NaN's payload, the sign of a zero included).
//  * MFMA cannot take a maximum: the rows of a dense-tile window are served from CSR by the sparse-row task body, one
//    lane group per row.
//  * Split rows: the forward's partial slots hold (value, position) pairs -- the values in the fp32 workspace, the
//    positions behind them (hcspmm_extremum_workspace_bytes) -- combined by their own fix-up kernel below.
//  * Backward: A^T of a pattern-symmetric graph is A's pattern, so row j's entry e_t gathers grad_Z[col(e_t)] and
//    arg[col(e_t)] and adds the columns whose arg is perm[e_t].  Sums run in the plan's fixed order (CSR order, the wide
//    shuffle tree, the binary fix-up pass over the fp32 workspace): deterministic, no atomics.
#include "extremum_common.h"  // the (value, position) order, kNone, XTinyT, the int32 lane vectors

namespace hcspmm {
namespace {

// per-lane state of VEC columns: forward = best (flipped) value and its entry; backward = the sums (bp unused)
template <int VEC, bool BWD> struct XState {
  float bv[VEC];
  int bp[VEC];
  __device__ __forceinline__ XState() {
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      bv[q] = BWD ? 0.0f : -__builtin_inff();
      bp[q] = kNone;
    }
  }
  __device__ __forceinline__ void take(float v, int p, int q) {
    if (xbeats(v, p, bv[q], bp[q])) {
      bv[q] = v;
      bp[q] = p;
    }
  }
};

// forward result of a whole row: the winner's own bits and entry; +0 and -1 for a row without entries
template <int VEC>
__device__ __forceinline__ void xstore_row(float* z, int* arg, const XState<VEC, false>& st, unsigned flip) {
  typename AccT<VEC>::type out;
  typename IntV<VEC>::type pos;
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    const bool none = st.bp[q] == kNone;
    aset(out, q, none ? 0.0f : xflip(st.bv[q], flip));
    iset(pos, q, none ? -1 : st.bp[q]);
  }
  Lane<F32, VEC>::store(z, out);
  if (arg != nullptr) istore<VEC>(arg, pos);
}

template <int VEC, bool BWD>
__device__ __forceinline__ void xstore_partial(float* p, int* pp, const XState<VEC, BWD>& st) {
  typename AccT<VEC>::type out;
  typename IntV<VEC>::type pos;
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    aset(out, q, st.bv[q]);
    iset(pos, q, st.bp[q]);
  }
  Lane<F32, VEC>::store_partial(p, out);
  if (!BWD) istore<VEC>(pp, pos);
}

template <int VEC, bool BWD>
__device__ __forceinline__ void xstore(const XArgs& xa, float* dz, int* da, float* dp, int* dpp, int c, const XState<VEC, BWD>& st) {
  if (dz != nullptr) {
    if constexpr (BWD) {
      typename AccT<VEC>::type out;
#pragma unroll
      for (int q = 0; q < VEC; ++q) aset(out, q, st.bv[q]);
      Lane<F32, VEC>::store(dz + c, out);
    } else {
      xstore_row<VEC>(dz + c, da != nullptr ? da + c : nullptr, st, xa.flip);
    }
  } else if (dp != nullptr) {
    xstore_partial<VEC, BWD>(dp + c, BWD ? nullptr : dpp + c, st);
  }
}

// one gathered row (VEC columns at entry e): forward takes the pair, backward adds the columns whose argmax is `pe`
template <int VEC, bool BWD>
__device__ __forceinline__ void xstep(XState<VEC, BWD>& st, const typename AccT<VEC>::type& v, const typename IntV<VEC>::type& ar,
                                      int e, int pe, unsigned flip) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    if constexpr (BWD) st.bv[q] = iget(ar, q) == pe ? st.bv[q] + aget(v, q) : st.bv[q];
    else st.take(xflip(aget(v, q), flip), e, q);
  }
}

// One branch-free batch of UB row gathers (spmm_impl.h gather_batch): lanes past a task's end hold idx -1 and take nothing
template <int VEC, int UB, bool BWD>
__device__ __forceinline__ void xbatch(const XArgs& xa, int csafe, bool cok, int myidx, int myperm, int src0, int ebase,
                                       XState<VEC, BWD>& st) {
  typedef Lane<F32, VEC> Ln;
  const float* X = reinterpret_cast<const float*>(xa.p.X);
  int idx[UB], pe[UB];
  typename Ln::raw_t v[UB];
  typename IntV<VEC>::type ar[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    idx[u] = __shfl(myidx, src0 + u, 64);
    pe[u] = BWD ? __shfl(myperm, src0 + u, 64) : 0;
  }
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    v[u] = Ln::load(X + (size_t)max(idx[u], 0) * xa.p.ldx + csafe);
    if constexpr (BWD) ar[u] = iload<VEC>(xa.garg + (size_t)max(idx[u], 0) * xa.ldarg + csafe);
    else ar[u] = typename IntV<VEC>::type{};
  }
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && idx[u] >= 0) xstep<VEC, BWD>(st, v[u], ar[u], ebase + u, pe[u], xa.flip);
}

// sparse_task (spmm_impl.h) with the extremum reduction: L lanes own the task = entries [e0, e0 + n); WIDE: the whole wave
// owns it and the 64/L lane-group results are combined by the fixed xor-shuffle tree
template <int L, int VEC, bool WIDE, bool BWD>
__device__ __forceinline__ void xtask(const XArgs& xa, float* dz, int* da, float* dp, int* dpp, int e0, int n, int c0, int cend,
                                      int lane) {
  constexpr int UMAX = BWD ? HCSPMM_SPARSE_U / 2 : HCSPMM_SPARSE_U;  // (backward: two loads per entry)
  constexpr int U = (L < UMAX) ? L : UMAX;
  constexpr int STRIDE = WIDE ? 64 : L;
  const int* __restrict__ col = xa.p.col;
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
    XState<VEC, BWD> st;
    int next = pos < n ? col[e0 + pos] : -1;
    int nextp = (BWD && pos < n) ? xa.perm[e0 + pos] : 0;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next, myperm = nextp;
      const bool more = base + STRIDE + pos < n;
      next = more ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      if (BWD) nextp = more ? xa.perm[e0 + base + STRIDE + pos] : 0;
      const int cnt = min(L, nmax - base);
      const int ebase = e0 + base + (WIDE ? gbase : 0);
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
        if (left > U / 2) {
          xbatch<VEC, U, BWD>(xa, c, cok, myidx, myperm, gbase + j, ebase + j, st);
          j += U;
        } else if (U >= 8 && left > U / 4) {
          xbatch<VEC, (U >= 8 ? U / 2 : 1), BWD>(xa, c, cok, myidx, myperm, gbase + j, ebase + j, st);
          j += U / 2;
        } else if (U >= 4 && left > 1) {
          xbatch<VEC, (U >= 8 ? U / 4 : 2), BWD>(xa, c, cok, myidx, myperm, gbase + j, ebase + j, st);
          j += (U >= 8 ? U / 4 : 2);
        } else {
          xbatch<VEC, 1, BWD>(xa, c, cok, myidx, myperm, gbase + j, ebase + j, st);
          j += 1;
        }
      }
    }
    if (WIDE) {
#pragma unroll
      for (int off = L; off < 64; off <<= 1) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float ov = __shfl_xor(st.bv[q], off, 64);
          if constexpr (BWD) {
            st.bv[q] += ov;
          } else {
            st.take(ov, __shfl_xor(st.bp[q], off, 64), q);
          }
        }
      }
    }
    if (cok && (!WIDE || lane < L)) xstore<VEC, BWD>(xa, dz, da, dp, dpp, c, st);
  }
}

// destinations of a task descriptor (row | first entry | length | partial slot or -1)
struct XDst {
  float* z;
  int* a;
  float* p;
  int* pp;
};
__device__ __forceinline__ XDst task_dst(const XArgs& xa, int row, int slot) {
  const PlanArgs& a = xa.p;
  XDst d{nullptr, nullptr, nullptr, nullptr};
  if (slot < 0) {
    d.z = reinterpret_cast<float*>(a.Z) + (size_t)row * a.ldz;
    if (xa.arg != nullptr) d.a = xa.arg + (size_t)row * xa.ldarg;
  } else {
    d.p = a.partial + (size_t)slot * (size_t)a.D;
    if (xa.ppos != nullptr) d.pp = xa.ppos + (size_t)slot * (size_t)a.D;
  }
  return d;
}

// first CSR entry of the split-row segment that owns partial slot s (spmm_weighted_impl.h segment_entry)
__device__ __forceinline__ int xsegment_entry(const XArgs& xa, int s) {
  const int4* fix = reinterpret_cast<const int4*>(xa.p.plan + xa.p.off_fixups);
  int lo = 0, hi = xa.p.n_split_rows;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (fix[mid].y <= s) lo = mid;
    else hi = mid;
  }
  const int4 f = fix[lo];
  return xa.rowptr[f.x] + (s - f.y) * xa.segment_len;
}

// tiny_tasks (spmm_impl.h): T tasks of at most two entries per lane group, indices inline in the descriptor; the entry
// position comes from rowptr (a whole row) or the fix-up list (the last segment of a split row)
template <int L, int VEC, int T, bool BWD>
__device__ __forceinline__ void xtiny(const XArgs& xa, int first, int c0, int cend, int lane) {
  typedef Lane<F32, VEC> Ln;
  const PlanArgs& a = xa.p;
  const float* X = reinterpret_cast<const float*>(a.X);
  constexpr int R = 64 / L;
  const int g = lane / L, s = lane & (L - 1);
  const int4* tasks = reinterpret_cast<const int4*>(a.plan + a.off_tasks);
  int4 d[T];
  int e[T], p0[T], p1[T];
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
    e[t] = 0;
    if (d[t].y >= 0) e[t] = d[t].x >= 0 ? xa.rowptr[d[t].x] : xsegment_entry(xa, -(d[t].x + 1));
    p0[t] = (BWD && d[t].y >= 0) ? xa.perm[e[t]] : 0;
    p1[t] = (BWD && d[t].w >= 0) ? xa.perm[e[t] + 1] : 0;
  }
  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const bool cok = pbase + s * VEC < cend;
    const int c = cok ? lane_col<VEC>(pbase + s * VEC, cend) : 0;
    typename Ln::raw_t v0[T], v1[T];
    typename IntV<VEC>::type a0[T], a1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      v0[t] = v1[t] = Ln::zero();
      a0[t] = a1[t] = typename IntV<VEC>::type{};
    }
    if (any1) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        v0[t] = Ln::load(X + (size_t)max(d[t].y, 0) * a.ldx + c);
        if (BWD) a0[t] = iload<VEC>(xa.garg + (size_t)max(d[t].y, 0) * xa.ldarg + c);
      }
    }
    if (any2) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        v1[t] = Ln::load(X + (size_t)max(d[t].w, 0) * a.ldx + c);
        if (BWD) a1[t] = iload<VEC>(xa.garg + (size_t)max(d[t].w, 0) * xa.ldarg + c);
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      XState<VEC, BWD> st;
      if (d[t].y >= 0) xstep<VEC, BWD>(st, v0[t], a0[t], e[t], p0[t], xa.flip);
      if (d[t].w >= 0) xstep<VEC, BWD>(st, v1[t], a1[t], e[t] + 1, p1[t], xa.flip);
      if (cok && d[t].z >= 0) {
        const XDst o = d[t].x >= 0 ? task_dst(xa, d[t].x, -1) : task_dst(xa, 0, -(d[t].x + 1));
        xstore<VEC, BWD>(xa, o.z, o.a, o.p, o.pp, c, st);
      }
    }
  }
}

// the 16 rows of a window from CSR, R = 64 / L at a time (dense-tile windows of the plan; every window plan-free)
template <int L, int VEC, bool BWD>
__device__ __forceinline__ void xwindow_rows(const XArgs& xa, int window, int c0, int cend, int lane) {
  constexpr int R = 64 / L;
  const int g = lane / L;
  for (int rb = 0; rb < 16; rb += R) {
    const int r = window * 16 + rb + g;
    int e0 = 0, n = 0;
    XDst o{nullptr, nullptr, nullptr, nullptr};
    if (rb + g < 16 && r < xa.p.N) {
      e0 = xa.rowptr[r];
      n = xa.rowptr[r + 1] - e0;
      o = task_dst(xa, r, -1);
    }
    xtask<L, VEC, false, BWD>(xa, o.z, o.a, o.p, o.pp, e0, n, c0, cend, lane);
  }
}

// ------------------------------------------------------------------------------------------
// Planned kernel: hybrid_plan_kernel's regions (sliced | wide | ordinary | tiny per column panel), then one wave per
// (dense-tile window, column panel) serving the window's rows from CSR.  Tiny tasks always run in their region here.
// ------------------------------------------------------------------------------------------
template <int L, int VEC, bool BWD, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void extremum_plan_kernel(XArgs xa) {
  const PlanArgs& a = xa.p;
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
      const XDst o = task_dst(xa, t.x, t.w);
      xtask<L, VEC, true, BWD>(xa, o.z, o.a, o.p, o.pp, __builtin_amdgcn_readfirstlane(t.y), __builtin_amdgcn_readfirstlane(t.z),
                               c0, cend, lane);
    } else if (bf >= sparse_wgs_pp_ordinary_end(a)) {
      if (bf >= a.free_wgs_pp) return;
      constexpr int R = 64 / L;
      const int first = a.n_tasks - a.n_tiny + ((bf - sparse_wgs_pp_ordinary_end(a)) * kWaves + wave) * (R * XTinyT<L>::value);
      if (first >= a.n_tasks) return;
      xtiny<L, VEC, XTinyT<L>::value, BWD>(xa, first, c0, cend, lane);
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
      XDst o{nullptr, nullptr, nullptr, nullptr};
      if (tp != nullptr) {
        const int4 t = *tp;
        if (t.x >= 0) {  // (slice padding: row -1)
          e0 = t.y;
          n = t.z;
          o = task_dst(xa, t.x, t.w);
        }
      }
      xtask<L, VEC, false, BWD>(xa, o.z, o.a, o.p, o.pp, e0, n, c0, cend, lane);
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
    xwindow_rows<L, VEC, BWD>(xa, window, c0, min(a.D, c0 + a.panel_cols), lane);
  }
}

// Forward fix-up: Z[row] and arg[row] of a split row = the best of its partial (value, position) pairs -- one wave per row,
// the 64/L lane groups taking every (64/L)-th slot and combined by the xor-shuffle tree (fixup_kernel's shape)
template <int VEC>
__global__ __launch_bounds__(kThreads) void extremum_fixup_kernel(XArgs xa) {
  const PlanArgs& a = xa.p;
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
    const size_t at = (size_t)s0 * (size_t)a.D + c;
    XState<VEC, false> st;
    int s = g;
    for (; s + 3 * R < ns; s += 4 * R) {  // four slots in flight per lane
      typename AccT<VEC>::type v[4];
      typename IntV<VEC>::type pp[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = Lane<F32, VEC>::load_partial(a.partial + at + (size_t)(s + u * R) * (size_t)a.D);
        pp[u] = iload<VEC>(xa.ppos + at + (size_t)(s + u * R) * (size_t)a.D);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) st.take(aget(v[u], q), iget(pp[u], q), q);
      }
    }
    for (; s < ns; s += R) {
      const typename AccT<VEC>::type v = Lane<F32, VEC>::load_partial(a.partial + at + (size_t)s * (size_t)a.D);
      const typename IntV<VEC>::type pp = iload<VEC>(xa.ppos + at + (size_t)s * (size_t)a.D);
#pragma unroll
      for (int q = 0; q < VEC; ++q) st.take(aget(v, q), iget(pp, q), q);
    }
    for (int off = L; off < 64; off <<= 1) {
#pragma unroll
      for (int q = 0; q < VEC; ++q) st.take(__shfl_xor(st.bv[q], off, 64), __shfl_xor(st.bp[q], off, 64), q);
    }
    if (cok && g == 0) {
      const XDst o = task_dst(xa, row, -1);
      xstore<VEC, false>(xa, o.z, o.a, nullptr, nullptr, c, st);
    }
  }
}

// Plan-free kernel: one workgroup per 16-row window, every window (dense-tile or not) served from CSR: rows up to
// kPlanFreeWide entries by one lane group each, longer ones by whole waves (hybrid_window_kernel's sparse branch)
template <int L, int VEC, bool BWD>
__global__ __launch_bounds__(kThreads) void extremum_window_kernel(XArgs xa) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = (int)blockDim.x >> 6;
  const int r0 = (int)blockIdx.x * 16, r1 = min(r0 + 16, xa.p.N);
  constexpr int R = 64 / L;
  const int G = R * nwaves;
  const int gi = wave * R + lane / L;
  for (int rb = r0; rb < r1; rb += G) {
    const int r = rb + gi;
    int e0 = 0, n = 0;
    XDst o{nullptr, nullptr, nullptr, nullptr};
    if (r < r1) {
      e0 = xa.rowptr[r];
      n = xa.rowptr[r + 1] - e0;
      if (R == 1 || n <= kPlanFreeWide) o = task_dst(xa, r, -1);
      else n = 0;  // left to the whole-wave pass below
    }
    xtask<L, VEC, false, BWD>(xa, o.z, o.a, o.p, o.pp, e0, n, 0, xa.p.D, lane);
  }
  if (R > 1) {
    int k = 0;
    for (int r = r0; r < r1; ++r) {
      const int e0 = xa.rowptr[r];
      const int n = xa.rowptr[r + 1] - e0;
      if (n > kPlanFreeWide) {
        if (k % nwaves == wave) {
          const XDst o = task_dst(xa, r, -1);
          xtask<L, VEC, true, BWD>(xa, o.z, o.a, o.p, o.pp, e0, n, 0, xa.p.D, lane);
        }
        ++k;
      }
    }
  }
}

template <int L, int VEC, bool BWD>
hipError_t launch_extremum_LV(const XArgs& xa, hipStream_t stream) {
  XArgs xb = xa;
  PlanArgs& b = xb.p;
  if (xa.p.plan == nullptr) {  // plan-free
    const int W = (b.N + 15) / 16;
    int waves = (16 * L + 63) / 64;
    if (waves > kWaves) waves = kWaves;
    if (W > 0) hipLaunchKernelGGL((extremum_window_kernel<L, VEC, BWD>), dim3(W), dim3(waves * 64), 0, stream, xb);
    return hipGetLastError();
  }
  b.fused = 0;
  // the shared layout (plan_layout.h): no launch of their own for the tiny tasks, dense windows once per column panel
  const int n_col_panels = plan_launch_layout(b, L, 0, 0, XTinyT<L>::value, false, 0);
  const long long dense_wgs = ((long long)b.n_dense * n_col_panels + kWaves - 1) / kWaves;
  const long long grid = (long long)b.sparse_wgs + dense_wgs;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (grid > 0)
    hipLaunchKernelGGL((extremum_plan_kernel<L, VEC, BWD, HCSPMM_MIN_WAVES_PER_SIMD>), dim3((unsigned)grid), dim3(kThreads), 0,
                       stream, xb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || b.n_split_rows == 0) return e;
  const int fg = (b.n_split_rows + kWaves - 1) / kWaves;
  if (BWD) hipLaunchKernelGGL((fixup_kernel<F32, VEC>), dim3(fg), dim3(kThreads), 0, stream, b);  // fp32 sums: the binary pass
  else hipLaunchKernelGGL((extremum_fixup_kernel<VEC>), dim3(fg), dim3(kThreads), 0, stream, xb);
  return hipGetLastError();
}

template <bool BWD>
hipError_t launch_extremum_any(const XArgs& a, int vec, hipStream_t stream) {
  if (vec == 4) {
    switch (pick_L(a.p.plan != nullptr ? a.p.panel_cols : a.p.D, 4)) {
      case 4: return launch_extremum_LV<4, 4, BWD>(a, stream);
      case 8: return launch_extremum_LV<8, 4, BWD>(a, stream);
      case 16: return launch_extremum_LV<16, 4, BWD>(a, stream);
      case 32: return launch_extremum_LV<32, 4, BWD>(a, stream);
      default: return launch_extremum_LV<64, 4, BWD>(a, stream);
    }
  }
  if (a.p.D > 4 * vec) return hipErrorInvalidValue;
  if (vec == 2) return launch_extremum_LV<4, 2, BWD>(a, stream);
  return launch_extremum_LV<4, 1, BWD>(a, stream);
}

}  // namespace

hipError_t launch_extremum_f32(const XArgs& a, int vec, hipStream_t stream) { return launch_extremum_any<false>(a, vec, stream); }
hipError_t launch_extremum_backward_f32(const XArgs& a, int vec, hipStream_t stream) {
  return launch_extremum_any<true>(a, vec, stream);
}

}  // namespace hcspmm
