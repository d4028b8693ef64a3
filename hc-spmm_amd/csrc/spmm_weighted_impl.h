// spmm_weighted_impl.h -- gfx950 device code of the edge-weighted hybrid SpMM  Z = A_w * X  (hcspmm_forward_weighted),
// templated on the feature element type like spmm_impl.h, whose building blocks (lane vectors, compact records, stores,
// dispatch) it reuses.  Included by spmm_weighted.hip (fp32) and spmm_weighted_h16.hip (fp16 / bf16).
//
// The kernels are the binary ones' shapes with one more operand per entry: values[e], aligned with column_index.  Every
// step is acc = fmaf(v, x, acc), in the order the binary kernel adds that row (CSR order on ordinary and tiny tasks,
// ascending window columns on the dense-tile path, the same shuffle tree on wide tasks, the same fix-up order for split
// rows), so values == 1 reproduces hcspmm_forward_typed bit for bit.  The binary kernels and the plan are untouched: the
// weighted launch finds each entry's position as follows.
//  * ordinary, wide and sliced tasks: descriptors carry their first entry e0; lane i of a chunk loads values[e0 + i] in the
//    same coalesced load as col[e0 + i], and both travel to the gathering lanes through ds_bpermute.
//  * tiny tasks: the descriptor holds the row (entry rowptr[row]) or the partial slot of a split row's last segment
//    (entry from the fix-up list: rowptr[row] + segment index * segment_len).
//  * dense-tile windows: lane l supplies A[row l & 15][k-step column l >> 4].  Columns are unique and ascending within a
//    row, so the j-th set bit of row i over the window's ascending columns is CSR entry rowptr[w*16 + i] + j: each lane
//    keeps a running popcount of its row's bits over the k-steps and loads values[entry] in the batch of its X gathers.
//    The A operand is that value instead of 1.0; v_mfma_f32_16x16x4_f32 stays a k-ordered fma chain.
//
// 8-bit features (spmm_weighted_f8.hip, hcspmm_forward_fp8): the same kernels with the entry weight read through
// entry_weight() -- values[e] times the fp32 scale of the gathered row, row_scale[col[e]], either of which may be absent.  The lane
// that loads col[e] loads the scale behind it (one dependent 4-byte gather) and multiplies before the broadcast, so the
// gathering lanes see one weight per entry, as in the fp32 / 16-bit builds.
#pragma once
#include "csr_schedule.h"  // segment_entry: a partial slot's first CSR entry

namespace hcspmm {

// Weight of a CSR entry whose column is c (c >= 0), read through a cursor `p` that stands at the entry: p + k is the cursor k
// entries on.  Plain values (the fp32 / 16-bit builds): the cursor is a pointer into values.
__device__ __forceinline__ float entry_weight(const float* p, int) { return *p; }
// The 8-bit build: w = values[e] * row_scale[c], one fp32 multiplication; a missing operand is 1.
struct ScaledCursor {
  const float* values;     // at the entry, or null
  const float* row_scale;  // [x_rows], or null
  __device__ __forceinline__ ScaledCursor operator+(int k) const { return ScaledCursor{values != nullptr ? values + k : nullptr, row_scale}; }
};
__device__ __forceinline__ float entry_weight(const ScaledCursor& p, int c) {
  float w = p.values != nullptr ? *p.values : 1.0f;
  if (p.row_scale != nullptr) w *= p.row_scale[c];
  return w;
}
// a cursor as a function parameter: the plain pointer keeps its __restrict__ (W is then named at the call, not deduced)
template <typename W> struct WParam { typedef W type; };
template <> struct WParam<const float*> { typedef const float* __restrict__ type; };
__device__ __forceinline__ const float* row_scale_of(const WPlanArgs& wa) { return wa.p.row_scale; }
__device__ __forceinline__ const float* row_scale_of(const WWindowArgs& wa) { return wa.row_scale; }
// the cursor at entry 0 of a launch (WA: WPlanArgs / WWindowArgs)
template <typename E, typename WA> __device__ __forceinline__ auto weights_of(const WA& wa) {
  if constexpr (sizeof(typename E::T) == 1) return ScaledCursor{wa.values, row_scale_of(wa)};
  else return wa.values;
}

// acc[q] = fmaf(w, x[q], acc[q]) for the VEC (widened) elements of one loaded vector
template <typename E, int VEC>
__device__ __forceinline__ void wfma(typename AccT<VEC>::type& acc, float w, const typename RawT<E, VEC>::type& v) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) aset(acc, q, __builtin_fmaf(w, Lane<E, VEC>::elem(v, q), aget(acc, q)));
}

// gather_batch with the entry values broadcast alongside the column indices (lanes past a task's end hold idx -1 and
// value 0: fmaf(0, 0, acc) adds +0 exactly as the binary batch does)
template <typename E, int VEC, int UB, typename W>
__device__ __forceinline__ void gather_batch_w(const typename E::T* __restrict__ X, size_t ldx, int csafe, bool cok, int myidx,
                                               float myval, int src0, typename AccT<VEC>::type& acc, const int* pf_col,
                                               W pf_val, int& next, float& nextv) {
  typedef Lane<E, VEC> Ln;
  int idx[UB];
  float w[UB];
  typename Ln::raw_t v[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    idx[u] = __shfl(myidx, src0 + u, 64);
    w[u] = __shfl(myval, src0 + u, 64);
  }
  if (pf_col != nullptr) {
    next = *pf_col;
    nextv = entry_weight(pf_val, next);
  }
#pragma unroll
  for (int u = 0; u < UB; ++u) v[u] = Ln::load(X + (size_t)max(idx[u], 0) * ldx + csafe);
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    if (!(cok && idx[u] >= 0)) v[u] = Ln::zero();
    wfma<E, VEC>(acc, w[u], v[u]);
  }
}

// tiny tasks per lane group in the hybrid launch's tiny region: TinyT (spmm_impl.h), except that the 8-bit build -- values, scales
// and the fp32 sums of 8 columns per lane -- keeps at most two in flight (four spill 20 bytes at L = 32)
template <typename E, int L> struct TinyWT {
  static constexpr int value = (sizeof(typename E::T) == 1 && TinyT<L>::value > 2) ? 2 : TinyT<L>::value;
};

// sparse_task (spmm_impl.h) with weights: the same chunking, batches and combine tree
template <typename E, int L, int VEC, bool WIDE, int UMAX = HCSPMM_SPARSE_U, typename W = const float*>
__device__ __forceinline__ void sparse_task_w(const typename E::T* __restrict__ X, typename E::Z* __restrict__ dstZ,
                                              float* __restrict__ dstP, const int* __restrict__ col, W vals, int e0,
                                              int n, size_t ldx, int c0, int cend, int lane) {
  typedef Lane<E, VEC> Ln;
  typedef typename Ln::acc_t acc_t;
  constexpr int U = (L < UMAX) ? L : UMAX;
  constexpr int STRIDE = WIDE ? 64 : L;
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
    const int csafe = c;
    acc_t acc = azero<VEC>();
    int next = -1;
    float nextv = 0.f;
    if (pos < n) {
      next = col[e0 + pos];
      nextv = entry_weight(vals + (e0 + pos), next);
    }
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      const float myval = nextv;
      const bool more = base + STRIDE + pos < n;
      next = -1;
      nextv = 0.f;
      const int cnt = min(L, nmax - base);
      const int* pf = more ? col + e0 + base + STRIDE + pos : nullptr;
      const W pfv = vals + e0 + base + STRIDE + pos;  // read only when pf is set
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
        if (left > U / 2) {
          gather_batch_w<E, VEC, U>(X, ldx, csafe, cok, myidx, myval, gbase + j, acc, pf, pfv, next, nextv);
          j += U;
        } else if (U >= 8 && left > U / 4) {
          gather_batch_w<E, VEC, (U >= 8 ? U / 2 : 1)>(X, ldx, csafe, cok, myidx, myval, gbase + j, acc, pf, pfv, next, nextv);
          j += U / 2;
        } else if (U >= 4 && left > 1) {
          gather_batch_w<E, VEC, (U >= 8 ? U / 4 : 2)>(X, ldx, csafe, cok, myidx, myval, gbase + j, acc, pf, pfv, next, nextv);
          j += (U >= 8 ? U / 4 : 2);
        } else {
          gather_batch_w<E, VEC, 1>(X, ldx, csafe, cok, myidx, myval, gbase + j, acc, pf, pfv, next, nextv);
          j += 1;
        }
        pf = nullptr;
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
      if (dstZ != nullptr) Ln::store(dstZ + c, acc);
      else if (dstP != nullptr) Ln::store_partial(dstP + c, acc);
    }
  }
}

// tiny_tasks (spmm_impl.h) with weights: the entry position comes from rowptr (a whole row) or the fix-up list (the last
// segment of a split row); the value loads follow it, next to the row gathers
template <typename E, int L, int VEC, int T>
__device__ __forceinline__ void tiny_tasks_w(const WPlanArgs& wa, int first, int c0, int cend, int lane) {
  typedef Lane<E, VEC> Ln;
  typedef typename E::T elem_t;
  const PlanArgs& a = wa.p;
  const elem_t* X = reinterpret_cast<const elem_t*>(a.X);
  typename E::Z* Z = reinterpret_cast<typename E::Z*>(a.Z);
  constexpr int R = 64 / L;
  const int g = lane / L, s = lane & (L - 1);
  const int4* tasks = reinterpret_cast<const int4*>(a.plan + a.off_tasks);
  int4 d[T];
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
  float w0[T], w1[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    int e = 0;
    if (d[t].y >= 0) e = d[t].x >= 0 ? wa.rowptr[d[t].x] : segment_entry(a, wa.rowptr, wa.segment_len, -(d[t].x + 1));
    w0[t] = d[t].y >= 0 ? entry_weight(weights_of<E>(wa) + e, d[t].y) : 0.f;
    w1[t] = d[t].w >= 0 ? entry_weight(weights_of<E>(wa) + (e + 1), d[t].w) : 0.f;
  }
  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const bool cok = pbase + s * VEC < cend;
    const int c = cok ? lane_col<VEC>(pbase + s * VEC, cend) : 0;
    const int csafe = c;
    typename Ln::raw_t v0[T], v1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) v0[t] = v1[t] = Ln::zero();
    if (any1) {
#pragma unroll
      for (int t = 0; t < T; ++t) v0[t] = Ln::load(X + (size_t)max(d[t].y, 0) * a.ldx + csafe);
    }
    if (any2) {
#pragma unroll
      for (int t = 0; t < T; ++t) v1[t] = Ln::load(X + (size_t)max(d[t].w, 0) * a.ldx + csafe);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      typename Ln::acc_t acc = azero<VEC>();
      if (d[t].y >= 0) wfma<E, VEC>(acc, w0[t], v0[t]);
      if (d[t].w >= 0) wfma<E, VEC>(acc, w1[t], v1[t]);
      if (cok && d[t].z >= 0) {
        if (d[t].x >= 0) Ln::store(Z + (size_t)d[t].x * a.ldz + c, acc);
        else Ln::store_partial(a.partial + (size_t)(-(d[t].x + 1)) * (size_t)a.D + c, acc);
      }
    }
  }
}

// ---------------------------------------------------------------- dense-tile path
// Per-lane entry tracking: lane l's row is i = l & 15; of a k-step's 64-bit mask, row i owns bits i, 16 + i, 32 + i, 48 + i
// (k = 0..3) and lane l's own bit is l.  `run` = the row's first entry + the set bits of earlier k-steps.
struct EntryRun {
  unsigned long long rowbits, below;
  int run;
  __device__ __forceinline__ EntryRun(int lane, int first) {
    rowbits = 0x0001000100010001ull << (lane & 15);
    below = (1ull << lane) - 1ull;
    run = first;
  }
  // entry of this lane in a k-step with mask m (m = 0 for steps past the end); 0 (a valid index: the window has
  // entries) when the lane's bit is clear -- *on tells
  __device__ __forceinline__ int step(unsigned long long m, int lane, bool* on) {
    const unsigned long long mr = m & rowbits;
    *on = ((mr >> lane) & 1ull) != 0;
    const int e = *on ? run + __popcll(mr & below) : 0;
    run += __popcll(mr);
    return e;
  }
};

__device__ __forceinline__ int window_row_first(const int* __restrict__ rowptr, int window, int N, int lane) {
  const int row = window * 16 + (lane & 15);
  return row < N ? rowptr[row] : 0;
}

template <typename E, int VEC, typename W>
__device__ __forceinline__ void dense_chain_w(const typename E::T* __restrict__ X, const int* __restrict__ U, cu64_p masks,
                                              int K4, int csafe, bool cok, size_t ldx, int lane, f32x4 (&acc)[VEC],
                                              typename WParam<W>::type vals, EntryRun& er) {
  typedef Lane<E, VEC> Ln;
  const int kq = lane >> 4;
  for (int kb = 0; kb < K4; kb += 16) {
    const int myU = (kb * 4 + lane < K4 * 4) ? U[kb * 4 + lane] : -1;
    const int steps = min(16, K4 - kb);
    // half the binary batch: with the value operand next to every gather, the full batch spilled 60-76 bytes per lane
    // at five waves per SIMD (the compact records keep their 8-step batches)
    constexpr int B0 = HCSPMM_DENSE_B * 8 / (VEC * (int)sizeof(typename E::T));
    constexpr int B = (sizeof(typename E::T) == 1 && B0 > HCSPMM_DENSE_B / 2) ? HCSPMM_DENSE_B / 2 : B0;  // (8-bit rows: as at 16 bytes per lane)
    for (int t0 = 0; t0 < steps; t0 += B) {
      int idx[B];
      bool on[B];
      typename Ln::raw_t x[B];
      float a[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int t = t0 + u;
        idx[u] = __shfl(myU, (4 * t + kq) & 63, 64);
        const unsigned long long m = t < steps ? masks[min(kb + t, K4 - 1)] : 0ull;  // wave-uniform: scalar load
        a[u] = entry_weight(vals + er.step(m, lane, &on[u]), max(idx[u], 0));  // the value loads lead the batch: the entry positions die at once
        if (t >= steps) idx[u] = -1;
      }
#pragma unroll
      for (int u = 0; u < B; ++u) x[u] = Ln::load(X + (size_t)max(idx[u], 0) * ldx + csafe);
#pragma unroll
      for (int u = 0; u < B; ++u) {
        if (!(cok && idx[u] >= 0)) x[u] = Ln::zero();
        if (!on[u]) a[u] = 0.0f;
        if (t0 + u < steps) {
#pragma unroll
          for (int q = 0; q < VEC; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], Ln::elem(x[u], q), acc[q], 0, 0, 0);
        }
      }
    }
  }
}

template <typename E, int VEC, typename W>
__device__ __forceinline__ void dense_unit_w(const typename E::T* __restrict__ X, typename E::Z* __restrict__ Z,
                                             const int* __restrict__ U, cu64_p masks, int K4, int window, int panel, int N,
                                             int D, size_t ldx, size_t ldz, int lane, typename WParam<W>::type vals,
                                             const int* __restrict__ rowptr) {
  const int kq = lane >> 4, j = lane & 15;
  const bool cok = panel * 16 * VEC + j * VEC < D;
  const int c = cok ? lane_col<VEC>(panel * 16 * VEC + j * VEC, D) : 0;
  f32x4 acc[VEC];
#pragma unroll
  for (int q = 0; q < VEC; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  EntryRun er(lane, window_row_first(rowptr, window, N, lane));
  dense_chain_w<E, VEC, W>(X, U, masks, K4, c, cok, ldx, lane, acc, vals, er);
  if (cok) dense_store<E, VEC>(Z, acc, window, kq, c, N, ldz);
}

// CompactSteps (spmm_impl.h) with weights
template <typename E, int VEC, int C, int KMAX, int STEPS, int T0>
struct CompactStepsW {
  template <int U, typename W>
  static __device__ __forceinline__ void meta(const Rec<C>& rec, int K4, int kq, int lane, int* idx, float* a, bool* on,
                                              typename WParam<W>::type vals, EntryRun& er) {
    if constexpr (U < STEPS) {
      constexpr int t = T0 + U;
      idx[U] = rec.template gather4<2 + 4 * t>(kq);
      const unsigned lo = (unsigned)rec.template scalar<2 + KMAX + 2 * t>();
      const unsigned hi = (unsigned)rec.template scalar<3 + KMAX + 2 * t>();
      const unsigned long long m = t < K4 ? (((unsigned long long)hi << 32) | lo) : 0ull;
      a[U] = entry_weight(vals + er.step(m, lane, &on[U]), max(idx[U], 0));
      if (t >= K4) idx[U] = -1;
      meta<U + 1, W>(rec, K4, kq, lane, idx, a, on, vals, er);
    }
  }
  template <typename W>
  static __device__ __forceinline__ void run(const typename E::T* __restrict__ X, const Rec<C>& rec, int K4, int csafe, bool cok,
                                             size_t ldx, int lane, f32x4 (&acc)[VEC], typename WParam<W>::type vals, EntryRun& er) {
    typedef Lane<E, VEC> Ln;
    int idx[STEPS];
    bool on[STEPS];
    typename Ln::raw_t x[STEPS];
    float a[STEPS];
    meta<0, W>(rec, K4, lane >> 4, lane, idx, a, on, vals, er);
#pragma unroll
    for (int u = 0; u < STEPS; ++u) x[u] = Ln::load(X + (size_t)max(idx[u], 0) * ldx + csafe);
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
      if (!(cok && idx[u] >= 0)) x[u] = Ln::zero();
      if (!on[u]) a[u] = 0.0f;
      if (T0 + u < K4) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], Ln::elem(x[u], q), acc[q], 0, 0, 0);
      }
    }
  }
};

template <typename E, int VEC, int C, typename W>
__device__ __forceinline__ void dense_compact_unit_w(const typename E::T* __restrict__ X, typename E::Z* __restrict__ Z,
                                                     const int* __restrict__ recp, int panel, int N, int D, size_t ldx,
                                                     size_t ldz, int lane, typename WParam<W>::type vals,
                                                     const int* __restrict__ rowptr) {
  constexpr int KMAX = C == 1 ? HCSPMM_COMPACT_K : HCSPMM_COMPACT2_K;
  Rec<C> rec;
#pragma unroll
  for (int c = 0; c < C; ++c) rec.w[c] = recp[64 * c + lane];
  const int window = rec.template scalar<0>();
  const int K4 = rec.template scalar<1>();
  const int kq = lane >> 4, j = lane & 15;
  const bool cok = panel * 16 * VEC + j * VEC < D;
  const int c = cok ? lane_col<VEC>(panel * 16 * VEC + j * VEC, D) : 0;
  f32x4 acc[VEC];
#pragma unroll
  for (int q = 0; q < VEC; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  EntryRun er(lane, window_row_first(rowptr, window, N, lane));
  typedef CompactStepsW<E, VEC, C, KMAX, 8, 0> S8;
  if constexpr (C == 1) {  // K4 <= 10
    if (K4 <= 2) CompactStepsW<E, VEC, C, KMAX, 2, 0>::template run<W>(X, rec, K4, c, cok, ldx, lane, acc, vals, er);
    else if (K4 <= 4) CompactStepsW<E, VEC, C, KMAX, 4, 0>::template run<W>(X, rec, K4, c, cok, ldx, lane, acc, vals, er);
    else {
      S8::template run<W>(X, rec, K4, c, cok, ldx, lane, acc, vals, er);
      if (K4 > 8) CompactStepsW<E, VEC, C, KMAX, 2, 8>::template run<W>(X, rec, K4, c, cok, ldx, lane, acc, vals, er);
    }
  } else {  // 12 <= K4 <= 20
    S8::template run<W>(X, rec, K4, c, cok, ldx, lane, acc, vals, er);
    if (K4 <= 12) CompactStepsW<E, VEC, C, KMAX, 4, 8>::template run<W>(X, rec, K4, c, cok, ldx, lane, acc, vals, er);
    else {
      CompactStepsW<E, VEC, C, KMAX, 8, 8>::template run<W>(X, rec, K4, c, cok, ldx, lane, acc, vals, er);
      if (K4 > 16) CompactStepsW<E, VEC, C, KMAX, 4, 16>::template run<W>(X, rec, K4, c, cok, ldx, lane, acc, vals, er);
    }
  }
  if (cok) dense_store<E, VEC>(Z, acc, window, kq, c, N, ldz);
}

// ------------------------------------------------------------------------------------------
// Planned weighted kernel: hybrid_plan_kernel's region layout (sliced | wide | ordinary | tiny per column panel, then
// the dense units), no fused forms.
// ------------------------------------------------------------------------------------------
template <typename E, int L, int VEC, int UNROLL, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void hybrid_plan_w_kernel(WPlanArgs wa) {
  typedef typename E::T elem_t;
  const PlanArgs& a = wa.p;
  const elem_t* X = reinterpret_cast<const elem_t*>(a.X);
  typename E::Z* Z = reinterpret_cast<typename E::Z*>(a.Z);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  typedef decltype(weights_of<E>(wa)) W;
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
      typename E::Z* dz = (t.w < 0) ? Z + (size_t)t.x * a.ldz : nullptr;
      float* dp = (t.w < 0) ? nullptr : a.partial + (size_t)t.w * (size_t)a.D;
      sparse_task_w<E, L, VEC, true, UNROLL>(X, dz, dp, a.col, weights_of<E>(wa), __builtin_amdgcn_readfirstlane(t.y),
                                             __builtin_amdgcn_readfirstlane(t.z), a.ldx, c0, cend, lane);
    } else if (bf >= sparse_wgs_pp_ordinary_end(a)) {
      if (bf >= a.free_wgs_pp) return;
      constexpr int R = 64 / L;
      const int first = a.n_tasks - a.n_tiny + ((bf - sparse_wgs_pp_ordinary_end(a)) * kWaves + wave) * (R * TinyWT<E, L>::value);
      if (first >= a.n_tasks) return;
      tiny_tasks_w<E, L, VEC, TinyWT<E, L>::value>(wa, first, c0, cend, lane);
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
      typename E::Z* dz = nullptr;
      float* dp = nullptr;
      if (tp != nullptr) {
        const int4 t = *tp;
        if (t.x >= 0) {
          e0 = t.y;
          n = t.z;
          if (t.w < 0) dz = Z + (size_t)t.x * a.ldz;
          else dp = a.partial + (size_t)t.w * (size_t)a.D;
        }
      }
      sparse_task_w<E, L, VEC, false, UNROLL>(X, dz, dp, a.col, weights_of<E>(wa), e0, n, a.ldx, c0, cend, lane);
    }
  } else {
    constexpr int VM = DenseV<VEC>::mid;
    int unit = ((int)blockIdx.x - a.sparse_wgs) * kWaves + wave;
    if (unit >= a.n_dense * a.n_panels) return;
    const int n_reg = a.n_dense - a.n_dense_compact - a.n_dense_compact2;
    if (unit >= n_reg * a.n_panels) {
      unit -= n_reg * a.n_panels;
      if (unit < a.n_dense_compact2 * a.n_panels) {
        const int panel = unit / a.n_dense_compact2, ci = unit - panel * a.n_dense_compact2;
        const int* rec = a.plan + a.off_dense_compact2 + ci * HCSPMM_COMPACT2_WORDS;
        if (a.dense_vec == VEC) dense_compact_unit_w<E, VEC, 2, W>(X, Z, rec, panel, a.N, a.D, a.ldx, a.ldz, lane, weights_of<E>(wa), wa.rowptr);
        else if (a.dense_vec == VM) dense_compact_unit_w<E, VM, 2, W>(X, Z, rec, panel, a.N, a.D, a.ldx, a.ldz, lane, weights_of<E>(wa), wa.rowptr);
        else dense_compact_unit_w<E, 1, 2, W>(X, Z, rec, panel, a.N, a.D, a.ldx, a.ldz, lane, weights_of<E>(wa), wa.rowptr);
        return;
      }
      unit -= a.n_dense_compact2 * a.n_panels;
      const int panel = unit / a.n_dense_compact, ci = unit - panel * a.n_dense_compact;
      const int* rec = a.plan + a.off_dense_compact + ci * HCSPMM_COMPACT_WORDS;
      if (a.dense_vec == VEC) dense_compact_unit_w<E, VEC, 1, W>(X, Z, rec, panel, a.N, a.D, a.ldx, a.ldz, lane, weights_of<E>(wa), wa.rowptr);
      else if (a.dense_vec == VM) dense_compact_unit_w<E, VM, 1, W>(X, Z, rec, panel, a.N, a.D, a.ldx, a.ldz, lane, weights_of<E>(wa), wa.rowptr);
      else dense_compact_unit_w<E, 1, 1, W>(X, Z, rec, panel, a.N, a.D, a.ldx, a.ldz, lane, weights_of<E>(wa), wa.rowptr);
      return;
    }
    const int panel = unit / n_reg, di = unit - panel * n_reg;
    cint_p dix = (cint_p)(a.plan + a.off_dense_index) + 4 * di;
    const int4 d = int4{dix[0], dix[1], dix[2], dix[3]};
    const int* U = a.plan + a.off_dense_pack + d.y;
    cu64_p masks = (cu64_p)(U + 4 * d.z);
    if (a.dense_vec == VEC) dense_unit_w<E, VEC, W>(X, Z, U, masks, d.z, d.x, panel, a.N, a.D, a.ldx, a.ldz, lane, weights_of<E>(wa), wa.rowptr);
    else if (a.dense_vec == VM) dense_unit_w<E, VM, W>(X, Z, U, masks, d.z, d.x, panel, a.N, a.D, a.ldx, a.ldz, lane, weights_of<E>(wa), wa.rowptr);
    else dense_unit_w<E, 1, W>(X, Z, U, masks, d.z, d.x, panel, a.N, a.D, a.ldx, a.ldz, lane, weights_of<E>(wa), wa.rowptr);
  }
}

// tiny_kernel (spmm_impl.h) with weights
// (the 8-bit build holds values, scales and fp32 sums of 8 columns per lane: 6 waves per SIMD, nothing spilled; at 8 it spills 44 bytes)
template <typename E> struct TinyWWaves { static constexpr int value = sizeof(typename E::T) == 1 ? 6 : HCSPMM_TINY_KERNEL_WAVES; };
template <typename E, int L, int VEC>
__global__ __launch_bounds__(kThreads, TinyWWaves<E>::value) void tiny_w_kernel(WPlanArgs wa) {
  const PlanArgs& a = wa.p;
  constexpr int R = 64 / L, T = HCSPMM_TINY_KERNEL_T;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = (int)blockIdx.x / a.tiny_kernel_wgs;
  const int b = (int)blockIdx.x - p * a.tiny_kernel_wgs;
  const int c0 = p * a.panel_cols;
  const int first = a.n_tasks - a.n_tiny + (b * kWaves + wave) * (R * T);
  if (first >= a.n_tasks) return;
  tiny_tasks_w<E, L, VEC, T>(wa, first, c0, min(a.D, c0 + a.panel_cols), lane);
}

// ------------------------------------------------------------------------------------------
// Plan-free weighted kernel: hybrid_window_kernel with weights.  Sparse windows walk CSR entries themselves (e at hand);
// dense windows rebuild U / masks in LDS as the binary kernel does and find each lane's entry by the running popcount,
// carried across the LDS chunks (they follow ascending condensed columns).
// ------------------------------------------------------------------------------------------
template <typename E, int L, int VEC>
__global__ __launch_bounds__(kThreads) void hybrid_window_w_kernel(WWindowArgs wa) {
  typedef Lane<E, VEC> Ln;
  typedef typename E::T elem_t;
  const WindowArgs& a = wa.w;
  const typename WParam<decltype(weights_of<E>(wa))>::type vals = weights_of<E>(wa);
  const elem_t* X = reinterpret_cast<const elem_t*>(a.X);
  typename E::Z* Z = reinterpret_cast<typename E::Z*>(a.Z);
  __shared__ int s_U[kChunkK];
  __shared__ unsigned int s_mask[kChunkK / 4 * 2];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nthreads = (int)blockDim.x, nwaves = nthreads >> 6;
  const int w = blockIdx.x;
  const int r0 = w * 16, r1 = min(r0 + 16, a.N);
  if (a.hybrid_type[w] == 0) {
    constexpr int R = 64 / L;
    const int G = R * nwaves;
    const int gi = wave * R + lane / L;
    for (int rb = r0; rb < r1; rb += G) {
      const int r = rb + gi;
      int e0 = 0, n = 0;
      typename E::Z* dst = nullptr;
      if (r < r1) {
        e0 = a.rowptr[r];
        n = a.rowptr[r + 1] - e0;
        dst = Z + (size_t)r * a.ldz;
        if (R > 1 && n > kPlanFreeWide) {
          n = 0;
          dst = nullptr;
        }
      }
      sparse_task_w<E, L, VEC, false>(X, dst, nullptr, a.col, vals, e0, n, a.ldx, 0, a.D, lane);
    }
    if (R > 1) {
      int k = 0;
      for (int r = r0; r < r1; ++r) {
        const int e0 = a.rowptr[r];
        const int n = a.rowptr[r + 1] - e0;
        if (n > kPlanFreeWide) {
          if (k % nwaves == wave)
            sparse_task_w<E, L, VEC, true>(X, Z + (size_t)r * a.ldz, nullptr, a.col, vals, e0, n, a.ldx, 0, a.D, lane);
          ++k;
        }
      }
    }
    return;
  }
  const int lo = a.rowptr[r0], hi = a.rowptr[r1];
  const int K = a.blockPartition[w] * 8;
  const int n_panels = (a.D + 16 * VEC - 1) / (16 * VEC);
  const int kq = lane >> 4, j = lane & 15;
  const int first = r0 + j < r1 ? a.rowptr[r0 + j] : 0;
  for (int pb = 0; pb < n_panels; pb += nwaves) {
    const int panel = pb + wave;
    const bool cok = panel < n_panels && panel * 16 * VEC + j * VEC < a.D;
    const int c = cok ? lane_col<VEC>(panel * 16 * VEC + j * VEC, a.D) : 0;
    f32x4 acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    EntryRun er(lane, first);
    for (int k0 = 0; k0 < K; k0 += kChunkK) {
      const int kc = min(kChunkK, K - k0);
      __syncthreads();
      for (int i = threadIdx.x; i < kChunkK; i += nthreads) s_U[i] = -1;
      for (int i = threadIdx.x; i < kChunkK / 2; i += nthreads) s_mask[i] = 0u;
      __syncthreads();
      for (int e = lo + (int)threadIdx.x; e < hi; e += nthreads) {
        const int cc = a.edgeToColumn[e] - k0;
        if (cc >= 0 && cc < kc) {
          const int rl = a.edgeToRow[e] - r0;
          const int bit = 16 * (cc & 3) + rl;
          atomicOr(&s_mask[(cc >> 2) * 2 + (bit >> 5)], 1u << (bit & 31));
          s_U[cc] = a.col[e];
        }
      }
      __syncthreads();
      const int steps = (kc + 3) / 4;
      for (int t0 = 0; t0 < steps; t0 += 4) {
        typename Ln::raw_t x[4];
        float av[4];
        int ent[4], ci[4];
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = t0 + u;
          const bool tv = t < steps;
          const int idx = tv ? s_U[min(4 * t + kq, kChunkK - 1)] : -1;
          const unsigned long long m =
              tv ? ((unsigned long long)s_mask[t * 2 + 1] << 32) | (unsigned long long)s_mask[t * 2] : 0ull;
          ent[u] = er.step(m, lane, &on[u]);
          ci[u] = max(idx, 0);
          x[u] = Ln::zero();
          if (cok && idx >= 0) x[u] = Ln::load(X + (size_t)idx * a.ldx + c);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) av[u] = on[u] ? entry_weight(vals + ent[u], ci[u]) : 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int q = 0; q < VEC; ++q)
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], Ln::elem(x[u], q), acc[q], 0, 0, 0);
        }
      }
    }
    if (cok) dense_store<E, VEC>(Z, acc, w, kq, c, a.N, a.ldz);
  }
}

// ------------------------------------------------------------------------------------------
// Host-side launchers: the grid of launch_plan_LV (plan_layout.h: same regions, same wide / tiny / slice decisions).
// ------------------------------------------------------------------------------------------
template <typename E, int L, int VEC>
static hipError_t launch_plan_w_LV(const WPlanArgs& wa, hipStream_t stream) {
  const PlanArgs& a = wa.p;
  WPlanArgs wb = wa;
  PlanArgs& b = wb.p;
  b.fused = 0;
  const int n_col_panels = plan_launch_layout(b, L, VEC, DenseV<VEC>::mid, TinyWT<E, L>::value, own_tiny_launch(b.n_tiny, 0), 0);
  constexpr int kMinWaves = sizeof(typename E::T) == 4 ? HCSPMM_MIN_WAVES_PER_SIMD : HCSPMM_MIN_WAVES_H16;
  const long long dense_wgs = ((long long)b.n_dense * b.n_panels + kWaves - 1) / kWaves;
  const long long grid = (long long)b.sparse_wgs + dense_wgs;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (grid > 0)
    hipLaunchKernelGGL((hybrid_plan_w_kernel<E, L, VEC, HCSPMM_SPARSE_U, kMinWaves>), dim3((unsigned)grid), dim3(kThreads), 0,
                       stream, wb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (b.tiny_kernel_wgs > 0) {
    hipLaunchKernelGGL((tiny_w_kernel<E, L, VEC>), dim3((unsigned)(b.tiny_kernel_wgs * n_col_panels)), dim3(kThreads), 0, stream, wb);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.n_split_rows > 0) {  // partial sums of split rows: the binary fix-up pass (it reads no values)
    const int fg = (a.n_split_rows + kWaves - 1) / kWaves;
    hipLaunchKernelGGL((fixup_kernel<E, VEC>), dim3(fg), dim3(kThreads), 0, stream, b);
    e = hipGetLastError();
  }
  return e;
}

template <typename E, int L, int VEC>
static hipError_t launch_window_w_LV(const WWindowArgs& wa, hipStream_t stream) {
  const WindowArgs& a = wa.w;
  const int W = (a.N + 15) / 16;
  const int n_panels = (a.D + 16 * VEC - 1) / (16 * VEC);
  int waves = (16 * L + 63) / 64;
  if (n_panels > waves) waves = n_panels;
  if (waves > kWaves) waves = kWaves;
  if (W > 0) hipLaunchKernelGGL((hybrid_window_w_kernel<E, L, VEC>), dim3(W), dim3(waves * 64), 0, stream, wa);
  return hipGetLastError();
}

}  // namespace hcspmm
