// spmm_weighted_heads_impl.h -- device code and launchers of the multi-head edge-weighted hybrid SpMM, in its two forms
// (DESIGN.md sections 3.11 and 3.14); instantiated by spmm_weighted_heads.hip (direct) and spmm_weighted_indexed.hip (indexed):
//   Z[r][h*Dh + j] = sum over the entries e of row r of values[h*nE + pos(e)] * X[col(e)][h*Dh + j],   D = heads * Dh, fp32,
//   pos(e) = e (direct: values aligned with column_index) or vindex[e] (indexed: the backward through A^T needs no permuted
//   copy of the values).  INDEXED, a compile-time flag of every template below, is the only difference between the two:
//   the indexed form with values[:, vindex] materialised gives every column the fmaf chain of the direct form, the same bits.
//
// The kernels are spmm_weighted_impl.h's (same regions, tasks, batches, combine trees and fix-up pass) with one change: the
// weight of a (entry, column) pair is the value of the column's head.  Dh % 4 == 0, so a lane's 4 / 2 / 1 columns never
// span two heads (and no lane is ever moved back by lane_col: D is a multiple of 4 and every lane starts on its own
// multiple); the indexed form also takes one head of any D (there is a single head to pick, whatever a lane's columns).
// Every column therefore gets the fmaf chain hcspmm_forward_weighted gives it with that head's values.
//  * sparse-row tasks (ordinary, wide, sliced, plan-free rows): the column indices are loaded and broadcast as before, one
//    load per entry for all heads; each lane loads the value of its own head for the entries of its batch.  Direct: at the
//    entry's own position, known from the batch's base.  Indexed: vindex[e] is loaded beside col[e], one coalesced load per
//    entry for all heads, broadcast by the same __shfl and prefetched with the next column index.
//  * tiny tasks: the (<= 2) value positions are found once per task, ahead of the column passes; each column pass loads the
//    values of its lanes' heads.
//  * dense-tile windows: a lane's entry (running popcount) gives its value position once (indexed: through vindex); every
//    head's value load uses it.  The A operand of v_mfma_f32_16x16x4_f32 is one value per (row, k) for all 16 columns of
//    the tile, so a tile covering several heads takes one MFMA per head, in ascending head order, with the B columns of the
//    other heads zeroed.  Adding fmaf(v, 0, acc) to a column leaves its finite acc unchanged (up to the sign of a zero), so
//    each column sees exactly the chain of its own head's MFMAs.  A single-head tile is the weighted kernel's step as it is.
#pragma once
#include "spmm_weighted_impl.h"

namespace hcspmm {
namespace {

// gather_batch_w with per-lane values: lanes past a task's end (idx -1) weigh 0, nothing read.  Direct: the batch's entries
// start at ebase.  Indexed: the value positions (myvi) are broadcast alongside the column indices, and prefetched with them
template <typename E, int VEC, int UB, bool INDEXED>
__device__ __forceinline__ void gather_batch_wh(const typename E::T* __restrict__ X, size_t ldx, int csafe, bool cok, int myidx,
                                                int myvi, const float* __restrict__ hv, int ebase, int src0,
                                                typename AccT<VEC>::type& acc, const int* pf_col, const int* pf_vi, int& next,
                                                int& nextvi) {
  typedef Lane<E, VEC> Ln;
  int idx[UB], vi[UB];
  float w[UB];
  typename Ln::raw_t v[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    idx[u] = __shfl(myidx, src0 + u, 64);
    if constexpr (INDEXED) vi[u] = __shfl(myvi, src0 + u, 64);
    else vi[u] = ebase + u;
  }
#pragma unroll
  for (int u = 0; u < UB; ++u) w[u] = idx[u] >= 0 ? hv[vi[u]] : 0.f;
  if (pf_col != nullptr) {
    next = *pf_col;
    if constexpr (INDEXED) nextvi = *pf_vi;
  }
#pragma unroll
  for (int u = 0; u < UB; ++u) v[u] = Ln::load(X + (size_t)max(idx[u], 0) * ldx + csafe);
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    if (!(cok && idx[u] >= 0)) v[u] = Ln::zero();
    wfma<E, VEC>(acc, w[u], v[u]);
  }
}

// sparse_task_w with the values of the lanes' heads (vals: [heads][nE], vindex: [entries] when INDEXED, dh: columns per head)
template <typename E, int L, int VEC, bool WIDE, bool INDEXED, int UMAX = HCSPMM_SPARSE_U>
__device__ __forceinline__ void sparse_task_wh(const typename E::T* __restrict__ X, typename E::T* __restrict__ dstZ,
                                               float* __restrict__ dstP, const int* __restrict__ col,
                                               const int* __restrict__ vindex, const float* __restrict__ vals, long long nE,
                                               int dh, int e0, int n, size_t ldx, int c0, int cend, int lane) {
  typedef Lane<E, VEC> Ln;
  typedef typename Ln::acc_t acc_t;
  constexpr int U = (L < UMAX) ? L : UMAX;
  constexpr int STRIDE = WIDE ? 64 : L;
  const int s = lane & (L - 1);
  const int pos = WIDE ? lane : s;
  const int gbase = lane & ~(L - 1);
  const int eg = e0 + (WIDE ? gbase : 0);  // direct: entry of broadcast source gbase + 0 in the first stride
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
    const float* __restrict__ hv = vals + (size_t)(c / dh) * (size_t)nE;
    acc_t acc = azero<VEC>();
    int next = -1, nextvi = 0;
    if (pos < n) {
      next = col[e0 + pos];
      if constexpr (INDEXED) nextvi = vindex[e0 + pos];
    }
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next, myvi = nextvi;
      const bool more = base + STRIDE + pos < n;
      next = -1;
      const int cnt = min(L, nmax - base);
      const int* pf = more ? col + e0 + base + STRIDE + pos : nullptr;
      const int* pfv = INDEXED ? vindex + e0 + base + STRIDE + pos : nullptr;  // read only when pf is set
      const int eb = eg + base;
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
#define HCSPMM_WH_BATCH(UB) gather_batch_wh<E, VEC, UB, INDEXED>(X, ldx, csafe, cok, myidx, myvi, hv, eb + j, gbase + j, acc, pf, pfv, next, nextvi)
        if (left > U / 2) {
          HCSPMM_WH_BATCH(U);
          j += U;
        } else if (U >= 8 && left > U / 4) {
          HCSPMM_WH_BATCH((U >= 8 ? U / 2 : 1));
          j += U / 2;
        } else if (U >= 4 && left > 1) {
          HCSPMM_WH_BATCH((U >= 8 ? U / 4 : 2));
          j += (U >= 8 ? U / 4 : 2);
        } else {
          HCSPMM_WH_BATCH(1);
          j += 1;
        }
#undef HCSPMM_WH_BATCH
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

// tiny_tasks_w with per-head values: the value positions once, the values per column pass
template <typename E, int L, int VEC, int T, bool INDEXED>
__device__ __forceinline__ void tiny_tasks_wh(const WHPlanArgs& ha, int first, int c0, int cend, int lane) {
  typedef Lane<E, VEC> Ln;
  typedef typename E::T elem_t;
  const WPlanArgs& wa = ha.w;
  const PlanArgs& a = wa.p;
  const elem_t* X = reinterpret_cast<const elem_t*>(a.X);
  elem_t* Z = reinterpret_cast<elem_t*>(a.Z);
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
  int p0[T], p1[T];  // value positions of the task's first and second entry (direct: p0 + 1, p1 unused)
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if constexpr (INDEXED) {
      int e = 0;
      if (d[t].y >= 0) e = d[t].x >= 0 ? wa.rowptr[d[t].x] : segment_entry(a, wa.rowptr, wa.segment_len, -(d[t].x + 1));
      p0[t] = d[t].y >= 0 ? ha.vindex[e] : 0;
      p1[t] = d[t].w >= 0 ? ha.vindex[e + 1] : 0;
    } else {
      p0[t] = 0;
      if (d[t].y >= 0) p0[t] = d[t].x >= 0 ? wa.rowptr[d[t].x] : segment_entry(a, wa.rowptr, wa.segment_len, -(d[t].x + 1));
    }
  }
  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const bool cok = pbase + s * VEC < cend;
    const int c = cok ? lane_col<VEC>(pbase + s * VEC, cend) : 0;
    const int csafe = c;
    const float* __restrict__ hv = wa.values + (size_t)(c / ha.dh) * (size_t)ha.E;
    float w0[T], w1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      w0[t] = d[t].y >= 0 ? hv[p0[t]] : 0.f;
      w1[t] = d[t].w >= 0 ? hv[INDEXED ? p1[t] : p0[t] + 1] : 0.f;
    }
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
// The heads a tile of 16 * VEC columns starting at column c0 covers: [h0, h1]; hl = the lane's own head.
struct TileHeads {
  int h0, h1, hl;
  __device__ __forceinline__ TileHeads(int c0, int width, int D, int dh, int c) {
    h0 = c0 / dh;
    h1 = (min(D, c0 + width) - 1) / dh;
    hl = c / dh;
  }
};

// the MFMAs of a batch of S k-steps, of which the first n are real: head h0's with the values a0 loaded alongside the
// gathers, then each further head's, its values loaded for the whole batch first.  ent[u]: the lane's value position in
// step u, < 0 when it has no entry there (value 0).  A lane's B operand is its X elements in its own head's MFMAs and 0 in
// the others'.
template <typename E, int VEC, int S>
__device__ __forceinline__ void heads_batch(f32x4 (&acc)[VEC], const typename Lane<E, VEC>::raw_t (&x)[S], const float (&a0)[S],
                                            const int (&ent)[S], int n, const float* __restrict__ vals, long long nE,
                                            const TileHeads& th) {
  typedef Lane<E, VEC> Ln;
#pragma unroll
  for (int u = 0; u < S; ++u) {
    if (u < n) {
#pragma unroll
      for (int q = 0; q < VEC; ++q)
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], th.hl == th.h0 ? Ln::elem(x[u], q) : 0.0f, acc[q], 0, 0, 0);
    }
  }
  for (int h = th.h0 + 1; h <= th.h1; ++h) {
    const float* __restrict__ vh = vals + (size_t)h * (size_t)nE;
    float a[S];
#pragma unroll
    for (int u = 0; u < S; ++u) a[u] = ent[u] >= 0 ? vh[ent[u]] : 0.0f;
#pragma unroll
    for (int u = 0; u < S; ++u) {
      if (u < n) {
#pragma unroll
        for (int q = 0; q < VEC; ++q)
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], th.hl == h ? Ln::elem(x[u], q) : 0.0f, acc[q], 0, 0, 0);
      }
    }
  }
}

// (The k-step of dense_chain_wh and CompactStepsWH::meta -- a lane's value position, -1 without an entry, and head h0's value
// there -- is written out at both sites: behind a helper function the direct form's planned kernel allocates its registers
// differently, and the direct form must stay the code it was.)
template <typename E, int VEC, bool INDEXED>
__device__ __forceinline__ void dense_chain_wh(const typename E::T* __restrict__ X, const int* __restrict__ U, cu64_p masks,
                                               int K4, int csafe, bool cok, size_t ldx, int lane, f32x4 (&acc)[VEC],
                                               const int* __restrict__ vindex, const float* __restrict__ vals, long long nE,
                                               const TileHeads& th, EntryRun& er) {
  typedef Lane<E, VEC> Ln;
  const int kq = lane >> 4;
  const float* __restrict__ v0 = vals + (size_t)th.h0 * (size_t)nE;
  for (int kb = 0; kb < K4; kb += 16) {
    const int myU = (kb * 4 + lane < K4 * 4) ? U[kb * 4 + lane] : -1;
    const int steps = min(16, K4 - kb);
    // half the weighted kernel's batch: the value positions stay live for the further heads' value loads
    constexpr int B = HCSPMM_DENSE_B * 4 / (VEC * (int)sizeof(typename E::T));
    for (int t0 = 0; t0 < steps; t0 += B) {
      int idx[B], ent[B];
      typename Ln::raw_t x[B];
      float a[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int t = t0 + u;
        idx[u] = __shfl(myU, (4 * t + kq) & 63, 64);
        const unsigned long long m = t < steps ? masks[min(kb + t, K4 - 1)] : 0ull;  // wave-uniform: scalar load
        bool on;
        const int e = er.step(m, lane, &on);
        if constexpr (INDEXED) {
          ent[u] = on ? vindex[e] : -1;
          a[u] = on ? v0[ent[u]] : 0.0f;
        } else {
          ent[u] = e;
          a[u] = on ? v0[ent[u]] : 0.0f;
          if (!on) ent[u] = -1;
        }
        if (t >= steps) idx[u] = -1;
      }
#pragma unroll
      for (int u = 0; u < B; ++u) x[u] = Ln::load(X + (size_t)max(idx[u], 0) * ldx + csafe);
#pragma unroll
      for (int u = 0; u < B; ++u)
        if (!(cok && idx[u] >= 0)) x[u] = Ln::zero();
      heads_batch<E, VEC, B>(acc, x, a, ent, steps - t0, vals, nE, th);
    }
  }
}

template <typename E, int VEC, bool INDEXED>
__device__ __forceinline__ void dense_unit_wh(const typename E::T* __restrict__ X, typename E::T* __restrict__ Z,
                                              const int* __restrict__ U, cu64_p masks, int K4, int window, int panel, int N, int D,
                                              size_t ldx, size_t ldz, int lane, const int* __restrict__ vindex,
                                              const float* __restrict__ vals, long long nE, int dh,
                                              const int* __restrict__ rowptr) {
  const int kq = lane >> 4, j = lane & 15;
  const bool cok = panel * 16 * VEC + j * VEC < D;
  const int c = cok ? lane_col<VEC>(panel * 16 * VEC + j * VEC, D) : 0;
  const TileHeads th(panel * 16 * VEC, 16 * VEC, D, dh, c);
  f32x4 acc[VEC];
#pragma unroll
  for (int q = 0; q < VEC; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  EntryRun er(lane, window_row_first(rowptr, window, N, lane));
  dense_chain_wh<E, VEC, INDEXED>(X, U, masks, K4, c, cok, ldx, lane, acc, vindex, vals, nE, th, er);
  if (cok) dense_store<E, VEC>(Z, acc, window, kq, c, N, ldz);
}

// CompactStepsW with per-head values
template <typename E, int VEC, int C, int KMAX, int STEPS, int T0, bool INDEXED>
struct CompactStepsWH {
  template <int U>
  static __device__ __forceinline__ void meta(const Rec<C>& rec, int K4, int kq, int lane, int* idx, int* ent, float* a,
                                              const int* __restrict__ vindex, const float* __restrict__ v0, EntryRun& er) {
    if constexpr (U < STEPS) {
      constexpr int t = T0 + U;
      idx[U] = rec.template gather4<2 + 4 * t>(kq);
      const unsigned lo = (unsigned)rec.template scalar<2 + KMAX + 2 * t>();
      const unsigned hi = (unsigned)rec.template scalar<3 + KMAX + 2 * t>();
      const unsigned long long m = t < K4 ? (((unsigned long long)hi << 32) | lo) : 0ull;
      bool on;
      const int e = er.step(m, lane, &on);
      if constexpr (INDEXED) {
        ent[U] = on ? vindex[e] : -1;
        a[U] = on ? v0[ent[U]] : 0.0f;
      } else {
        ent[U] = e;
        a[U] = on ? v0[ent[U]] : 0.0f;
        if (!on) ent[U] = -1;
      }
      if (t >= K4) idx[U] = -1;
      meta<U + 1>(rec, K4, kq, lane, idx, ent, a, vindex, v0, er);
    }
  }
  static __device__ __forceinline__ void run(const typename E::T* __restrict__ X, const Rec<C>& rec, int K4, int csafe, bool cok,
                                             size_t ldx, int lane, f32x4 (&acc)[VEC], const int* __restrict__ vindex,
                                             const float* __restrict__ vals, long long nE, const TileHeads& th, EntryRun& er) {
    typedef Lane<E, VEC> Ln;
    int idx[STEPS], ent[STEPS];
    typename Ln::raw_t x[STEPS];
    float a[STEPS];
    meta<0>(rec, K4, lane >> 4, lane, idx, ent, a, vindex, vals + (size_t)th.h0 * (size_t)nE, er);
#pragma unroll
    for (int u = 0; u < STEPS; ++u) x[u] = Ln::load(X + (size_t)max(idx[u], 0) * ldx + csafe);
#pragma unroll
    for (int u = 0; u < STEPS; ++u)
      if (!(cok && idx[u] >= 0)) x[u] = Ln::zero();
    heads_batch<E, VEC, STEPS>(acc, x, a, ent, K4 - T0, vals, nE, th);
  }
};

template <typename E, int VEC, int C, bool INDEXED>
__device__ __forceinline__ void dense_compact_unit_wh(const typename E::T* __restrict__ X, typename E::T* __restrict__ Z,
                                                      const int* __restrict__ recp, int panel, int N, int D, size_t ldx, size_t ldz,
                                                      int lane, const int* __restrict__ vindex, const float* __restrict__ vals,
                                                      long long nE, int dh, const int* __restrict__ rowptr) {
  constexpr int KMAX = C == 1 ? HCSPMM_COMPACT_K : HCSPMM_COMPACT2_K;
  Rec<C> rec;
#pragma unroll
  for (int c = 0; c < C; ++c) rec.w[c] = recp[64 * c + lane];
  const int window = rec.template scalar<0>();
  const int K4 = rec.template scalar<1>();
  const int kq = lane >> 4, j = lane & 15;
  const bool cok = panel * 16 * VEC + j * VEC < D;
  const int c = cok ? lane_col<VEC>(panel * 16 * VEC + j * VEC, D) : 0;
  const TileHeads th(panel * 16 * VEC, 16 * VEC, D, dh, c);
  f32x4 acc[VEC];
#pragma unroll
  for (int q = 0; q < VEC; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  EntryRun er(lane, window_row_first(rowptr, window, N, lane));
  // the weighted kernel's runs with every 8-step run cut in two (registers, as in dense_chain_wh): the same k order
#define HCSPMM_WH_RUN(S, T0) \
  CompactStepsWH<E, VEC, C, KMAX, S, T0, INDEXED>::run(X, rec, K4, c, cok, ldx, lane, acc, vindex, vals, nE, th, er)
  if constexpr (C == 1) {  // K4 <= 10
    if (K4 <= 2) HCSPMM_WH_RUN(2, 0);
    else if (K4 <= 4) HCSPMM_WH_RUN(4, 0);
    else {
      HCSPMM_WH_RUN(4, 0);
      HCSPMM_WH_RUN(4, 4);
      if (K4 > 8) HCSPMM_WH_RUN(2, 8);
    }
  } else {  // 12 <= K4 <= 20
    HCSPMM_WH_RUN(4, 0);
    HCSPMM_WH_RUN(4, 4);
    HCSPMM_WH_RUN(4, 8);
    if (K4 > 12) {
      HCSPMM_WH_RUN(4, 12);
      if (K4 > 16) HCSPMM_WH_RUN(4, 16);
    }
  }
#undef HCSPMM_WH_RUN
  if (cok) dense_store<E, VEC>(Z, acc, window, kq, c, N, ldz);
}

// ------------------------------------------------------------------------------------------
// Planned kernel: hybrid_plan_w_kernel's regions and unit decode
// ------------------------------------------------------------------------------------------
template <typename E, int L, int VEC, int UNROLL, int MINW, bool INDEXED>
__global__ __launch_bounds__(kThreads, MINW) void hybrid_plan_wh_kernel(WHPlanArgs ha) {
  typedef typename E::T elem_t;
  const WPlanArgs& wa = ha.w;
  const PlanArgs& a = wa.p;
  const elem_t* X = reinterpret_cast<const elem_t*>(a.X);
  elem_t* Z = reinterpret_cast<elem_t*>(a.Z);
  const int* __restrict__ vindex = ha.vindex;
  const float* __restrict__ vals = wa.values;
  const long long nE = ha.E;  // values per head
  const int dh = ha.dh;
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
      elem_t* dz = (t.w < 0) ? Z + (size_t)t.x * a.ldz : nullptr;
      float* dp = (t.w < 0) ? nullptr : a.partial + (size_t)t.w * (size_t)a.D;
      sparse_task_wh<E, L, VEC, true, INDEXED, UNROLL>(X, dz, dp, a.col, vindex, vals, nE, dh,
                                                       __builtin_amdgcn_readfirstlane(t.y),
                                                       __builtin_amdgcn_readfirstlane(t.z), a.ldx, c0, cend, lane);
    } else if (bf >= sparse_wgs_pp_ordinary_end(a)) {
      if (bf >= a.free_wgs_pp) return;
      constexpr int R = 64 / L;
      const int first = a.n_tasks - a.n_tiny + ((bf - sparse_wgs_pp_ordinary_end(a)) * kWaves + wave) * (R * TinyT<L>::value);
      if (first >= a.n_tasks) return;
      tiny_tasks_wh<E, L, VEC, TinyT<L>::value, INDEXED>(ha, first, c0, cend, lane);
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
      elem_t* dz = nullptr;
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
      sparse_task_wh<E, L, VEC, false, INDEXED, UNROLL>(X, dz, dp, a.col, vindex, vals, nE, dh, e0, n, a.ldx, c0, cend, lane);
    }
  } else {
    constexpr int VM = DenseV<VEC>::mid;
    int unit = ((int)blockIdx.x - a.sparse_wgs) * kWaves + wave;
    if (unit >= a.n_dense * a.n_panels) return;
    const int n_reg = a.n_dense - a.n_dense_compact - a.n_dense_compact2;
#define HCSPMM_WH_TAIL a.N, a.D, a.ldx, a.ldz, lane, vindex, vals, nE, dh, wa.rowptr
    if (unit >= n_reg * a.n_panels) {
      unit -= n_reg * a.n_panels;
      if (unit < a.n_dense_compact2 * a.n_panels) {
        const int panel = unit / a.n_dense_compact2, ci = unit - panel * a.n_dense_compact2;
        const int* rec = a.plan + a.off_dense_compact2 + ci * HCSPMM_COMPACT2_WORDS;
        if (a.dense_vec == VEC) dense_compact_unit_wh<E, VEC, 2, INDEXED>(X, Z, rec, panel, HCSPMM_WH_TAIL);
        else if (a.dense_vec == VM) dense_compact_unit_wh<E, VM, 2, INDEXED>(X, Z, rec, panel, HCSPMM_WH_TAIL);
        else dense_compact_unit_wh<E, 1, 2, INDEXED>(X, Z, rec, panel, HCSPMM_WH_TAIL);
        return;
      }
      unit -= a.n_dense_compact2 * a.n_panels;
      const int panel = unit / a.n_dense_compact, ci = unit - panel * a.n_dense_compact;
      const int* rec = a.plan + a.off_dense_compact + ci * HCSPMM_COMPACT_WORDS;
      if (a.dense_vec == VEC) dense_compact_unit_wh<E, VEC, 1, INDEXED>(X, Z, rec, panel, HCSPMM_WH_TAIL);
      else if (a.dense_vec == VM) dense_compact_unit_wh<E, VM, 1, INDEXED>(X, Z, rec, panel, HCSPMM_WH_TAIL);
      else dense_compact_unit_wh<E, 1, 1, INDEXED>(X, Z, rec, panel, HCSPMM_WH_TAIL);
      return;
    }
    const int panel = unit / n_reg, di = unit - panel * n_reg;
    cint_p dix = (cint_p)(a.plan + a.off_dense_index) + 4 * di;
    const int4 d = int4{dix[0], dix[1], dix[2], dix[3]};
    const int* U = a.plan + a.off_dense_pack + d.y;
    cu64_p masks = (cu64_p)(U + 4 * d.z);
    if (a.dense_vec == VEC) dense_unit_wh<E, VEC, INDEXED>(X, Z, U, masks, d.z, d.x, panel, HCSPMM_WH_TAIL);
    else if (a.dense_vec == VM) dense_unit_wh<E, VM, INDEXED>(X, Z, U, masks, d.z, d.x, panel, HCSPMM_WH_TAIL);
    else dense_unit_wh<E, 1, INDEXED>(X, Z, U, masks, d.z, d.x, panel, HCSPMM_WH_TAIL);
#undef HCSPMM_WH_TAIL
  }
}

// tiny_w_kernel with per-head values
template <typename E, int L, int VEC, bool INDEXED>
__global__ __launch_bounds__(kThreads, HCSPMM_TINY_KERNEL_WAVES) void tiny_wh_kernel(WHPlanArgs ha) {
  const PlanArgs& a = ha.w.p;
  constexpr int R = 64 / L, T = HCSPMM_TINY_KERNEL_T;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = (int)blockIdx.x / a.tiny_kernel_wgs;
  const int b = (int)blockIdx.x - p * a.tiny_kernel_wgs;
  const int c0 = p * a.panel_cols;
  const int first = a.n_tasks - a.n_tiny + (b * kWaves + wave) * (R * T);
  if (first >= a.n_tasks) return;
  tiny_tasks_wh<E, L, VEC, T, INDEXED>(ha, first, c0, min(a.D, c0 + a.panel_cols), lane);
}

// ------------------------------------------------------------------------------------------
// Plan-free kernel: hybrid_window_w_kernel with per-head values
// ------------------------------------------------------------------------------------------
template <typename E, int L, int VEC, bool INDEXED>
__global__ __launch_bounds__(kThreads) void hybrid_window_wh_kernel(WHWindowArgs ha) {
  typedef Lane<E, VEC> Ln;
  typedef typename E::T elem_t;
  const WindowArgs& a = ha.w.w;
  const int* __restrict__ vindex = ha.vindex;
  const float* __restrict__ vals = ha.w.values;
  const long long nE = ha.E;
  const int dh = ha.dh;
  const elem_t* X = reinterpret_cast<const elem_t*>(a.X);
  elem_t* Z = reinterpret_cast<elem_t*>(a.Z);
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
      elem_t* dst = nullptr;
      if (r < r1) {
        e0 = a.rowptr[r];
        n = a.rowptr[r + 1] - e0;
        dst = Z + (size_t)r * a.ldz;
        if (R > 1 && n > kPlanFreeWide) {
          n = 0;
          dst = nullptr;
        }
      }
      sparse_task_wh<E, L, VEC, false, INDEXED>(X, dst, nullptr, a.col, vindex, vals, nE, dh, e0, n, a.ldx, 0, a.D, lane);
    }
    if (R > 1) {
      int k = 0;
      for (int r = r0; r < r1; ++r) {
        const int e0 = a.rowptr[r];
        const int n = a.rowptr[r + 1] - e0;
        if (n > kPlanFreeWide) {
          if (k % nwaves == wave)
            sparse_task_wh<E, L, VEC, true, INDEXED>(X, Z + (size_t)r * a.ldz, nullptr, a.col, vindex, vals, nE, dh, e0, n, a.ldx,
                                                     0, a.D, lane);
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
    const TileHeads th(min(panel, n_panels - 1) * 16 * VEC, 16 * VEC, a.D, dh, c);
    const float* __restrict__ v0 = vals + (size_t)th.h0 * (size_t)nE;
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
        int ent[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = t0 + u;
          const bool tv = t < steps;
          const int idx = tv ? s_U[min(4 * t + kq, kChunkK - 1)] : -1;
          const unsigned long long m =
              tv ? ((unsigned long long)s_mask[t * 2 + 1] << 32) | (unsigned long long)s_mask[t * 2] : 0ull;
          bool on;
          const int e = er.step(m, lane, &on);
          ent[u] = on ? (INDEXED ? vindex[e] : e) : -1;
          x[u] = Ln::zero();
          if (cok && idx >= 0) x[u] = Ln::load(X + (size_t)idx * a.ldx + c);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) av[u] = ent[u] >= 0 ? v0[ent[u]] : 0.0f;
        heads_batch<E, VEC, 4>(acc, x, av, ent, 4, vals, nE, th);
      }
    }
    if (cok) dense_store<E, VEC>(Z, acc, w, kq, c, a.N, a.ldz);
  }
}

// ------------------------------------------------------------------------------------------
// Host-side launchers: launch_plan_w_LV / launch_window_w_LV's grids (plan_layout.h), decisions and fix-up pass.  The form
// follows the arguments: indexed exactly when vindex is set.
// ------------------------------------------------------------------------------------------
template <typename E, int L, int VEC, bool INDEXED>
hipError_t launch_plan_wh_LV(const WHPlanArgs& ha, hipStream_t stream) {
  if ((ha.vindex != nullptr) != INDEXED) return hipErrorInvalidValue;  // each translation unit builds one form
  WHPlanArgs hb = ha;
  PlanArgs& b = hb.w.p;
  b.fused = 0;
  const int n_col_panels = plan_launch_layout(b, L, VEC, DenseV<VEC>::mid, TinyT<L>::value, own_tiny_launch(b.n_tiny, 0), 0);
  const long long dense_wgs = ((long long)b.n_dense * b.n_panels + kWaves - 1) / kWaves;
  const long long grid = (long long)b.sparse_wgs + dense_wgs;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (grid > 0)
    hipLaunchKernelGGL((hybrid_plan_wh_kernel<E, L, VEC, HCSPMM_SPARSE_U, HCSPMM_MIN_WAVES_PER_SIMD, INDEXED>),
                       dim3((unsigned)grid), dim3(kThreads), 0, stream, hb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (b.tiny_kernel_wgs > 0) {
    hipLaunchKernelGGL((tiny_wh_kernel<E, L, VEC, INDEXED>), dim3((unsigned)(b.tiny_kernel_wgs * n_col_panels)), dim3(kThreads), 0,
                       stream, hb);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (b.n_split_rows > 0) {  // partial sums of split rows: the binary fix-up pass (it reads no values)
    const int fg = (b.n_split_rows + kWaves - 1) / kWaves;
    hipLaunchKernelGGL((fixup_kernel<E, VEC>), dim3(fg), dim3(kThreads), 0, stream, b);
    e = hipGetLastError();
  }
  return e;
}

template <typename E, int L, int VEC, bool INDEXED>
hipError_t launch_window_wh_LV(const WHWindowArgs& ha, hipStream_t stream) {
  if ((ha.vindex != nullptr) != INDEXED) return hipErrorInvalidValue;
  const WindowArgs& a = ha.w.w;
  const int W = (a.N + 15) / 16;
  const int n_panels = (a.D + 16 * VEC - 1) / (16 * VEC);
  int waves = (16 * L + 63) / 64;
  if (n_panels > waves) waves = n_panels;
  if (waves > kWaves) waves = kWaves;
  if (W > 0) hipLaunchKernelGGL((hybrid_window_wh_kernel<E, L, VEC, INDEXED>), dim3(W), dim3(waves * 64), 0, stream, ha);
  return hipGetLastError();
}

}  // namespace
}  // namespace hcspmm
