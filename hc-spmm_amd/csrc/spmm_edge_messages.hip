// spmm_edge_messages.hip -- edge-feature messages (hcspmm_forward_edge_messages), fp32 on the binary
// product's plan: a neighbour's row combined with a feature VECTOR of the edge,
//   Z[r][d] = sum over the entries e of row r of m(X[col(e)][d], F[fi(e)][d]),  fi(e) = findex ? findex[e] : e
//   mul: fmaf(f, x, acc)    add_relu: acc + ((x + f) < 0 ? +0 : x + f)    copy: acc + f (X is not read)
//
// The schedule is csr_schedule.h's, then the fix-up pass over split rows.
//  * Every entry issues two 16-byte loads per lane, the X row through col[e] and the F row through fi(e), both through the
//    element-aligned lanes (Lane / lane_col), F in 64-bit addressing.  The lane that loads col[e] loads findex[e] behind it
//    (or takes e itself) and both travel to the gathering lanes through ds_bpermute; a lane past its task's end holds
//    fi = -1 and takes nothing.  HCSPMM_EDGE_U entries are in flight per lane (copy, one load per entry: HCSPMM_SPARSE_U).
//  * MFMA cannot take a per-column value: the rows of a dense-tile window are served from CSR by the sparse-row task body,
//    one lane group per row (spmm_extremum.hip does the same).
//  * Sums run in hcspmm_forward_weighted's order: CSR order on ordinary and tiny tasks, the wide tasks' xor-shuffle tree, fp32
//    partials of sliced and segmented rows added by the fix-up pass in fixup_kernel's order.  No atomics.
//  * Gradient with respect to X: this launch on A^T's graph with findex = entry_index_t (hcspmm.h).
#include "csr_schedule.h"

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
    if (d[t].y >= 0) e = d[t].x >= 0 ? ea.rowptr[d[t].x] : segment_entry(a, ea.rowptr, ea.segment_len, -(d[t].x + 1));
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

// what csr_schedule.h's walks call
template <int OP, int L, int VEC> struct EBody {
  const EdgeMsgArgs& ea;
  typedef EDst Dst;
  __device__ __forceinline__ Dst dst(int row, int slot) const { return task_dst(ea, row, slot); }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    etask<OP, L, VEC, WIDE>(ea, o.z, o.p, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    etiny<OP, L, VEC, ETinyT<L>::value>(ea, first, c0, cend, lane);
  }
};

// the planned kernel (csr_schedule.h)
template <int OP, int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void edge_messages_plan_kernel(EdgeMsgArgs ea) {
  csr_plan_walk<L, ETinyT<L>::value>(ea.p, ea.rowptr, EBody<OP, L, VEC>{ea});
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

// the plan-free kernel (csr_schedule.h)
template <int OP, int L, int VEC>
__global__ __launch_bounds__(kThreads) void edge_messages_window_kernel(EdgeMsgArgs ea) {
  csr_window_walk<L>(ea.p, ea.rowptr, EBody<OP, L, VEC>{ea});
}

template <int OP>
hipError_t launch_edge_messages_op(const EdgeMsgArgs& a, int vec, hipStream_t stream) {
  return csr_dispatch(a.p, vec, [&](auto lv) {
    constexpr int L = decltype(lv)::L, VEC = decltype(lv)::VEC;
    return csr_launch(a, L, ETinyT<L>::value, edge_messages_window_kernel<OP, L, VEC>,
                      edge_messages_plan_kernel<OP, L, VEC, HCSPMM_MIN_WAVES_PER_SIMD>, edge_messages_fixup_kernel<VEC>, stream);
  });
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
