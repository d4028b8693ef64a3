// spmm_extremum.hip -- max / min neighbour aggregation with its argmax, and the backward of it (hcspmm_forward_extremum*,
// DESIGN.md section 3.12), fp32 on the binary product's plan:
//   forward   Z[r][d] = max (min) over the entries e of row r of X[col(e)][d],  arg[r][d] = the winning e
//   backward  grad_X[j][d] = sum of grad_Z[i][d] over the entries e = (i, j) with arg[i][d] == e
//
// The schedule is csr_schedule.h's, then a fix-up pass over split rows.
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
#include "csr_schedule.h"
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
    if (d[t].y >= 0) e[t] = d[t].x >= 0 ? xa.rowptr[d[t].x] : segment_entry(a, xa.rowptr, xa.segment_len, -(d[t].x + 1));
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

// what csr_schedule.h's walks call
template <int L, int VEC, bool BWD> struct XBody {
  const XArgs& xa;
  typedef XDst Dst;
  __device__ __forceinline__ Dst dst(int row, int slot) const { return task_dst(xa, row, slot); }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    xtask<L, VEC, WIDE, BWD>(xa, o.z, o.a, o.p, o.pp, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    xtiny<L, VEC, XTinyT<L>::value, BWD>(xa, first, c0, cend, lane);
  }
};

// the planned kernel (csr_schedule.h)
template <int L, int VEC, bool BWD, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void extremum_plan_kernel(XArgs xa) {
  csr_plan_walk<L, XTinyT<L>::value>(xa.p, xa.rowptr, XBody<L, VEC, BWD>{xa});
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

// the plan-free kernel (csr_schedule.h)
template <int L, int VEC, bool BWD>
__global__ __launch_bounds__(kThreads) void extremum_window_kernel(XArgs xa) {
  csr_window_walk<L>(xa.p, xa.rowptr, XBody<L, VEC, BWD>{xa});
}

template <bool BWD>
hipError_t launch_extremum_any(const XArgs& a, int vec, hipStream_t stream) {
  return csr_dispatch(a.p, vec, [&](auto lv) {
    constexpr int L = decltype(lv)::L, VEC = decltype(lv)::VEC;
    constexpr auto window = extremum_window_kernel<L, VEC, BWD>;
    constexpr auto plan = extremum_plan_kernel<L, VEC, BWD, HCSPMM_MIN_WAVES_PER_SIMD>;
    if constexpr (BWD) return csr_launch(a, L, XTinyT<L>::value, window, plan, fixup_kernel<F32, VEC>, stream);  // fp32 sums: the binary pass
    else return csr_launch(a, L, XTinyT<L>::value, window, plan, extremum_fixup_kernel<VEC>, stream);
  });
}

}  // namespace

hipError_t launch_extremum_f32(const XArgs& a, int vec, hipStream_t stream) { return launch_extremum_any<false>(a, vec, stream); }
hipError_t launch_extremum_backward_f32(const XArgs& a, int vec, hipStream_t stream) {
  return launch_extremum_any<true>(a, vec, stream);
}

}  // namespace hcspmm
