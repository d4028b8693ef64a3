// spmm_multi.hip -- sum, sum of squares, max and min of each row's neighbours with both argmaxes, in ONE gather pass
// (hcspmm_forward_multi), fp32 on the binary product's plan:
//   Z_sum[r][d] = sum x_e    Z_sumsq[r][d] = sum fl(x_e * x_e)    Z_max / arg_max, Z_min / arg_min as spmm_extremum.hip
// over the entries e of row r, x_e = X[col(e)][d].  A PNA layer needs all four; as four launches each one gathers the same X
// lines again, and every one of them is bound by those gathers.
//
// The schedule is csr_schedule.h's: every row, a dense-tile window's included, is a sparse-row task; a fix-up pass over split
// rows follows.  The per-lane state is six vectors.
//  * sum and sumsq run in CSR order inside a lane group, through the fixed xor-shuffle tree on wide tasks and in slot order
//    (then the tree) in the fix-up: deterministic, no atomics.  The square is rounded before it is added (__fmul_rn: never
//    contracted into an fma), so a sequentially summed row has the bits of an fp32 scan.  A sum never holds -0: it starts at
//    +0, and in round-to-nearest only (-0) + (-0) gives -0.
//  * max and min keep extremum_common.h's (value, position) order -- min as max over the sign-flipped values -- which is total
//    on distinct positions, so the combine works on partial slots unchanged and gives a sequential scan's bits on any split.
//  * One build computes all four; which are stored is a run-time matter (a null output is skipped).  A partial slot always
//    holds all six arrays.
#include "csr_schedule.h"
#include "extremum_common.h"

namespace hcspmm {
namespace {

constexpr unsigned kSign = 0x80000000u;
// row gathers in flight per lane: the binary path's eight.  With the 24 state registers the 16-byte-lane builds take 89-97
// registers, no scratch, four or five waves per SIMD (DESIGN.md section 3.17 has the compiler's figures per build)
constexpr int kMultiU = HCSPMM_SPARSE_U;

// per-lane state of VEC columns: the two sums, the best value and entry of the max, the best NEGATED value and entry of the min
template <int VEC> struct MState {
  float s[VEC], q[VEC], xv[VEC], nv[VEC];
  int xp[VEC], np[VEC];
  __device__ __forceinline__ MState() {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      s[i] = q[i] = 0.0f;
      xv[i] = nv[i] = -__builtin_inff();
      xp[i] = np[i] = kNone;
    }
  }
  // the (value, position) pairs of a partial result: max as it is, min already negated
  __device__ __forceinline__ void take_pairs(float mx, int mxp, float mn, int mnp, int i) {
    if (xbeats(mx, mxp, xv[i], xp[i])) {
      xv[i] = mx;
      xp[i] = mxp;
    }
    if (xbeats(mn, mnp, nv[i], np[i])) {
      nv[i] = mn;
      np[i] = mnp;
    }
  }
  // one gathered element at entry e
  __device__ __forceinline__ void take(float v, int e, int i) {
    s[i] += v;
    q[i] += __fmul_rn(v, v);
    take_pairs(v, e, xflip(v, kSign), e, i);
  }
  // another partial result of the same row and column
  __device__ __forceinline__ void merge(float os, float oq, float mx, int mxp, float mn, int mnp, int i) {
    s[i] += os;
    q[i] += oq;
    take_pairs(mx, mxp, mn, mnp, i);
  }
};

template <int VEC> __device__ __forceinline__ typename AccT<VEC>::type mvec(const float (&a)[VEC]) {
  typename AccT<VEC>::type out;
#pragma unroll
  for (int i = 0; i < VEC; ++i) aset(out, i, a[i]);
  return out;
}
template <int VEC> __device__ __forceinline__ typename IntV<VEC>::type mivec(const int (&a)[VEC]) {
  typename IntV<VEC>::type out;
#pragma unroll
  for (int i = 0; i < VEC; ++i) iset(out, i, a[i]);
  return out;
}

// Result of a whole row (slot < 0, row >= 0) or of one partial slot (slot >= 0) at columns [c, c + VEC); row < 0 and
// slot < 0: a lane group without a task.  Rows without entries: +0 in the four values (the sums are +0 already), -1 in both args
template <int VEC> __device__ __forceinline__ void mstore(const MArgs& ma, int row, int slot, int c, const MState<VEC>& st) {
  typedef Lane<F32, VEC> Ln;
  if (slot >= 0) {
    float* p = ma.p.partial + (size_t)slot * (size_t)ma.p.D + c;
    Ln::store_partial(p, mvec<VEC>(st.s));
    Ln::store_partial(p + ma.area, mvec<VEC>(st.q));
    Ln::store_partial(p + 2 * ma.area, mvec<VEC>(st.xv));
    istore<VEC>(reinterpret_cast<int*>(p + 3 * ma.area), mivec<VEC>(st.xp));
    Ln::store_partial(p + 4 * ma.area, mvec<VEC>(st.nv));
    istore<VEC>(reinterpret_cast<int*>(p + 5 * ma.area), mivec<VEC>(st.np));
    return;
  }
  if (row < 0) return;
  const size_t zo = (size_t)row * ma.p.ldz + c, ao = (size_t)row * ma.ldarg + c;
  if (ma.zsum != nullptr) Ln::store(ma.zsum + zo, mvec<VEC>(st.s));
  if (ma.zsumsq != nullptr) Ln::store(ma.zsumsq + zo, mvec<VEC>(st.q));
  typename AccT<VEC>::type mx, mn;
  typename IntV<VEC>::type pmx, pmn;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    const bool none = st.xp[i] == kNone;  // (the min has no entry either)
    aset(mx, i, none ? 0.0f : st.xv[i]);
    aset(mn, i, none ? 0.0f : xflip(st.nv[i], kSign));
    iset(pmx, i, none ? -1 : st.xp[i]);
    iset(pmn, i, none ? -1 : st.np[i]);
  }
  if (ma.zmax != nullptr) Ln::store(ma.zmax + zo, mx);
  if (ma.zmin != nullptr) Ln::store(ma.zmin + zo, mn);
  if (ma.amax != nullptr) istore<VEC>(ma.amax + ao, pmx);
  if (ma.amin != nullptr) istore<VEC>(ma.amin + ao, pmn);
}

// One branch-free batch of UB row gathers (spmm_impl.h gather_batch): lanes past a task's end hold idx -1 and take nothing
template <int VEC, int UB>
__device__ __forceinline__ void mbatch(const MArgs& ma, int csafe, bool cok, int myidx, int src0, int ebase, MState<VEC>& st) {
  typedef Lane<F32, VEC> Ln;
  const float* X = reinterpret_cast<const float*>(ma.p.X);
  int idx[UB];
  typename Ln::raw_t v[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = __shfl(myidx, src0 + u, 64);
#pragma unroll
  for (int u = 0; u < UB; ++u) v[u] = Ln::load(X + (size_t)max(idx[u], 0) * ma.p.ldx + csafe);
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    if (cok && idx[u] >= 0) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) st.take(aget(v[u], i), ebase + u, i);
    }
  }
}

// sparse_task (spmm_impl.h) with the six-vector state: L lanes own the task = entries [e0, e0 + n); WIDE: the whole wave owns
// it and the 64/L lane-group results are combined by the fixed xor-shuffle tree
template <int L, int VEC, bool WIDE>
__device__ __forceinline__ void mtask(const MArgs& ma, int row, int slot, int e0, int n, int c0, int cend, int lane) {
  constexpr int U = (L < kMultiU) ? L : kMultiU;
  constexpr int STRIDE = WIDE ? 64 : L;
  const int* __restrict__ col = ma.p.col;
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
    MState<VEC> st;
    int next = pos < n ? col[e0 + pos] : -1;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      next = base + STRIDE + pos < n ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      const int cnt = min(L, nmax - base);
      const int ebase = e0 + base + (WIDE ? gbase : 0);
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
        if (left > U / 2) {
          mbatch<VEC, U>(ma, c, cok, myidx, gbase + j, ebase + j, st);
          j += U;
        } else if (U >= 4 && left > 1) {
          mbatch<VEC, (U >= 4 ? U / 2 : 1)>(ma, c, cok, myidx, gbase + j, ebase + j, st);
          j += U / 2;
        } else {
          mbatch<VEC, 1>(ma, c, cok, myidx, gbase + j, ebase + j, st);
          j += 1;
        }
      }
    }
    if (WIDE) {
#pragma unroll
      for (int off = L; off < 64; off <<= 1) {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
          st.merge(__shfl_xor(st.s[i], off, 64), __shfl_xor(st.q[i], off, 64), __shfl_xor(st.xv[i], off, 64),
                   __shfl_xor(st.xp[i], off, 64), __shfl_xor(st.nv[i], off, 64), __shfl_xor(st.np[i], off, 64), i);
      }
    }
    if (cok && (!WIDE || lane < L)) mstore<VEC>(ma, row, slot, c, st);
  }
}

// tiny_tasks (spmm_impl.h): T tasks of at most two entries per lane group, indices inline in the descriptor; the entry
// position comes from rowptr (a whole row) or the fix-up list (the last segment of a split row)
template <int L, int VEC, int T>
__device__ __forceinline__ void mtiny(const MArgs& ma, int first, int c0, int cend, int lane) {
  typedef Lane<F32, VEC> Ln;
  const PlanArgs& a = ma.p;
  const float* X = reinterpret_cast<const float*>(a.X);
  constexpr int R = 64 / L;
  const int g = lane / L, s = lane & (L - 1);
  const int4* tasks = reinterpret_cast<const int4*>(a.plan + a.off_tasks);
  int4 d[T];
  int e[T];
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
    if (d[t].y >= 0) e[t] = d[t].x >= 0 ? ma.rowptr[d[t].x] : segment_entry(a, ma.rowptr, ma.segment_len, -(d[t].x + 1));
  }
  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const bool cok = pbase + s * VEC < cend;
    const int c = cok ? lane_col<VEC>(pbase + s * VEC, cend) : 0;
    typename Ln::raw_t v0[T], v1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) v0[t] = v1[t] = Ln::zero();
    if (any1) {
#pragma unroll
      for (int t = 0; t < T; ++t) v0[t] = Ln::load(X + (size_t)max(d[t].y, 0) * a.ldx + c);
    }
    if (any2) {
#pragma unroll
      for (int t = 0; t < T; ++t) v1[t] = Ln::load(X + (size_t)max(d[t].w, 0) * a.ldx + c);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      MState<VEC> st;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        if (d[t].y >= 0) st.take(aget(v0[t], i), e[t], i);
        if (d[t].w >= 0) st.take(aget(v1[t], i), e[t] + 1, i);
      }
      if (cok && d[t].z >= 0) mstore<VEC>(ma, d[t].x, d[t].x >= 0 ? -1 : -(d[t].x + 1), c, st);
    }
  }
}

// what csr_schedule.h's walks call
template <int L, int VEC> struct MBody {
  const MArgs& ma;
  typedef RowSlot Dst;  // mstore finds the place
  __device__ __forceinline__ Dst dst(int row, int slot) const { return Dst{row, slot}; }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    mtask<L, VEC, WIDE>(ma, o.row, o.slot, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    mtiny<L, VEC, XTinyT<L>::value>(ma, first, c0, cend, lane);
  }
};

// Fix-up: the six results of a split row from its partial slots -- one wave per row, the 64/L lane groups taking every
// (64/L)-th slot in slot order and combined by the xor-shuffle tree (extremum_fixup_kernel's shape; two slots in flight per
// lane, twelve loads)
template <int VEC>
__global__ __launch_bounds__(kThreads) void multi_fixup_kernel(MArgs ma) {
  typedef Lane<F32, VEC> Ln;
  const PlanArgs& a = ma.p;
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
    const float* at = a.partial + (size_t)s0 * (size_t)a.D + c;
    MState<VEC> st;
    int s = g;
    for (; s + R < ns; s += 2 * R) {
      typename AccT<VEC>::type vs[2], vq[2], vx[2], vn[2];
      typename IntV<VEC>::type px[2], pn[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float* p = at + (size_t)(s + u * R) * (size_t)a.D;
        vs[u] = Ln::load_partial(p);
        vq[u] = Ln::load_partial(p + ma.area);
        vx[u] = Ln::load_partial(p + 2 * ma.area);
        px[u] = iload<VEC>(reinterpret_cast<const int*>(p + 3 * ma.area));
        vn[u] = Ln::load_partial(p + 4 * ma.area);
        pn[u] = iload<VEC>(reinterpret_cast<const int*>(p + 5 * ma.area));
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
          st.merge(aget(vs[u], i), aget(vq[u], i), aget(vx[u], i), iget(px[u], i), aget(vn[u], i), iget(pn[u], i), i);
      }
    }
    for (; s < ns; s += R) {
      const float* p = at + (size_t)s * (size_t)a.D;
      const typename AccT<VEC>::type vs = Ln::load_partial(p), vq = Ln::load_partial(p + ma.area),
                                     vx = Ln::load_partial(p + 2 * ma.area), vn = Ln::load_partial(p + 4 * ma.area);
      const typename IntV<VEC>::type px = iload<VEC>(reinterpret_cast<const int*>(p + 3 * ma.area)),
                                     pn = iload<VEC>(reinterpret_cast<const int*>(p + 5 * ma.area));
#pragma unroll
      for (int i = 0; i < VEC; ++i) st.merge(aget(vs, i), aget(vq, i), aget(vx, i), iget(px, i), aget(vn, i), iget(pn, i), i);
    }
    for (int off = L; off < 64; off <<= 1) {
#pragma unroll
      for (int i = 0; i < VEC; ++i)
        st.merge(__shfl_xor(st.s[i], off, 64), __shfl_xor(st.q[i], off, 64), __shfl_xor(st.xv[i], off, 64),
                 __shfl_xor(st.xp[i], off, 64), __shfl_xor(st.nv[i], off, 64), __shfl_xor(st.np[i], off, 64), i);
    }
    if (cok && g == 0) mstore<VEC>(ma, row, -1, c, st);
  }
}

constexpr int kMultiMinWaves = 4;  // 128 registers per lane

// the planned and the plan-free kernel (csr_schedule.h)
template <int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void multi_plan_kernel(MArgs ma) {
  csr_plan_walk<L, XTinyT<L>::value>(ma.p, ma.rowptr, MBody<L, VEC>{ma});
}
template <int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void multi_window_kernel(MArgs ma) {
  csr_window_walk<L>(ma.p, ma.rowptr, MBody<L, VEC>{ma});
}

}  // namespace

hipError_t launch_multi_f32(const MArgs& a, int vec, hipStream_t stream) {
  return csr_dispatch(a.p, vec, [&](auto lv) {
    constexpr int L = decltype(lv)::L, VEC = decltype(lv)::VEC;
    return csr_launch(a, L, XTinyT<L>::value, multi_window_kernel<L, VEC, kMultiMinWaves>, multi_plan_kernel<L, VEC, kMultiMinWaves>,
                      multi_fixup_kernel<VEC>, stream);
  });
}

}  // namespace hcspmm
