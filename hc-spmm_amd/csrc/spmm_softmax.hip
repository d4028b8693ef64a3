// spmm_softmax.hip -- per-channel softmax aggregation of each row's neighbours in ONE gather pass (hcspmm_forward_softmax,
// DESIGN.md section 3.18), fp32 on the binary product's plan:
//   Z[r][d] = sum_e p_e x_e,  p_e = exp(s_e) / sum_e' exp(s_e'),  s_e = fl(beta[d] * x_e),  x_e = X[col(e)][d]
// over the entries e of row r (DeeperGCN's softmax aggregation: beta -> +-inf is max / min, beta = 0 the mean), with the
// statistics its backward needs: M = max_e s_e, L = sum_e exp(s_e - M) and Q = sum_e p_e fl(x_e * x_e).
//
// The schedule is csr_schedule.h's: every row, a dense-tile window's included, is a sparse-row task; a fix-up pass over split
// rows follows.  The per-lane state is the online-softmax quadruple (m, l, a, q) per column,
//   m = running max of s,  l = sum exp(s - m),  a = sum exp(s - m) x,  q = sum exp(s - m) fl(x x).
//  * ONE exponential per gathered element: with d = s - m and t = exp(-|d|), a new maximum (d > 0) rescales the state by t and
//    adds the element with weight 1; otherwise the element is added with weight t.  The exponent never sees a positive
//    argument, so any finite beta * x is safe; a state that took no entry is (m = -inf, l = a = q = 0), and its first entry
//    has d = +inf, t = 0.
//  * Two partial states of a row and column (the wide tasks' xor-shuffle tree, the fix-up's slots) merge by the same rule
//    with d = m2 - m1; d = NaN (-inf - -inf: both sides empty) is replaced by 0 BEFORE the exponential, so an empty side
//    leaves the other one unchanged and no NaN is made.
//  * Order: CSR order inside a lane group, the fixed tree on wide tasks, slot order (then the tree) in the fix-up:
//    deterministic, no atomics.  s is a rounded product (__fmul_rn: never contracted into the subtraction), so M is bit for
//    bit the maximum of fl(beta x); the square is rounded before it is weighted.
//  * One build computes all four; which of M, L, Q are stored is a run-time matter (a null output is skipped).  A partial
//    slot always holds the four raw state arrays.
#include "csr_schedule.h"
#include "extremum_common.h"

namespace hcspmm {
namespace {

// row gathers in flight per lane: the binary path's eight
constexpr int kSoftU = HCSPMM_SPARSE_U;
constexpr float kLog2e = 1.44269504088896340736f;

// exp(-|d|) for d finite or +-inf, one v_exp_f32: never a positive argument, exp2(0) = 1 and exp2(-inf) = 0 exactly
__device__ __forceinline__ float exp_neg_abs(float d) { return __builtin_amdgcn_exp2f(-__builtin_fabsf(d) * kLog2e); }

template <int VEC> struct SState {
  float m[VEC], l[VEC], a[VEC], q[VEC];
  __device__ __forceinline__ SState() {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      m[i] = -__builtin_inff();
      l[i] = a[i] = q[i] = 0.0f;
    }
  }
  // the state (om, ol, oa, oq) joins this one; d = om - m[i], not NaN
  __device__ __forceinline__ void combine(float d, float om, float ol, float oa, float oq, int i) {
    const float t = exp_neg_abs(d);
    const bool up = d > 0.0f;
    const float mine = up ? t : 1.0f, theirs = up ? 1.0f : t;
    l[i] = __builtin_fmaf(l[i], mine, ol * theirs);
    a[i] = __builtin_fmaf(a[i], mine, oa * theirs);
    q[i] = __builtin_fmaf(q[i], mine, oq * theirs);
    m[i] = up ? om : m[i];
  }
  // one gathered element x of a column with coefficient b
  __device__ __forceinline__ void take(float x, float b, int i) {
    const float s = __fmul_rn(b, x);
    combine(__fsub_rn(s, m[i]), s, 1.0f, x, __fmul_rn(x, x), i);
  }
  // another partial state of the same row and column; either side may be empty
  __device__ __forceinline__ void merge(float om, float ol, float oa, float oq, int i) {
    const float d = __fsub_rn(om, m[i]);
    combine(d != d ? 0.0f : d, om, ol, oa, oq, i);
  }
};

template <int VEC> __device__ __forceinline__ typename AccT<VEC>::type svec(const float (&a)[VEC]) {
  typename AccT<VEC>::type out;
#pragma unroll
  for (int i = 0; i < VEC; ++i) aset(out, i, a[i]);
  return out;
}

// Result of a whole row (slot < 0, row >= 0) or of one partial slot (slot >= 0) at columns [c, c + VEC); row < 0 and
// slot < 0: a lane group without a task.  Rows without entries: Z = Q = +0, M = -inf, L = 0
template <int VEC> __device__ __forceinline__ void sstore(const SArgs& sa, int row, int slot, int c, const SState<VEC>& st) {
  typedef Lane<F32, VEC> Ln;
  if (slot >= 0) {
    float* p = sa.p.partial + (size_t)slot * (size_t)sa.p.D + c;
    Ln::store_partial(p, svec<VEC>(st.m));
    Ln::store_partial(p + sa.area, svec<VEC>(st.l));
    Ln::store_partial(p + 2 * sa.area, svec<VEC>(st.a));
    Ln::store_partial(p + 3 * sa.area, svec<VEC>(st.q));
    return;
  }
  if (row < 0) return;
  const size_t zo = (size_t)row * sa.p.ldz + c;
  typename AccT<VEC>::type z;
#pragma unroll
  for (int i = 0; i < VEC; ++i) aset(z, i, st.l[i] > 0.0f ? st.a[i] / st.l[i] : 0.0f);
  Ln::store(sa.z + zo, z);
  if (sa.m != nullptr) Ln::store(sa.m + zo, svec<VEC>(st.m));
  if (sa.l != nullptr) Ln::store(sa.l + zo, svec<VEC>(st.l));
  if (sa.q != nullptr) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) aset(z, i, st.l[i] > 0.0f ? st.q[i] / st.l[i] : 0.0f);
    Ln::store(sa.q + zo, z);
  }
}

// One branch-free batch of UB row gathers (spmm_impl.h gather_batch): lanes past a task's end hold idx -1 and take nothing
template <int VEC, int UB>
__device__ __forceinline__ void sbatch(const SArgs& sa, int csafe, bool cok, int myidx, int src0,
                                       const typename AccT<VEC>::type& beta, SState<VEC>& st) {
  typedef Lane<F32, VEC> Ln;
  const float* X = reinterpret_cast<const float*>(sa.p.X);
  int idx[UB];
  typename Ln::raw_t v[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = __shfl(myidx, src0 + u, 64);
#pragma unroll
  for (int u = 0; u < UB; ++u) v[u] = Ln::load(X + (size_t)max(idx[u], 0) * sa.p.ldx + csafe);
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    if (cok && idx[u] >= 0) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) st.take(aget(v[u], i), aget(beta, i), i);
    }
  }
}

// the 64/L lane-group states of a wave into every group (the group-0 lanes store), by the fixed xor-shuffle tree
template <int VEC> __device__ __forceinline__ void stree(SState<VEC>& st, int L) {
  for (int off = L; off < 64; off <<= 1) {
#pragma unroll
    for (int i = 0; i < VEC; ++i)
      st.merge(__shfl_xor(st.m[i], off, 64), __shfl_xor(st.l[i], off, 64), __shfl_xor(st.a[i], off, 64),
               __shfl_xor(st.q[i], off, 64), i);
  }
}

// sparse_task (spmm_impl.h) with the softmax state: L lanes own the task = entries [e0, e0 + n); WIDE: the whole wave owns
// it and the 64/L lane-group states are merged by the tree
template <int L, int VEC, bool WIDE>
__device__ __forceinline__ void stask(const SArgs& sa, int row, int slot, int e0, int n, int c0, int cend, int lane) {
  typedef Lane<F32, VEC> Ln;
  constexpr int U = (L < kSoftU) ? L : kSoftU;
  constexpr int STRIDE = WIDE ? 64 : L;
  const int* __restrict__ col = sa.p.col;
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
    const typename AccT<VEC>::type beta = Ln::load(sa.beta + c);  // once per lane and column chunk
    SState<VEC> st;
    int next = pos < n ? col[e0 + pos] : -1;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      next = base + STRIDE + pos < n ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      const int cnt = min(L, nmax - base);
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
        if (left > U / 2) {
          sbatch<VEC, U>(sa, c, cok, myidx, gbase + j, beta, st);
          j += U;
        } else if (U >= 4 && left > 1) {
          sbatch<VEC, (U >= 4 ? U / 2 : 1)>(sa, c, cok, myidx, gbase + j, beta, st);
          j += U / 2;
        } else {
          sbatch<VEC, 1>(sa, c, cok, myidx, gbase + j, beta, st);
          j += 1;
        }
      }
    }
    if (WIDE) stree<VEC>(st, L);
    if (cok && (!WIDE || lane < L)) sstore<VEC>(sa, row, slot, c, st);
  }
}

// tiny_tasks (spmm_impl.h): T tasks of at most two entries per lane group, indices inline in the descriptor
template <int L, int VEC, int T>
__device__ __forceinline__ void stiny(const SArgs& sa, int first, int c0, int cend, int lane) {
  typedef Lane<F32, VEC> Ln;
  const PlanArgs& a = sa.p;
  const float* X = reinterpret_cast<const float*>(a.X);
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
  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const bool cok = pbase + s * VEC < cend;
    const int c = cok ? lane_col<VEC>(pbase + s * VEC, cend) : 0;
    const typename AccT<VEC>::type beta = Ln::load(sa.beta + c);
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
      SState<VEC> st;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        if (d[t].y >= 0) st.take(aget(v0[t], i), aget(beta, i), i);
        if (d[t].w >= 0) st.take(aget(v1[t], i), aget(beta, i), i);
      }
      if (cok && d[t].z >= 0) sstore<VEC>(sa, d[t].x, d[t].x >= 0 ? -1 : -(d[t].x + 1), c, st);
    }
  }
}

// what csr_schedule.h's walks call
template <int L, int VEC> struct SBody {
  const SArgs& sa;
  typedef RowSlot Dst;  // sstore finds the place
  __device__ __forceinline__ Dst dst(int row, int slot) const { return Dst{row, slot}; }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    stask<L, VEC, WIDE>(sa, o.row, o.slot, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    stiny<L, VEC, XTinyT<L>::value>(sa, first, c0, cend, lane);
  }
};

// Fix-up: the state of a split row from its partial slots -- one wave per row, the 64/L lane groups taking every (64/L)-th
// slot in slot order and merged by the xor-shuffle tree (multi_fixup_kernel's shape; two slots in flight per lane, eight
// loads)
template <int VEC>
__global__ __launch_bounds__(kThreads) void softmax_fixup_kernel(SArgs sa) {
  typedef Lane<F32, VEC> Ln;
  typedef typename AccT<VEC>::type acc_t;
  const PlanArgs& a = sa.p;
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
    SState<VEC> st;
    int s = g;
    for (; s + R < ns; s += 2 * R) {
      acc_t vm[2], vl[2], va[2], vq[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float* p = at + (size_t)(s + u * R) * (size_t)a.D;
        vm[u] = Ln::load_partial(p);
        vl[u] = Ln::load_partial(p + sa.area);
        va[u] = Ln::load_partial(p + 2 * sa.area);
        vq[u] = Ln::load_partial(p + 3 * sa.area);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) st.merge(aget(vm[u], i), aget(vl[u], i), aget(va[u], i), aget(vq[u], i), i);
      }
    }
    for (; s < ns; s += R) {
      const float* p = at + (size_t)s * (size_t)a.D;
      const acc_t vm = Ln::load_partial(p), vl = Ln::load_partial(p + sa.area), va = Ln::load_partial(p + 2 * sa.area),
                  vq = Ln::load_partial(p + 3 * sa.area);
#pragma unroll
      for (int i = 0; i < VEC; ++i) st.merge(aget(vm, i), aget(vl, i), aget(va, i), aget(vq, i), i);
    }
    stree<VEC>(st, L);
    if (cok && g == 0) sstore<VEC>(sa, row, -1, c, st);
  }
}

constexpr int kSoftMinWaves = 4;  // 128 registers per lane

// the planned and the plan-free kernel (csr_schedule.h)
template <int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void softmax_plan_kernel(SArgs sa) {
  csr_plan_walk<L, XTinyT<L>::value>(sa.p, sa.rowptr, SBody<L, VEC>{sa});
}
template <int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void softmax_window_kernel(SArgs sa) {
  csr_window_walk<L>(sa.p, sa.rowptr, SBody<L, VEC>{sa});
}

}  // namespace

hipError_t launch_softmax_f32(const SArgs& a, int vec, hipStream_t stream) {
  return csr_dispatch(a.p, vec, [&](auto lv) {
    constexpr int L = decltype(lv)::L, VEC = decltype(lv)::VEC;
    return csr_launch(a, L, XTinyT<L>::value, softmax_window_kernel<L, VEC, kSoftMinWaves>, softmax_plan_kernel<L, VEC, kSoftMinWaves>,
                      softmax_fixup_kernel<VEC>, stream);
  });
}

}  // namespace hcspmm
