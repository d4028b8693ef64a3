// spmm_softmax.hip -- per-channel softmax aggregation of each row's neighbours in ONE gather pass (hcspmm_forward_softmax,
// DESIGN.md section 3.18), fp32 on the binary product's plan:
//   Z[r][d] = sum_e p_e x_e,  p_e = exp(s_e) / sum_e' exp(s_e'),  s_e = fl(beta[d] * x_e),  x_e = X[col(e)][d]
// over the entries e of row r (DeeperGCN's softmax aggregation: beta -> +-inf is max / min, beta = 0 the mean), with the
// statistics its backward needs: M = max_e s_e, L = sum_e exp(s_e - M) and Q = sum_e p_e fl(x_e * x_e).
//
// The schedule is spmm_multi.hip's, which is the hybrid launch's (spmm_impl.h): sliced | wide | ordinary | tiny regions per
// column panel, the dense-tile windows served from CSR by the sparse-row task body, a fix-up pass over split rows, and a
// plan-free window kernel.  Only the per-lane state differs: the online-softmax quadruple (m, l, a, q) per column,
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

// the 16 rows of a window from CSR, R = 64 / L at a time (dense-tile windows of the plan; every window plan-free)
template <int L, int VEC>
__device__ __forceinline__ void swindow_rows(const SArgs& sa, int window, int c0, int cend, int lane) {
  constexpr int R = 64 / L;
  const int g = lane / L;
  for (int rb = 0; rb < 16; rb += R) {
    const int r = window * 16 + rb + g;
    int e0 = 0, n = 0, row = -1;
    if (rb + g < 16 && r < sa.p.N) {
      e0 = sa.rowptr[r];
      n = sa.rowptr[r + 1] - e0;
      row = r;
    }
    stask<L, VEC, false>(sa, row, -1, e0, n, c0, cend, lane);
  }
}

// ------------------------------------------------------------------------------------------
// Planned kernel: multi_plan_kernel's decode (sliced | wide | ordinary | tiny per column panel, then one wave per
// (dense-tile window, column panel) serving the window's rows from CSR).  Tiny tasks always run in their region here.
// ------------------------------------------------------------------------------------------
template <int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void softmax_plan_kernel(SArgs sa) {
  const PlanArgs& a = sa.p;
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
      stask<L, VEC, true>(sa, t.x, t.w, __builtin_amdgcn_readfirstlane(t.y), __builtin_amdgcn_readfirstlane(t.z), c0, cend, lane);
    } else if (bf >= sparse_wgs_pp_ordinary_end(a)) {
      if (bf >= a.free_wgs_pp) return;
      constexpr int R = 64 / L;
      const int first = a.n_tasks - a.n_tiny + ((bf - sparse_wgs_pp_ordinary_end(a)) * kWaves + wave) * (R * XTinyT<L>::value);
      if (first >= a.n_tasks) return;
      stiny<L, VEC, XTinyT<L>::value>(sa, first, c0, cend, lane);
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
      int e0 = 0, n = 0, row = -1, slot = -1;
      if (tp != nullptr) {
        const int4 t = *tp;
        if (t.x >= 0) {  // (slice padding: row -1)
          e0 = t.y;
          n = t.z;
          row = t.x;
          slot = t.w;
        }
      }
      stask<L, VEC, false>(sa, row, slot, e0, n, c0, cend, lane);
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
    swindow_rows<L, VEC>(sa, window, c0, min(a.D, c0 + a.panel_cols), lane);
  }
}

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

// Plan-free kernel: one workgroup per 16-row window, every window (dense-tile or not) served from CSR: rows up to
// kPlanFreeWide entries by one lane group each, longer ones by whole waves (multi_window_kernel's shape)
template <int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void softmax_window_kernel(SArgs sa) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = (int)blockDim.x >> 6;
  const int r0 = (int)blockIdx.x * 16, r1 = min(r0 + 16, sa.p.N);
  constexpr int R = 64 / L;
  const int G = R * nwaves;
  const int gi = wave * R + lane / L;
  for (int rb = r0; rb < r1; rb += G) {
    const int r = rb + gi;
    int e0 = 0, n = 0, row = -1;
    if (r < r1) {
      e0 = sa.rowptr[r];
      n = sa.rowptr[r + 1] - e0;
      if (R == 1 || n <= kPlanFreeWide) row = r;
      else n = 0;  // left to the whole-wave pass below
    }
    stask<L, VEC, false>(sa, row, -1, e0, n, 0, sa.p.D, lane);
  }
  if (R > 1) {
    int k = 0;
    for (int r = r0; r < r1; ++r) {
      const int e0 = sa.rowptr[r];
      const int n = sa.rowptr[r + 1] - e0;
      if (n > kPlanFreeWide) {
        if (k % nwaves == wave) stask<L, VEC, true>(sa, r, -1, e0, n, 0, sa.p.D, lane);
        ++k;
      }
    }
  }
}

constexpr int kSoftMinWaves = 4;  // 128 registers per lane

template <int L, int VEC>
hipError_t launch_softmax_LV(const SArgs& sa, hipStream_t stream) {
  SArgs sb = sa;
  PlanArgs& b = sb.p;
  if (sa.p.plan == nullptr) {  // plan-free
    const int W = (b.N + 15) / 16;
    int waves = (16 * L + 63) / 64;
    if (waves > kWaves) waves = kWaves;
    if (W > 0) hipLaunchKernelGGL((softmax_window_kernel<L, VEC, kSoftMinWaves>), dim3(W), dim3(waves * 64), 0, stream, sb);
    return hipGetLastError();
  }
  b.fused = 0;
  // the shared layout (plan_layout.h), in the extremum form: no launch of their own for the tiny tasks, dense windows once
  // per column panel
  const int n_col_panels = plan_launch_layout(b, L, 0, 0, XTinyT<L>::value, false, 0);
  const long long dense_wgs = ((long long)b.n_dense * n_col_panels + kWaves - 1) / kWaves;
  const long long grid = (long long)b.sparse_wgs + dense_wgs;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (grid > 0)
    hipLaunchKernelGGL((softmax_plan_kernel<L, VEC, kSoftMinWaves>), dim3((unsigned)grid), dim3(kThreads), 0, stream, sb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || b.n_split_rows == 0) return e;
  const int fg = (b.n_split_rows + kWaves - 1) / kWaves;
  hipLaunchKernelGGL((softmax_fixup_kernel<VEC>), dim3(fg), dim3(kThreads), 0, stream, sb);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_softmax_f32(const SArgs& a, int vec, hipStream_t stream) {
  if (vec == 4) {
    switch (pick_L(a.p.plan != nullptr ? a.p.panel_cols : a.p.D, 4)) {
      case 4: return launch_softmax_LV<4, 4>(a, stream);
      case 8: return launch_softmax_LV<8, 4>(a, stream);
      case 16: return launch_softmax_LV<16, 4>(a, stream);
      case 32: return launch_softmax_LV<32, 4>(a, stream);
      default: return launch_softmax_LV<64, 4>(a, stream);
    }
  }
  if (a.p.D > 4 * vec) return hipErrorInvalidValue;
  if (vec == 2) return launch_softmax_LV<4, 2>(a, stream);
  return launch_softmax_LV<4, 1>(a, stream);
}

}  // namespace hcspmm
