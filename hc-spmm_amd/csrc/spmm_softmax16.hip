// spmm_softmax16.hip -- per-channel softmax aggregation on fp16 / bf16 features in ONE gather pass (hcspmm_forward_softmax_typed,
// DESIGN.md section 3.18b).  With x_e = widen(X[col(e)][d]) (exact) and s_e = fl32(beta[d] * x_e) over the entries e of row r:
//   Z[r][d]   = rne16(zf),  zf = sum_e p_e x_e,  p_e = exp(s_e) / sum_e' exp(s_e')        (16-bit, rounded once)
//   LSE[r][d] = fl32(m + ln l),  m = max_e s_e,  l = sum_e exp(s_e - m)                   (fp32, nullable)
//   Var[r][d] = fl32(fl32(q / l) - fl32(zf zf)),  q = sum_e exp(s_e - m) fl32(x_e x_e)    (fp32, nullable, from the UNROUNDED zf)
// One statistic where the fp32 unit stores two: the backward needs exp(s - m) / l = exp(s - LSE) only.  Var is what the gradient
// of beta multiplies: Q - Z^2 cancels badly once Z has 8 or 11 significant bits, so the difference is taken here.
//
// State.  The fp32 unit's online quadruple (m, l, a, q) per column and its arithmetic, operation for operation (spmm_softmax.hip:
// one exponential per gathered element, never a positive argument; the merge rule with the NaN-to-0 guard; the wide tasks'
// xor-shuffle tree) -- copied, not shared, so that unit stays as it is.  Whether q EXISTS is a template argument (WQ): a build
// without Var has no q registers, no square and no fma for it -- 24 state registers per lane instead of 32 at 8 columns.
// Lanes.  Rows sit on the dword grid (even width, even strides, 4-byte aligned bases): a lane owns 8 columns -- one 16-byte load
// per gathered row -- from 32 columns per panel on and 4 columns (8-byte loads) below, a lane whose columns would run past a
// ragged end moved back onto the last ones (lane_col; its duplicate stores carry the same bits).  Eight loads are in flight per
// lane; they stay RAW dwords (4 registers per 16-byte load) and a dword is widened where it is used, both halves at once.  beta is
// loaded once per lane and column chunk.
// Split rows keep the fp32 unit's workspace: four fp32 areas (m, l, a, q; a build without Var leaves the fourth untouched), merged
// in slot order and then by the tree in the unit's own fix-up kernel, which stores 16-bit Z and fp32 LSE / Var.
// Schedule: csr_schedule.h's walks; tiny tasks XTinyT<L> per lane group, as the fp32 unit.  Deterministic, no atomics.
#include "csr_schedule.h"
#include "extremum_common.h"  // XTinyT

namespace hcspmm {
namespace {

constexpr int kSoft16MinWaves = 4;  // 128 registers per lane
constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.693147180559945309417f;

// the two 16-bit elements of a dword, widened (exact)
template <typename E> __device__ __forceinline__ void s16_widen(unsigned w, float& lo, float& hi);
template <> __device__ __forceinline__ void s16_widen<BF16>(unsigned w, float& lo, float& hi) {
  lo = __uint_as_float(w << 16);
  hi = __uint_as_float(w & 0xffff0000u);
}
template <> __device__ __forceinline__ void s16_widen<F16>(unsigned w, float& lo, float& hi) {
  lo = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
  hi = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
}

// exp(-|d|) for d finite or +-inf, one v_exp_f32: never a positive argument, exp2(0) = 1 and exp2(-inf) = 0 exactly
__device__ __forceinline__ float s16_exp_neg_abs(float d) { return __builtin_amdgcn_exp2f(-__builtin_fabsf(d) * kLog2e); }

// SState (spmm_softmax.hip) with q optional: a build with WQ = false never names it
template <int VEC, bool WQ> struct S16State {
  float m[VEC], l[VEC], a[VEC], q[WQ ? VEC : 1];
  __device__ __forceinline__ S16State() {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      m[i] = -__builtin_inff();
      l[i] = a[i] = 0.0f;
      if constexpr (WQ) q[i] = 0.0f;
    }
  }
  __device__ __forceinline__ float qat(int i) const {
    if constexpr (WQ) return q[i];
    else return 0.0f;
  }
  // the state (om, ol, oa, oq) joins this one; d = om - m[i], not NaN
  __device__ __forceinline__ void combine(float d, float om, float ol, float oa, float oq, int i) {
    const float t = s16_exp_neg_abs(d);
    const bool up = d > 0.0f;
    const float mine = up ? t : 1.0f, theirs = up ? 1.0f : t;
    l[i] = __builtin_fmaf(l[i], mine, ol * theirs);
    a[i] = __builtin_fmaf(a[i], mine, oa * theirs);
    if constexpr (WQ) q[i] = __builtin_fmaf(q[i], mine, oq * theirs);
    m[i] = up ? om : m[i];
  }
  // one gathered element x of a column with coefficient b
  __device__ __forceinline__ void take(float x, float b, int i) {
    const float s = __fmul_rn(b, x);
    float xx = 0.0f;
    if constexpr (WQ) xx = __fmul_rn(x, x);
    combine(__fsub_rn(s, m[i]), s, 1.0f, x, xx, i);
  }
  // another partial state of the same row and column; either side may be empty
  __device__ __forceinline__ void merge(float om, float ol, float oa, float oq, int i) {
    const float d = __fsub_rn(om, m[i]);
    combine(d != d ? 0.0f : d, om, ol, oa, oq, i);
  }
};

// VEC floats of a state array to / from fp32 memory, four at a time (the slots and the statistics are fp32 whatever the lanes are)
template <int VEC> __device__ __forceinline__ void s16_put(float* p, const float (&v)[VEC], bool partial) {
#pragma unroll
  for (int h = 0; h < VEC; h += 4) {
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = v[h + i];
    if (partial) Lane<F32, 4>::store_partial(p + h, o);
    else Lane<F32, 4>::store(p + h, o);
  }
}
template <int VEC> __device__ __forceinline__ void s16_get(const float* p, float (&v)[VEC]) {
#pragma unroll
  for (int h = 0; h < VEC; h += 4) {
    const f32x4 o = Lane<F32, 4>::load(p + h);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[h + i] = o[i];
  }
}

// Result of a whole row (slot < 0, row >= 0): 16-bit Z, fp32 LSE / Var; or of one partial slot (slot >= 0): the raw state arrays;
// row < 0 and slot < 0: a lane group without a task.  Rows without entries: Z = +0, LSE = -inf, Var = +0
template <typename E, int VEC, bool WQ>
__device__ __forceinline__ void s16_store(const S16Args& sa, int row, int slot, int c, const S16State<VEC, WQ>& st) {
  if (slot >= 0) {
    float* p = sa.p.partial + (size_t)slot * (size_t)sa.p.D + c;
    s16_put<VEC>(p, st.m, true);
    s16_put<VEC>(p + sa.area, st.l, true);
    s16_put<VEC>(p + 2 * sa.area, st.a, true);
    if constexpr (WQ) s16_put<VEC>(p + 3 * sa.area, st.q, true);
    return;
  }
  if (row < 0) return;
  float zf[VEC];
  typename AccT<VEC>::type z;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    zf[i] = st.l[i] > 0.0f ? st.a[i] / st.l[i] : 0.0f;
    aset(z, i, zf[i]);
  }
  Lane<E, VEC>::store(reinterpret_cast<unsigned short*>(sa.p.Z) + (size_t)row * sa.p.ldz + c, z);  // one rounding per element
  const size_t so = (size_t)row * sa.ld_stat + c;
  if (sa.lse != nullptr) {
    float o[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i)
      o[i] = st.l[i] > 0.0f ? __fadd_rn(st.m[i], __fmul_rn(__builtin_amdgcn_logf(st.l[i]), kLn2)) : -__builtin_inff();
    s16_put<VEC>(sa.lse + so, o, false);
  }
  if constexpr (WQ) {
    float o[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = st.l[i] > 0.0f ? __fsub_rn(st.q[i] / st.l[i], __fmul_rn(zf[i], zf[i])) : 0.0f;
    s16_put<VEC>(sa.var + so, o, false);
  }
}

// one gathered row as loaded: VEC columns, a dword at a time
template <typename E, int VEC, bool WQ>
__device__ __forceinline__ void s16_step(S16State<VEC, WQ>& st, const typename Lane<E, VEC>::raw_t& r, const float (&beta)[VEC]) {
#pragma unroll
  for (int w = 0; w < VEC / 2; ++w) {
    float lo, hi;
    s16_widen<E>(rword(r, w), lo, hi);
    st.take(lo, beta[2 * w], 2 * w);
    st.take(hi, beta[2 * w + 1], 2 * w + 1);
  }
}

// One branch-free batch of UB row gathers, kept raw: lanes past a task's end hold idx -1, re-read row 0 and take nothing
template <typename E, int VEC, bool WQ, int UB>
__device__ __forceinline__ void s16_batch(const S16Args& sa, int csafe, bool cok, int myidx, int src0, const float (&beta)[VEC],
                                          S16State<VEC, WQ>& st) {
  typedef Lane<E, VEC> Ln;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(sa.p.X);
  int idx[UB];
  typename Ln::raw_t v[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = __shfl(myidx, src0 + u, 64);
#pragma unroll
  for (int u = 0; u < UB; ++u) v[u] = Ln::load(X + (size_t)max(idx[u], 0) * sa.p.ldx + csafe);
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && idx[u] >= 0) s16_step<E, VEC, WQ>(st, v[u], beta);
}

// At most four columns' shuffles of a tree level in flight, the fp32 unit's count.  Left alone, all 32 shuffles of a level are
// issued above the merges and the builds with q spill (12 ... 64 bytes per lane).  The shuffle inputs of columns 4 ... 7 pass
// through an empty statement that also reads the merged columns 0 ... 3, so they cannot be issued before those merges; no
// instruction is emitted
template <bool WQ> __device__ __forceinline__ void s16_after(S16State<8, WQ>& st) {
  asm volatile("" : "+v"(st.m[4]), "+v"(st.m[5]), "+v"(st.m[6]), "+v"(st.m[7]), "+v"(st.l[4]), "+v"(st.l[5]), "+v"(st.l[6]),
                    "+v"(st.l[7]), "+v"(st.a[4]), "+v"(st.a[5]), "+v"(st.a[6]), "+v"(st.a[7])
               : "v"(st.l[0]), "v"(st.l[1]), "v"(st.l[2]), "v"(st.l[3]));
  if constexpr (WQ)
    asm volatile("" : "+v"(st.q[4]), "+v"(st.q[5]), "+v"(st.q[6]), "+v"(st.q[7]) : "v"(st.l[0]), "v"(st.l[1]), "v"(st.l[2]), "v"(st.l[3]));
}

// the 64/L lane-group states of a wave into every group (the group-0 lanes store), by the fixed xor-shuffle tree
template <int VEC, bool WQ> __device__ __forceinline__ void s16_tree(S16State<VEC, WQ>& st, int L) {
  for (int off = L; off < 64; off <<= 1) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      float oq = 0.0f;
      if constexpr (WQ) oq = __shfl_xor(st.q[i], off, 64);
      st.merge(__shfl_xor(st.m[i], off, 64), __shfl_xor(st.l[i], off, 64), __shfl_xor(st.a[i], off, 64), oq, i);
      if constexpr (VEC > 4) {
        if (i == 3) s16_after(st);
      }
    }
  }
}

// L lanes own the task = entries [e0, e0 + n) (row < 0 and slot < 0: a lane group without a task); WIDE: the whole wave owns it and
// the 64/L lane-group states are merged by the tree
template <typename E, int L, int VEC, bool WQ, bool WIDE>
__device__ __forceinline__ void s16_task(const S16Args& sa, int row, int slot, int e0, int n, int c0, int cend, int lane) {
  constexpr int U = (L < HCSPMM_SPARSE_U) ? L : HCSPMM_SPARSE_U;
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
    float beta[VEC];
    s16_get<VEC>(sa.beta + c, beta);  // once per lane and column chunk
    S16State<VEC, WQ> st;
    int next = pos < n ? col[e0 + pos] : -1;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      next = base + STRIDE + pos < n ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      const int cnt = min(L, nmax - base);
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
        if (left > U / 2) {
          s16_batch<E, VEC, WQ, U>(sa, c, cok, myidx, gbase + j, beta, st);
          j += U;
        } else if (U >= 4 && left > 1) {
          s16_batch<E, VEC, WQ, (U >= 4 ? U / 2 : 1)>(sa, c, cok, myidx, gbase + j, beta, st);
          j += U / 2;
        } else {
          s16_batch<E, VEC, WQ, 1>(sa, c, cok, myidx, gbase + j, beta, st);
          j += 1;
        }
      }
    }
    if (WIDE) s16_tree<VEC, WQ>(st, L);
    if (cok && (!WIDE || lane < L)) s16_store<E, VEC, WQ>(sa, row, slot, c, st);
  }
}

// T tasks of at most two entries per lane group, column ids inline in the descriptor: 2 T raw loads in flight
template <typename E, int L, int VEC, bool WQ, int T>
__device__ __forceinline__ void s16_tiny(const S16Args& sa, int first, int c0, int cend, int lane) {
  typedef Lane<E, VEC> Ln;
  const PlanArgs& a = sa.p;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(a.X);
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
    float beta[VEC];
    s16_get<VEC>(sa.beta + c, beta);
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
      S16State<VEC, WQ> st;
      if (d[t].y >= 0) s16_step<E, VEC, WQ>(st, v0[t], beta);
      if (d[t].w >= 0) s16_step<E, VEC, WQ>(st, v1[t], beta);
      if (cok && d[t].z >= 0) s16_store<E, VEC, WQ>(sa, d[t].x, d[t].x >= 0 ? -1 : -(d[t].x + 1), c, st);
    }
  }
}

// what csr_schedule.h's walks call
template <typename E, int L, int VEC, bool WQ> struct S16Body {
  const S16Args& sa;
  typedef RowSlot Dst;  // s16_store finds the place
  __device__ __forceinline__ Dst dst(int row, int slot) const { return Dst{row, slot}; }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    s16_task<E, L, VEC, WQ, WIDE>(sa, o.row, o.slot, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    s16_tiny<E, L, VEC, WQ, XTinyT<L>::value>(sa, first, c0, cend, lane);
  }
};

// the planned and the plan-free kernel (csr_schedule.h)
template <typename E, int L, int VEC, bool WQ>
__global__ __launch_bounds__(kThreads, kSoft16MinWaves) void softmax16_plan_kernel(S16Args sa) {
  csr_plan_walk<L, XTinyT<L>::value>(sa.p, sa.rowptr, S16Body<E, L, VEC, WQ>{sa});
}
template <typename E, int L, int VEC, bool WQ>
__global__ __launch_bounds__(kThreads, kSoft16MinWaves) void softmax16_window_kernel(S16Args sa) {
  csr_window_walk<L>(sa.p, sa.rowptr, S16Body<E, L, VEC, WQ>{sa});
}

// Fix-up: the state of a split row from its partial slots -- one wave per row at four columns per lane (the slots are fp32 whatever
// the panel's lanes were), the 64/L lane groups taking every (64/L)-th slot in slot order, two slots in flight per lane (six or
// eight loads), merged by the xor-shuffle tree; the result is stored as 16-bit Z and fp32 LSE / Var
template <typename E, bool WQ>
__global__ __launch_bounds__(kThreads) void softmax16_fixup_kernel(S16Args sa) {
  constexpr int VEC = 4;
  typedef Lane<F32, VEC> Ln;
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
    S16State<VEC, WQ> st;
    int s = g;
    for (; s + R < ns; s += 2 * R) {
      f32x4 vm[2], vl[2], va[2], vq[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float* p = at + (size_t)(s + u * R) * (size_t)a.D;
        vm[u] = Ln::load_partial(p);
        vl[u] = Ln::load_partial(p + sa.area);
        va[u] = Ln::load_partial(p + 2 * sa.area);
        if constexpr (WQ) vq[u] = Ln::load_partial(p + 3 * sa.area);
        else vq[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) st.merge(vm[u][i], vl[u][i], va[u][i], vq[u][i], i);
      }
    }
    for (; s < ns; s += R) {
      const float* p = at + (size_t)s * (size_t)a.D;
      const f32x4 vm = Ln::load_partial(p), vl = Ln::load_partial(p + sa.area), va = Ln::load_partial(p + 2 * sa.area);
      f32x4 vq = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (WQ) vq = Ln::load_partial(p + 3 * sa.area);
#pragma unroll
      for (int i = 0; i < VEC; ++i) st.merge(vm[i], vl[i], va[i], vq[i], i);
    }
    s16_tree<VEC, WQ>(st, L);
    if (cok && g == 0) s16_store<E, VEC, WQ>(sa, row, -1, c, st);
  }
}

template <typename E, int L, int VEC> hipError_t s16_launch(const S16Args& a, hipStream_t stream) {
  if (a.var != nullptr)
    return csr_launch(a, L, XTinyT<L>::value, softmax16_window_kernel<E, L, VEC, true>, softmax16_plan_kernel<E, L, VEC, true>,
                      softmax16_fixup_kernel<E, true>, stream);
  return csr_launch(a, L, XTinyT<L>::value, softmax16_window_kernel<E, L, VEC, false>, softmax16_plan_kernel<E, L, VEC, false>,
                    softmax16_fixup_kernel<E, false>, stream);
}

// The unit's own dispatch (csr_dispatch serves 4-element lanes and narrower): 8 elements per lane and L = pick_L of the panel
// (planned) or of D (plan-free) from 32 columns on, 4 elements per lane with L = 4 or 8 below
template <typename E> hipError_t s16_dispatch(const S16Args& a, hipStream_t stream) {
  const int width = a.p.plan != nullptr ? a.p.panel_cols : a.p.D;
  if (a.p.D < 4 || width < 4 || ((a.p.D | width) & 1)) return hipErrorInvalidValue;
  if (width >= 32) {
    switch (pick_L(width, 8)) {
      case 4: return s16_launch<E, 4, 8>(a, stream);
      case 8: return s16_launch<E, 8, 8>(a, stream);
      case 16: return s16_launch<E, 16, 8>(a, stream);
      case 32: return s16_launch<E, 32, 8>(a, stream);
      default: return s16_launch<E, 64, 8>(a, stream);
    }
  }
  return pick_L(width, 4) == 4 ? s16_launch<E, 4, 4>(a, stream) : s16_launch<E, 8, 4>(a, stream);
}

}  // namespace

hipError_t launch_softmax16(const S16Args& a, int dtype, hipStream_t stream) {
  if (dtype == HCSPMM_DTYPE_F16) return s16_dispatch<F16>(a, stream);
  if (dtype == HCSPMM_DTYPE_BF16) return s16_dispatch<BF16>(a, stream);
  return hipErrorInvalidValue;
}

}  // namespace hcspmm
