// spmm_gate16.hip -- gated neighbour aggregation on fp16 / bf16 operands (the 16-bit dtypes of the typed gated entry point,
// DESIGN.md section 3.21b).  P, Q and V hold 16-bit elements, both outputs are fp32.  For entry e = (r, c) of row r:
//   p, q, v = widen(P[r][d]), widen(Q[c][d]), widen(V[c][d])    (exact)        z = fl32(p + q)
//   Z_gate [r][d] = sum over e of sigma (z) * v               Z_dgate[r][d] = sum over e of sigma'(z) * v
// After the widening the arithmetic is the fp32 unit's, operation for operation (section 3.21): t = exp2(fl(-|z| log2e)),
// r = rcp(1 + t), sigma = z >= 0 ? r : fl(t r), sigma' = fl(fl(t r) r), fma accumulation from +0 -- so gates saturate exactly from
// |z| = 104 on, NaN propagates, rows without entries give +0, and wherever the summation order is the fp32 launch's the bits are.
//
// Lanes.  Rows sit on the dword grid (even width, even strides, 4-byte aligned bases), so a lane owns 8 columns (4 below 32
// columns) and an entry costs it two 16-byte (8-byte) loads at lane_col-moved-back positions: half the gathered bytes of the fp32
// unit per column.  The loaded dwords stay RAW in the in-flight arrays (4 registers per 16-byte load, not 8) and are widened pair
// by pair where they are used: a bf16 pair by a shift and a mask, an fp16 pair by one conversion per half.  kGate16U = 4 entries =
// eight loads are in flight per lane, the fp32 unit's count: 32 raw registers next to the 16 accumulators and 8 own-row floats of
// the widest build, inside the 128 registers of four waves per SIMD (table in DESIGN.md).
// The own row of P is loaded and widened once per task and column chunk (a lane group without a task reads nothing); a tiny task
// that carries a partial slot finds its row through the fix-up list.  Which outputs exist is a template argument (OUT: 1 = gate,
// 2 = dgate, 3 = both); the single-output builds never name the second accumulator.
// Schedule and order: csr_schedule.h's walks; CSR order on ordinary, tiny and window rows, the xor-shuffle tree on wide tasks,
// fp32 partial slots of split rows added by the binary fix-up pass at the fp32 output's lanes, once per output.  No atomics.
#include "csr_schedule.h"

namespace hcspmm {
namespace {

constexpr int kGate16U = 4;  // entries in flight per lane: eight loads
constexpr float kLog2e = 1.44269504088896340736f;
constexpr int kGate = 1, kDgate = 2;
constexpr int kGate16MinWaves = 4;  // 128 registers per lane

// the two 16-bit elements of a dword, widened (exact)
template <typename E> __device__ __forceinline__ void widen_pair(unsigned w, float& lo, float& hi);
template <> __device__ __forceinline__ void widen_pair<BF16>(unsigned w, float& lo, float& hi) {
  lo = __uint_as_float(w << 16);
  hi = __uint_as_float(w & 0xffff0000u);
}
template <> __device__ __forceinline__ void widen_pair<F16>(unsigned w, float& lo, float& hi) {
  lo = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
  hi = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
}

// the two sums of VEC columns; `b` is touched by the two-output builds only
template <int VEC> struct G16Sum {
  typename AccT<VEC>::type a = azero<VEC>(), b = azero<VEC>();
};

// the task's own row of P at columns [c, c + VEC), widened once; a lane group without a task (row < 0) reads nothing
template <typename E, int VEC>
__device__ __forceinline__ typename AccT<VEC>::type gate16_own(const Gate16Args& ga, int row, int c) {
  typename AccT<VEC>::type p = azero<VEC>();
  if (row >= 0) {
    const typename Lane<E, VEC>::raw_t raw = Lane<E, VEC>::load(ga.P + (size_t)row * ga.ldp + c);
#pragma unroll
    for (int w = 0; w < VEC / 2; ++w) {
      float lo, hi;
      widen_pair<E>(rword(raw, w), lo, hi);
      aset(p, 2 * w, lo);
      aset(p, 2 * w + 1, hi);
    }
  }
  return p;
}

// one column of one entry: the fp32 unit's gate, operation for operation
template <int OUT> __device__ __forceinline__ void gate16_column(float p, float qv, float v, float& a, float& b) {
  const float z = __fadd_rn(p, qv);
  const float t = __builtin_amdgcn_exp2f(__fmul_rn(-__builtin_fabsf(z), kLog2e));
  const float r = __builtin_amdgcn_rcpf(__fadd_rn(1.0f, t));
  const float tr = __fmul_rn(t, r);
  if (OUT == kGate || OUT == (kGate | kDgate)) a = __builtin_fmaf(z >= 0.0f ? r : tr, v, a);
  if (OUT == kDgate) a = __builtin_fmaf(__fmul_rn(tr, r), v, a);
  if (OUT == (kGate | kDgate)) b = __builtin_fmaf(__fmul_rn(tr, r), v, b);
}

// one entry: VEC columns of the gathered Q and V rows as loaded, widened a dword at a time
template <typename E, int VEC, int OUT>
__device__ __forceinline__ void gate16_step(G16Sum<VEC>& acc, const typename AccT<VEC>::type& p,
                                            const typename Lane<E, VEC>::raw_t& qr, const typename Lane<E, VEC>::raw_t& vr) {
#pragma unroll
  for (int w = 0; w < VEC / 2; ++w) {
    float q2[2], v2[2];
    widen_pair<E>(rword(qr, w), q2[0], q2[1]);
    widen_pair<E>(rword(vr, w), v2[0], v2[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = 2 * w + h;
      float a = aget(acc.a, q), b = 0.f;
      if (OUT == (kGate | kDgate)) b = aget(acc.b, q);
      gate16_column<OUT>(aget(p, q), q2[h], v2[h], a, b);
      aset(acc.a, q, a);
      if (OUT == (kGate | kDgate)) aset(acc.b, q, b);
    }
  }
}

// combine with another lane group's sums of the same columns
template <int VEC, int OUT> __device__ __forceinline__ void gate16_fold(G16Sum<VEC>& acc, int off) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    aset(acc.a, q, aget(acc.a, q) + __shfl_xor(aget(acc.a, q), off, 64));
    if (OUT == (kGate | kDgate)) aset(acc.b, q, aget(acc.b, q) + __shfl_xor(aget(acc.b, q), off, 64));
  }
}

// Result of a whole row (slot < 0, row >= 0) or of one partial slot (slot >= 0) at columns [c, c + VEC), fp32 either way; row < 0
// and slot < 0: a lane group without a task.  The first (or only) output is p.Z / p.partial, the second one z2 / the next area
template <int VEC, int OUT>
__device__ __forceinline__ void gate16_store(const Gate16Args& ga, int row, int slot, int c, const G16Sum<VEC>& acc) {
  typedef Lane<F32, VEC> Ln;
  if (slot >= 0) {
    float* p = ga.p.partial + (size_t)slot * (size_t)ga.p.D + c;
    Ln::store_partial(p, acc.a);
    if (OUT == (kGate | kDgate)) Ln::store_partial(p + ga.area, acc.b);
    return;
  }
  if (row < 0) return;
  const size_t zo = (size_t)row * ga.p.ldz + c;
  Ln::store(reinterpret_cast<float*>(ga.p.Z) + zo, acc.a);
  if (OUT == (kGate | kDgate)) Ln::store(ga.z2 + zo, acc.b);
}

// One branch-free batch of UB entries: 2 UB loads back to back, kept raw; lanes past a task's end hold idx -1, re-read row 0 and
// take nothing
template <typename E, int VEC, int OUT, int UB>
__device__ __forceinline__ void gate16_batch(const Gate16Args& ga, int csafe, bool cok, int myidx, int src0,
                                             const typename AccT<VEC>::type& p, G16Sum<VEC>& acc) {
  typedef Lane<E, VEC> Ln;
  int idx[UB];
  typename Ln::raw_t qr[UB], vr[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = __shfl(myidx, src0 + u, 64);
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const size_t r = (size_t)max(idx[u], 0);
    qr[u] = Ln::load(ga.Q + r * ga.ldq + csafe);
    vr[u] = Ln::load(ga.V + r * ga.ldv + csafe);
  }
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && idx[u] >= 0) gate16_step<E, VEC, OUT>(acc, p, qr[u], vr[u]);
}

// L lanes own the task = entries [e0, e0 + n) of row `row` (< 0: a lane group without a task); WIDE: the whole wave owns it and
// the 64/L lane-group sums are combined by the fixed tree
template <typename E, int L, int VEC, int OUT, bool WIDE>
__device__ __forceinline__ void gate16_task(const Gate16Args& ga, int row, int slot, int e0, int n, int c0, int cend, int lane) {
  constexpr int U = (L < kGate16U) ? L : kGate16U;
  constexpr int STRIDE = WIDE ? 64 : L;
  const int* __restrict__ col = ga.p.col;
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
    const typename AccT<VEC>::type p = gate16_own<E, VEC>(ga, row, c);
    G16Sum<VEC> acc;
    int next = pos < n ? col[e0 + pos] : -1;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      next = base + STRIDE + pos < n ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      const int cnt = min(L, nmax - base);
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
        if (left > U / 2) {
          gate16_batch<E, VEC, OUT, U>(ga, c, cok, myidx, gbase + j, p, acc);
          j += U;
        } else if (U >= 4 && left > 1) {
          gate16_batch<E, VEC, OUT, (U >= 4 ? U / 2 : 1)>(ga, c, cok, myidx, gbase + j, p, acc);
          j += U / 2;
        } else {
          gate16_batch<E, VEC, OUT, 1>(ga, c, cok, myidx, gbase + j, p, acc);
          j += 1;
        }
      }
    }
    if (WIDE) {
#pragma unroll
      for (int off = L; off < 64; off <<= 1) gate16_fold<VEC, OUT>(acc, off);
    }
    if (cok && (!WIDE || lane < L)) gate16_store<VEC, OUT>(ga, row, slot, c, acc);
  }
}

// one task of at most two entries per lane group (four loads), column ids inline in the descriptor; the own row comes from the
// descriptor (a whole row) or the fix-up list (the last segment of a split row)
template <typename E, int L, int VEC, int OUT>
__device__ __forceinline__ void gate16_tiny(const Gate16Args& ga, int first, int c0, int cend, int lane) {
  typedef Lane<E, VEC> Ln;
  typedef typename Ln::raw_t raw_t;
  const PlanArgs& a = ga.p;
  const int g = lane / L, s = lane & (L - 1);
  const int tid = first + g;
  const int4 d = (tid < a.n_tasks) ? reinterpret_cast<const int4*>(a.plan + a.off_tasks)[tid] : int4{0, -1, -1, -1};
  const bool any1 = __builtin_amdgcn_ballot_w64(d.y >= 0) != 0, any2 = __builtin_amdgcn_ballot_w64(d.w >= 0) != 0;
  int row = -1;
  if (d.z >= 0) row = d.x >= 0 ? d.x : fixup_of_slot(a, -(d.x + 1)).x;
  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const bool cok = pbase + s * VEC < cend;
    const int c = cok ? lane_col<VEC>(pbase + s * VEC, cend) : 0;
    const typename AccT<VEC>::type p = gate16_own<E, VEC>(ga, row, c);
    raw_t q0 = Ln::zero(), v0 = q0, q1 = q0, v1 = q0;
    if (any1) {
      const size_t r = (size_t)max(d.y, 0);
      q0 = Ln::load(ga.Q + r * ga.ldq + c);
      v0 = Ln::load(ga.V + r * ga.ldv + c);
    }
    if (any2) {
      const size_t r = (size_t)max(d.w, 0);
      q1 = Ln::load(ga.Q + r * ga.ldq + c);
      v1 = Ln::load(ga.V + r * ga.ldv + c);
    }
    G16Sum<VEC> acc;
    if (d.y >= 0) gate16_step<E, VEC, OUT>(acc, p, q0, v0);
    if (d.w >= 0) gate16_step<E, VEC, OUT>(acc, p, q1, v1);
    if (cok && d.z >= 0) gate16_store<VEC, OUT>(ga, d.x, d.x >= 0 ? -1 : -(d.x + 1), c, acc);
  }
}

// what csr_schedule.h's walks call: one tiny task per lane group
template <typename E, int L, int VEC, int OUT> struct Gate16Body {
  const Gate16Args& ga;
  typedef RowSlot Dst;  // the task body reads the task's own row of P as well; gate16_store finds the place
  __device__ __forceinline__ Dst dst(int row, int slot) const { return Dst{row, slot}; }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    gate16_task<E, L, VEC, OUT, WIDE>(ga, o.row, o.slot, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    gate16_tiny<E, L, VEC, OUT>(ga, first, c0, cend, lane);
  }
};

// the planned and the plan-free kernel (csr_schedule.h)
template <typename E, int OUT, int L, int VEC>
__global__ __launch_bounds__(kThreads, kGate16MinWaves) void gate16_plan_kernel(Gate16Args ga) {
  csr_plan_walk<L, 1>(ga.p, ga.rowptr, Gate16Body<E, L, VEC, OUT>{ga});
}
template <typename E, int OUT, int L, int VEC>
__global__ __launch_bounds__(kThreads, kGate16MinWaves) void gate16_window_kernel(Gate16Args ga) {
  csr_window_walk<L>(ga.p, ga.rowptr, Gate16Body<E, L, VEC, OUT>{ga});
}

// the outputs are fp32 at any width served (D >= 4): the fix-up pass is the binary one at four floats per lane, once per output
template <typename E, int OUT, int L, int VEC> hipError_t gate16_launch(const Gate16Args& a, hipStream_t stream) {
  const hipError_t e = csr_launch(a, L, 1, gate16_window_kernel<E, OUT, L, VEC>, gate16_plan_kernel<E, OUT, L, VEC>,
                                  fixup_kernel<F32, 4>, stream);
  if (OUT != (kGate | kDgate) || e != hipSuccess || a.p.plan == nullptr || a.p.n_split_rows == 0) return e;
  PlanArgs p = a.p;
  p.Z = a.z2;
  p.partial = a.p.partial + a.area;
  hipLaunchKernelGGL((fixup_kernel<F32, 4>), dim3((p.n_split_rows + kWaves - 1) / kWaves), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}

template <typename E, int L, int VEC> hipError_t gate16_outputs(const Gate16Args& a, hipStream_t stream) {
  switch (a.outputs) {
    case kGate: return gate16_launch<E, kGate, L, VEC>(a, stream);
    case kDgate: return gate16_launch<E, kDgate, L, VEC>(a, stream);
    case kGate | kDgate: return gate16_launch<E, kGate | kDgate, L, VEC>(a, stream);
    default: return hipErrorInvalidValue;
  }
}

// The unit's own dispatch (csr_dispatch serves 4-element lanes and narrower): 8 elements per lane with L = pick_L of the panel
// (planned) or of D (plan-free), 4 elements per lane with L = 4 or 8 below 32 columns
template <typename E> hipError_t gate16_dispatch(const Gate16Args& a, int vec, hipStream_t stream) {
  const int width = a.p.plan != nullptr ? a.p.panel_cols : a.p.D;
  if (a.p.D < 4 || (a.p.D & 1)) return hipErrorInvalidValue;
  if (vec == 8) {
    switch (pick_L(width, 8)) {
      case 4: return gate16_outputs<E, 4, 8>(a, stream);
      case 8: return gate16_outputs<E, 8, 8>(a, stream);
      case 16: return gate16_outputs<E, 16, 8>(a, stream);
      case 32: return gate16_outputs<E, 32, 8>(a, stream);
      default: return gate16_outputs<E, 64, 8>(a, stream);
    }
  }
  if (vec != 4 || a.p.D >= 32) return hipErrorInvalidValue;
  return pick_L(width, 4) == 4 ? gate16_outputs<E, 4, 4>(a, stream) : gate16_outputs<E, 8, 4>(a, stream);
}

}  // namespace

hipError_t launch_gate16(const Gate16Args& a, int dtype, int vec, hipStream_t stream) {
  if (dtype == HCSPMM_DTYPE_F16) return gate16_dispatch<F16>(a, vec, stream);
  if (dtype == HCSPMM_DTYPE_BF16) return gate16_dispatch<BF16>(a, vec, stream);
  return hipErrorInvalidValue;
}

}  // namespace hcspmm
