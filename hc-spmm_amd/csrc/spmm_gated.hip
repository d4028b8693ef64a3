// spmm_gated.hip -- gated neighbour aggregation (hcspmm_forward_gated), fp32 on the binary product's
// plan.  For entry e = (r, c) of row r and z = fl(P[r][d] + Q[c][d]) (one fp32 add, never contracted):
//   Z_gate [r][d] = sum over e of sigma (z) * V[c][d]      sigma (z) = 1 / (1 + exp(-z))
//   Z_dgate[r][d] = sum over e of sigma'(z) * V[c][d]      sigma'(z) = sigma(z) (1 - sigma(z))
// The message depends on the DESTINATION row as well as on the gathered one: no [E, D] gate tensor is built.
//
// A plain-sum sparse-row launch on csr_schedule.h's schedule (every row, a dense-tile window's included, is a sparse-row
// task), with fixup_kernel's pass over split rows, once per output.
//  * The gate never takes an exponential of a positive argument: t = exp(-|z|), r = 1 / (1 + t), sigma = z >= 0 ? r : t r,
//    sigma' = t r r.  Where t underflows to 0 (|z| >= 104) r is exactly 1: sigma is exactly 1 (z > 0) or 0 (z < 0) and sigma'
//    exactly 0.  A NaN in z reaches every output (z >= 0 is false, t r is NaN); +-inf behaves as the limit.
//  * P is indexed by the task's OWN row: a per-lane constant of a column chunk, loaded once per task (a lane group without a
//    task reads nothing).  A tiny task that carries a partial slot instead of its row finds the row through the fix-up list.
//  * Q and V are indexed by column id: two 16-byte loads per entry and lane through the element-aligned lanes, kGatedU
//    entries in flight per lane.  P, Q, V have their own row strides.
//  * Which outputs exist is a template argument (OUT: 1 = gate, 2 = dgate, 3 = both): an absent output costs no register and
//    no store, and both sums of OUT = 3 come out of one gather pass.  Every build evaluates the gate with the same explicitly
//    rounded operations and adds with an explicit fma, so an output of a two-output call has the bits of the single-output call.
//  * Sums run in hcspmm_forward_weighted's order: CSR order on ordinary and tiny tasks, the wide tasks' xor-shuffle tree, fp32
//    partials of sliced and segmented rows added by the fix-up pass in fixup_kernel's order.  No atomics.  A sum starts at
//    +0 and never holds -0, so rows without entries, and columns whose gates all vanish, get +0.
#include "csr_schedule.h"

namespace hcspmm {
namespace {

constexpr int kGatedU = 4;  // entries in flight per lane: eight 16-byte loads, the binary gather's count
constexpr float kLog2e = 1.44269504088896340736f;
constexpr int kGate = 1, kDgate = 2;

// the two sums of VEC columns; `b` is touched by the two-output builds only (the others never name it: no register)
template <int VEC> struct GSum {
  typename AccT<VEC>::type a = azero<VEC>(), b = azero<VEC>();
};

// the task's own row of P at columns [c, c + VEC); a lane group without a task (row < 0) reads nothing
template <int VEC>
__device__ __forceinline__ typename AccT<VEC>::type gated_own(const GatedArgs& ga, int row, int c) {
  return row >= 0 ? Lane<F32, VEC>::load(ga.P + (size_t)row * ga.ldp + c) : azero<VEC>();
}

// one entry: VEC columns of the gathered Q and V rows
template <int VEC, int OUT>
__device__ __forceinline__ void gated_step(GSum<VEC>& acc, const typename AccT<VEC>::type& p, const typename AccT<VEC>::type& qv,
                                           const typename AccT<VEC>::type& v) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    const float z = __fadd_rn(aget(p, q), aget(qv, q));
    const float t = __builtin_amdgcn_exp2f(__fmul_rn(-__builtin_fabsf(z), kLog2e));
    const float r = __builtin_amdgcn_rcpf(__fadd_rn(1.0f, t));
    const float tr = __fmul_rn(t, r);
    if (OUT == kGate || OUT == (kGate | kDgate)) aset(acc.a, q, __builtin_fmaf(z >= 0.0f ? r : tr, aget(v, q), aget(acc.a, q)));
    if (OUT == kDgate) aset(acc.a, q, __builtin_fmaf(__fmul_rn(tr, r), aget(v, q), aget(acc.a, q)));
    if (OUT == (kGate | kDgate)) aset(acc.b, q, __builtin_fmaf(__fmul_rn(tr, r), aget(v, q), aget(acc.b, q)));
  }
}

// combine with another lane group's sums of the same columns
template <int VEC, int OUT> __device__ __forceinline__ void gated_fold(GSum<VEC>& acc, int off) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    aset(acc.a, q, aget(acc.a, q) + __shfl_xor(aget(acc.a, q), off, 64));
    if (OUT == (kGate | kDgate)) aset(acc.b, q, aget(acc.b, q) + __shfl_xor(aget(acc.b, q), off, 64));
  }
}

// Result of a whole row (slot < 0, row >= 0) or of one partial slot (slot >= 0) at columns [c, c + VEC); row < 0 and slot < 0: a
// lane group without a task.  The first (or only) output is p.Z / p.partial, the second one z2 / the next workspace area
template <int VEC, int OUT>
__device__ __forceinline__ void gated_store(const GatedArgs& ga, int row, int slot, int c, const GSum<VEC>& acc) {
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

// One branch-free batch of UB entries (spmm_impl.h gather_batch): lanes past a task's end hold idx -1, re-read row 0 and take
// nothing
template <int VEC, int OUT, int UB>
__device__ __forceinline__ void gated_batch(const GatedArgs& ga, int csafe, bool cok, int myidx, int src0,
                                            const typename AccT<VEC>::type& p, GSum<VEC>& acc) {
  typedef Lane<F32, VEC> Ln;
  int idx[UB];
  typename AccT<VEC>::type qv[UB], v[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = __shfl(myidx, src0 + u, 64);
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const size_t r = (size_t)max(idx[u], 0);
    qv[u] = Ln::load(ga.Q + r * ga.ldq + csafe);
    v[u] = Ln::load(ga.V + r * ga.ldv + csafe);
  }
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && idx[u] >= 0) gated_step<VEC, OUT>(acc, p, qv[u], v[u]);
}

// sparse_task_w (spmm_weighted_impl.h) with the gate step: L lanes own the task = entries [e0, e0 + n) of row `row` (< 0: a
// lane group without a task); WIDE: the whole wave owns it and the 64/L lane-group sums are combined by the fixed tree
template <int L, int VEC, int OUT, bool WIDE>
__device__ __forceinline__ void gated_task(const GatedArgs& ga, int row, int slot, int e0, int n, int c0, int cend, int lane) {
  constexpr int U = (L < kGatedU) ? L : kGatedU;
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
    const typename AccT<VEC>::type p = gated_own<VEC>(ga, row, c);
    GSum<VEC> acc;
    int next = pos < n ? col[e0 + pos] : -1;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      next = base + STRIDE + pos < n ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      const int cnt = min(L, nmax - base);
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
        if (left > U / 2) {
          gated_batch<VEC, OUT, U>(ga, c, cok, myidx, gbase + j, p, acc);
          j += U;
        } else if (U >= 4 && left > 1) {
          gated_batch<VEC, OUT, (U >= 4 ? U / 2 : 1)>(ga, c, cok, myidx, gbase + j, p, acc);
          j += U / 2;
        } else {
          gated_batch<VEC, OUT, 1>(ga, c, cok, myidx, gbase + j, p, acc);
          j += 1;
        }
      }
    }
    if (WIDE) {
#pragma unroll
      for (int off = L; off < 64; off <<= 1) gated_fold<VEC, OUT>(acc, off);
    }
    if (cok && (!WIDE || lane < L)) gated_store<VEC, OUT>(ga, row, slot, c, acc);
  }
}

// tiny_tasks_w (spmm_weighted_impl.h), one task of at most two entries per lane group (four loads), column ids inline in the
// descriptor; the own row comes from the descriptor (a whole row) or the fix-up list (the last segment of a split row)
template <int L, int VEC, int OUT>
__device__ __forceinline__ void gated_tiny(const GatedArgs& ga, int first, int c0, int cend, int lane) {
  typedef Lane<F32, VEC> Ln;
  typedef typename AccT<VEC>::type acc_t;
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
    const acc_t p = gated_own<VEC>(ga, row, c);
    acc_t q0 = azero<VEC>(), v0 = q0, q1 = q0, v1 = q0;
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
    GSum<VEC> acc;
    if (d.y >= 0) gated_step<VEC, OUT>(acc, p, q0, v0);
    if (d.w >= 0) gated_step<VEC, OUT>(acc, p, q1, v1);
    if (cok && d.z >= 0) gated_store<VEC, OUT>(ga, d.x, d.x >= 0 ? -1 : -(d.x + 1), c, acc);
  }
}

// what csr_schedule.h's walks call: one tiny task per lane group
template <int L, int VEC, int OUT> struct GatedBody {
  const GatedArgs& ga;
  typedef RowSlot Dst;  // gated_task reads the task's own row of P as well; gated_store finds the place
  __device__ __forceinline__ Dst dst(int row, int slot) const { return Dst{row, slot}; }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    gated_task<L, VEC, OUT, WIDE>(ga, o.row, o.slot, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    gated_tiny<L, VEC, OUT>(ga, first, c0, cend, lane);
  }
};

constexpr int kGatedMinWaves = 4;  // 128 registers per lane

// the planned and the plan-free kernel (csr_schedule.h)
template <int OUT, int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void gated_plan_kernel(GatedArgs ga) {
  csr_plan_walk<L, 1>(ga.p, ga.rowptr, GatedBody<L, VEC, OUT>{ga});
}
template <int OUT, int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void gated_window_kernel(GatedArgs ga) {
  csr_window_walk<L>(ga.p, ga.rowptr, GatedBody<L, VEC, OUT>{ga});
}

template <int OUT, int L, int VEC> hipError_t gated_launch(const GatedArgs& a, hipStream_t stream) {
  const hipError_t e = csr_launch(a, L, 1, gated_window_kernel<OUT, L, VEC, kGatedMinWaves>,
                                  gated_plan_kernel<OUT, L, VEC, kGatedMinWaves>, fixup_kernel<F32, VEC>, stream);  // fp32 sums: the binary pass
  if (OUT != (kGate | kDgate) || e != hipSuccess || a.p.plan == nullptr || a.p.n_split_rows == 0) return e;
  // ... and once more for the second output, from its own workspace area
  PlanArgs p = a.p;
  p.Z = a.z2;
  p.partial = a.p.partial + a.area;
  hipLaunchKernelGGL((fixup_kernel<F32, VEC>), dim3((p.n_split_rows + kWaves - 1) / kWaves), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_gated_f32(const GatedArgs& a, int vec, hipStream_t stream) {
  return csr_dispatch(a.p, vec, [&](auto lv) {
    constexpr int L = decltype(lv)::L, VEC = decltype(lv)::VEC;
    switch (a.outputs) {
      case kGate: return gated_launch<kGate, L, VEC>(a, stream);
      case kDgate: return gated_launch<kDgate, L, VEC>(a, stream);
      case kGate | kDgate: return gated_launch<kGate | kDgate, L, VEC>(a, stream);
      default: return hipErrorInvalidValue;
    }
  });
}

}  // namespace hcspmm
