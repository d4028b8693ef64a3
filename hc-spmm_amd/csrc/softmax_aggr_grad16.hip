// softmax_aggr_grad16.hip -- gradient of the 16-bit softmax aggregation with respect to X (hcspmm_softmax_backward_typed,
// DESIGN.md section 3.18b), on the plan of the graph the backward walks (A^T's, or A's own for a symmetric pattern):
//   dX[j][d] = sum over the entries (j, i) of row j of  exp(s_j - LSE[i][d]) * g_i * (1 + beta[d] (x_j - z_i)),
//   x_j = widen(X[j][d]), s_j = fl32(beta[d] * x_j), g_i = widen(G[i][d]), z_i = widen(Z[i][d])      (fp32 dX)
// The softmax weight of entry (i, j) of A is recomputed from the forward's log-sum-exp alone: exp(s - m) / l = exp(s - LSE), so one
// fp32 statistic is gathered where the fp32 unit gathers two, and no reciprocal is taken.  On the true transpose s_j <= LSE[i]
// (j is among row i's entries), so the exponent is <= 0.
//
// A plain-sum sparse-row launch on csr_schedule.h's schedule, with the binary fix-up pass (fixup_kernel<F32, 4>) over split rows.
//  * Rows of X, G and Z sit on the dword grid (even width, even strides, 4-byte aligned bases): a lane owns 8 columns from 32
//    columns per panel on and 4 below, moved back at a ragged end (lane_col).  Per entry a lane of 8 columns issues ONE 16-byte
//    load of G, ONE of Z and TWO of LSE: 8 gathered bytes per column against the fp32 unit's 16.  Two entries are in flight per
//    lane: eight loads, 32 raw registers; the 16-bit dwords are widened pair by pair where they are used.
//  * The task's own row (x, beta, s) is widened once per task and column chunk.  A tiny task that carries a partial slot instead
//    of its row finds the row through the fix-up list.
//  * Each step is p = exp2((s - lse) log2e), k = fma(beta, x - z, 1), acc = fma(p g, k, acc).
//  * Sums run in hcspmm_forward_weighted's order: CSR order on ordinary and tiny tasks, the wide tasks' xor-shuffle tree, fp32
//    partials of sliced and segmented rows added by the fix-up pass.  No atomics.
#include "csr_schedule.h"

namespace hcspmm {
namespace {

constexpr int kGrad16U = 2;  // entries in flight per lane: eight loads at 8 columns per lane
constexpr int kGrad16MinWaves = 4;  // 128 registers per lane
constexpr float kLog2e = 1.44269504088896340736f;

// the two 16-bit elements of a dword, widened (exact)
template <typename E> __device__ __forceinline__ void g16_widen(unsigned w, float& lo, float& hi);
template <> __device__ __forceinline__ void g16_widen<BF16>(unsigned w, float& lo, float& hi) {
  lo = __uint_as_float(w << 16);
  hi = __uint_as_float(w & 0xffff0000u);
}
template <> __device__ __forceinline__ void g16_widen<F16>(unsigned w, float& lo, float& hi) {
  lo = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
  hi = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
}

// per-lane constants of a column chunk: the task's own x (widened), beta and s = fl(beta x)
template <int VEC> struct G16Own {
  float x[VEC], b[VEC], s[VEC];
};

// a lane group without a task (row < 0) reads no row: x = 0
template <typename E, int VEC>
__device__ __forceinline__ G16Own<VEC> g16_own(const SGrad16Args& ga, int row, int c) {
  G16Own<VEC> o;
#pragma unroll
  for (int h = 0; h < VEC; h += 4) {
    const f32x4 b = Lane<F32, 4>::load(ga.beta + c + h);
#pragma unroll
    for (int q = 0; q < 4; ++q) o.b[h + q] = b[q];
  }
  typename Lane<E, VEC>::raw_t raw = Lane<E, VEC>::zero();
  if (row >= 0) raw = Lane<E, VEC>::load(reinterpret_cast<const unsigned short*>(ga.p.X) + (size_t)row * ga.p.ldx + c);
#pragma unroll
  for (int w = 0; w < VEC / 2; ++w) g16_widen<E>(rword(raw, w), o.x[2 * w], o.x[2 * w + 1]);
#pragma unroll
  for (int q = 0; q < VEC; ++q) o.s[q] = __fmul_rn(o.b[q], o.x[q]);
  return o;
}

// the gathered rows of one entry as loaded: VEC 16-bit elements of G and of Z, VEC floats of LSE
template <typename E, int VEC> struct G16In {
  typename Lane<E, VEC>::raw_t g, z;
  f32x4 lse[VEC / 4];
};

template <typename E, int VEC>
__device__ __forceinline__ G16In<E, VEC> g16_load(const SGrad16Args& ga, int idx, int c) {
  typedef Lane<E, VEC> Ln;
  G16In<E, VEC> in;
  const size_t r = (size_t)max(idx, 0);
  in.g = Ln::load(ga.G + r * ga.ld_in + c);
  in.z = Ln::load(ga.Zh + r * ga.ld_in + c);
#pragma unroll
  for (int h = 0; h < VEC / 4; ++h) in.lse[h] = Lane<F32, 4>::load(ga.LSE + r * ga.ld_stat + c + 4 * h);
  return in;
}

// one entry: VEC columns
template <typename E, int VEC>
__device__ __forceinline__ void g16_step(float (&acc)[VEC], const G16Own<VEC>& o, const G16In<E, VEC>& in) {
#pragma unroll
  for (int w = 0; w < VEC / 2; ++w) {
    float g2[2], z2[2];
    g16_widen<E>(rword(in.g, w), g2[0], g2[1]);
    g16_widen<E>(rword(in.z, w), z2[0], z2[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = 2 * w + h;
      const float p = __builtin_amdgcn_exp2f(__fsub_rn(o.s[q], in.lse[q >> 2][q & 3]) * kLog2e);
      const float k = __builtin_fmaf(o.b[q], __fsub_rn(o.x[q], z2[h]), 1.0f);
      acc[q] = __builtin_fmaf(p * g2[h], k, acc[q]);
    }
  }
}

// VEC fp32 sums to Z[row] (partial = false) or a partial slot, four at a time
template <int VEC> __device__ __forceinline__ void g16_put(float* p, const float (&acc)[VEC], bool partial) {
#pragma unroll
  for (int h = 0; h < VEC; h += 4) {
    f32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = acc[h + q];
    if (partial) Lane<F32, 4>::store_partial(p + h, o);
    else Lane<F32, 4>::store(p + h, o);
  }
}

// One branch-free batch of UB entries, 4 UB loads back to back: lanes past a task's end hold idx -1, re-read row 0 and take nothing
template <typename E, int VEC, int UB>
__device__ __forceinline__ void g16_batch(const SGrad16Args& ga, int csafe, bool cok, int myidx, int src0, const G16Own<VEC>& o,
                                          float (&acc)[VEC]) {
  int idx[UB];
  G16In<E, VEC> in[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = __shfl(myidx, src0 + u, 64);
#pragma unroll
  for (int u = 0; u < UB; ++u) in[u] = g16_load<E, VEC>(ga, idx[u], csafe);
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && idx[u] >= 0) g16_step<E, VEC>(acc, o, in[u]);
}

// destinations of a task descriptor (row | first entry | length | partial slot or -1)
struct G16Dst {
  int row = -1;  // the task's own row of X
  float* z = nullptr;
  float* p = nullptr;
};
__device__ __forceinline__ G16Dst g16_dst(const SGrad16Args& ga, int own, int row, int slot) {
  const PlanArgs& a = ga.p;
  G16Dst d;
  d.row = own;
  if (slot < 0) d.z = reinterpret_cast<float*>(a.Z) + (size_t)row * a.ldz;
  else d.p = a.partial + (size_t)slot * (size_t)a.D;
  return d;
}

// L lanes own the task = entries [e0, e0 + n) of row d.row (< 0: a lane group without a task); WIDE: the whole wave owns it and the
// 64/L lane-group sums are combined by the fixed tree
template <typename E, int L, int VEC, bool WIDE>
__device__ __forceinline__ void g16_task(const SGrad16Args& ga, const G16Dst& d, int e0, int n, int c0, int cend, int lane) {
  constexpr int U = (L < kGrad16U) ? L : kGrad16U;
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
    const G16Own<VEC> o = g16_own<E, VEC>(ga, d.row, c);
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    int next = pos < n ? col[e0 + pos] : -1;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      next = base + STRIDE + pos < n ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      const int cnt = min(L, nmax - base);
      for (int j = 0; j < cnt;) {
        if (U >= 2 && cnt - j > 1) {
          g16_batch<E, VEC, U>(ga, c, cok, myidx, gbase + j, o, acc);
          j += U;
        } else {
          g16_batch<E, VEC, 1>(ga, c, cok, myidx, gbase + j, o, acc);
          j += 1;
        }
      }
    }
    if (WIDE) {
#pragma unroll
      for (int off = L; off < 64; off <<= 1) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = acc[q] + __shfl_xor(acc[q], off, 64);
      }
    }
    if (cok && (!WIDE || lane < L)) {
      if (d.z != nullptr) g16_put<VEC>(d.z + c, acc, false);
      else if (d.p != nullptr) g16_put<VEC>(d.p + c, acc, true);
    }
  }
}

// one task of at most two entries per lane group (eight loads), column ids inline in the descriptor; the own row comes from the
// descriptor (a whole row) or the fix-up list (the last segment of a split row)
template <typename E, int L, int VEC>
__device__ __forceinline__ void g16_tiny(const SGrad16Args& ga, int first, int c0, int cend, int lane) {
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
    const G16Own<VEC> o = g16_own<E, VEC>(ga, row, c);
    G16In<E, VEC> in0{}, in1{};
    if (any1) in0 = g16_load<E, VEC>(ga, d.y, c);
    if (any2) in1 = g16_load<E, VEC>(ga, d.w, c);
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    if (d.y >= 0) g16_step<E, VEC>(acc, o, in0);
    if (d.w >= 0) g16_step<E, VEC>(acc, o, in1);
    if (cok && d.z >= 0) {
      if (d.x >= 0) g16_put<VEC>(reinterpret_cast<float*>(a.Z) + (size_t)d.x * a.ldz + c, acc, false);
      else g16_put<VEC>(a.partial + (size_t)(-(d.x + 1)) * (size_t)a.D + c, acc, true);
    }
  }
}

// what csr_schedule.h's walks call: one tiny task per lane group
template <typename E, int L, int VEC> struct G16Body {
  const SGrad16Args& ga;
  typedef G16Dst Dst;  // g16_task reads the task's own row of X as well
  __device__ __forceinline__ Dst dst(int row, int slot) const { return g16_dst(ga, row, row, slot); }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& d, int e0, int n, int c0, int cend, int lane) const {
    g16_task<E, L, VEC, WIDE>(ga, d, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const { g16_tiny<E, L, VEC>(ga, first, c0, cend, lane); }
};

// the planned and the plan-free kernel (csr_schedule.h)
template <typename E, int L, int VEC>
__global__ __launch_bounds__(kThreads, kGrad16MinWaves) void softmax_grad16_plan_kernel(SGrad16Args ga) {
  csr_plan_walk<L, 1>(ga.p, ga.rowptr, G16Body<E, L, VEC>{ga});
}
template <typename E, int L, int VEC>
__global__ __launch_bounds__(kThreads, kGrad16MinWaves) void softmax_grad16_window_kernel(SGrad16Args ga) {
  csr_window_walk<L>(ga.p, ga.rowptr, G16Body<E, L, VEC>{ga});
}

// dX is fp32 at any width served (D >= 4): the fix-up pass is the binary one at four floats per lane
template <typename E, int L, int VEC> hipError_t g16_launch(const SGrad16Args& a, hipStream_t stream) {
  return csr_launch(a, L, 1, softmax_grad16_window_kernel<E, L, VEC>, softmax_grad16_plan_kernel<E, L, VEC>, fixup_kernel<F32, 4>,
                    stream);
}

// The unit's own dispatch: 8 elements per lane and L = pick_L of the panel (planned) or of D (plan-free) from 32 columns on, 4
// elements per lane with L = 4 or 8 below
template <typename E> hipError_t g16_dispatch(const SGrad16Args& a, hipStream_t stream) {
  const int width = a.p.plan != nullptr ? a.p.panel_cols : a.p.D;
  if (a.p.D < 4 || width < 4 || ((a.p.D | width) & 1)) return hipErrorInvalidValue;
  if (width >= 32) {
    switch (pick_L(width, 8)) {
      case 4: return g16_launch<E, 4, 8>(a, stream);
      case 8: return g16_launch<E, 8, 8>(a, stream);
      case 16: return g16_launch<E, 16, 8>(a, stream);
      case 32: return g16_launch<E, 32, 8>(a, stream);
      default: return g16_launch<E, 64, 8>(a, stream);
    }
  }
  return pick_L(width, 4) == 4 ? g16_launch<E, 4, 4>(a, stream) : g16_launch<E, 8, 4>(a, stream);
}

}  // namespace

hipError_t launch_softmax_backward16(const SGrad16Args& a, int dtype, hipStream_t stream) {
  if (dtype == HCSPMM_DTYPE_F16) return g16_dispatch<F16>(a, stream);
  if (dtype == HCSPMM_DTYPE_BF16) return g16_dispatch<BF16>(a, stream);
  return hipErrorInvalidValue;
}

}  // namespace hcspmm
