// softmax_aggr_grad.hip -- gradient of the softmax aggregation with respect to X (hcspmm_softmax_backward, DESIGN.md section
// 3.18), fp32 on the plan of the graph the backward walks (A^T's, or A's own for a symmetric pattern):
//   dX[j][d] = sum over the entries (j, i) of row j of  exp(s_j - M[i][d]) / L[i][d] * G[i][d] * (1 + beta[d] (x_j - Z[i][d])),
//   x_j = X[j][d], s_j = fl(beta[d] * x_j)
// The softmax weight of entry (i, j) of A is recomputed from the forward's M and L: no [E, D] tensor, no transpose
// permutation.  On the true transpose s_j <= M[i] (j is among row i's entries), so the exponent is <= 0, and L >= 1.
//
// A plain-sum sparse-row launch on csr_schedule.h's schedule (every row, a dense-tile window's included, is a sparse-row
// task), with fixup_kernel's pass over split rows.
//  * Every entry issues FOUR 16-byte loads per lane (G, Z, M, L rows of one stride through col[e]); two entries are in flight
//    per lane, the binary gather's eight loads.
//  * The task's own row of X and beta are per-lane constants of a column chunk.  A tiny task that carries a partial slot
//    instead of its row finds the row through the fix-up list.
//  * Sums run in hcspmm_forward_weighted's order: CSR order on ordinary and tiny tasks, the wide tasks' xor-shuffle tree, fp32
//    partials of sliced and segmented rows added by the fix-up pass in fixup_kernel's order.  No atomics.
#include "csr_schedule.h"

namespace hcspmm {
namespace {

constexpr int kGradU = 2;  // entries in flight per lane: eight 16-byte loads
constexpr float kLog2e = 1.44269504088896340736f;

// per-lane constants of a column chunk: the task's own x, beta and s = fl(beta x)
template <int VEC> struct GOwn {
  typename AccT<VEC>::type x, b, s;
};

template <int VEC>
__device__ __forceinline__ GOwn<VEC> gown(const SGradArgs& ga, int row, int c) {
  typedef Lane<F32, VEC> Ln;
  GOwn<VEC> o;
  o.b = Ln::load(ga.beta + c);
  o.x = row >= 0 ? Ln::load(reinterpret_cast<const float*>(ga.p.X) + (size_t)row * ga.p.ldx + c) : azero<VEC>();
#pragma unroll
  for (int q = 0; q < VEC; ++q) aset(o.s, q, __fmul_rn(aget(o.b, q), aget(o.x, q)));
  return o;
}

// one entry: VEC columns of the gathered G, Z, M, L rows
template <int VEC>
__device__ __forceinline__ void gstep(typename AccT<VEC>::type& acc, const GOwn<VEC>& o, const typename AccT<VEC>::type& g,
                                      const typename AccT<VEC>::type& z, const typename AccT<VEC>::type& m,
                                      const typename AccT<VEC>::type& l) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    const float p = __builtin_amdgcn_exp2f(__fsub_rn(aget(o.s, q), aget(m, q)) * kLog2e) * __builtin_amdgcn_rcpf(aget(l, q));
    const float k = __builtin_fmaf(aget(o.b, q), __fsub_rn(aget(o.x, q), aget(z, q)), 1.0f);
    aset(acc, q, __builtin_fmaf(p * aget(g, q), k, aget(acc, q)));
  }
}

// One branch-free batch of UB entries (spmm_impl.h gather_batch): lanes past a task's end hold idx -1, re-read row 0 and take
// nothing
template <int VEC, int UB>
__device__ __forceinline__ void gbatch(const SGradArgs& ga, int csafe, bool cok, int myidx, int src0, const GOwn<VEC>& o,
                                       typename AccT<VEC>::type& acc) {
  typedef Lane<F32, VEC> Ln;
  int idx[UB];
  typename AccT<VEC>::type g[UB], z[UB], m[UB], l[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = __shfl(myidx, src0 + u, 64);
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const size_t off = (size_t)max(idx[u], 0) * ga.ld_in + csafe;
    g[u] = Ln::load(ga.G + off);
    z[u] = Ln::load(ga.Zf + off);
    m[u] = Ln::load(ga.M + off);
    l[u] = Ln::load(ga.L + off);
  }
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && idx[u] >= 0) gstep<VEC>(acc, o, g[u], z[u], m[u], l[u]);
}

// sparse_task_w (spmm_weighted_impl.h) with the gradient step: L lanes own the task = entries [e0, e0 + n) of row `row` (< 0: a
// lane group without a task); WIDE: the whole wave owns it and the 64/L lane-group sums are combined by the fixed tree
template <int L, int VEC, bool WIDE>
__device__ __forceinline__ void gtask(const SGradArgs& ga, int row, float* dz, float* dp, int e0, int n, int c0, int cend, int lane) {
  typedef Lane<F32, VEC> Ln;
  constexpr int U = (L < kGradU) ? L : kGradU;
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
    const GOwn<VEC> o = gown<VEC>(ga, row, c);
    typename AccT<VEC>::type acc = azero<VEC>();
    int next = pos < n ? col[e0 + pos] : -1;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      next = base + STRIDE + pos < n ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      const int cnt = min(L, nmax - base);
      for (int j = 0; j < cnt;) {
        if (U >= 2 && cnt - j > 1) {
          gbatch<VEC, U>(ga, c, cok, myidx, gbase + j, o, acc);
          j += U;
        } else {
          gbatch<VEC, 1>(ga, c, cok, myidx, gbase + j, o, acc);
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
struct GDst {
  float* z;
  float* p;
};
__device__ __forceinline__ GDst task_dst(const SGradArgs& ga, int row, int slot) {
  const PlanArgs& a = ga.p;
  GDst d{nullptr, nullptr};
  if (slot < 0) d.z = reinterpret_cast<float*>(a.Z) + (size_t)row * a.ldz;
  else d.p = a.partial + (size_t)slot * (size_t)a.D;
  return d;
}

// tiny_tasks_w (spmm_weighted_impl.h), one task of at most two entries per lane group (eight loads), column ids inline in the
// descriptor; the own row comes from the descriptor (a whole row) or the fix-up list (the last segment of a split row)
template <int L, int VEC>
__device__ __forceinline__ void gtiny(const SGradArgs& ga, int first, int c0, int cend, int lane) {
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
    const GOwn<VEC> o = gown<VEC>(ga, row, c);
    acc_t g0 = azero<VEC>(), z0 = g0, m0 = g0, l0 = g0, g1 = g0, z1 = g0, m1 = g0, l1 = g0;
    if (any1) {
      const size_t off = (size_t)max(d.y, 0) * ga.ld_in + c;
      g0 = Ln::load(ga.G + off);
      z0 = Ln::load(ga.Zf + off);
      m0 = Ln::load(ga.M + off);
      l0 = Ln::load(ga.L + off);
    }
    if (any2) {
      const size_t off = (size_t)max(d.w, 0) * ga.ld_in + c;
      g1 = Ln::load(ga.G + off);
      z1 = Ln::load(ga.Zf + off);
      m1 = Ln::load(ga.M + off);
      l1 = Ln::load(ga.L + off);
    }
    acc_t acc = azero<VEC>();
    if (d.y >= 0) gstep<VEC>(acc, o, g0, z0, m0, l0);
    if (d.w >= 0) gstep<VEC>(acc, o, g1, z1, m1, l1);
    if (cok && d.z >= 0) {
      const GDst t = d.x >= 0 ? task_dst(ga, d.x, -1) : task_dst(ga, 0, -(d.x + 1));
      if (t.z != nullptr) Ln::store(t.z + c, acc);
      else Ln::store_partial(t.p + c, acc);
    }
  }
}

// what csr_schedule.h's walks call: one tiny task per lane group
template <int L, int VEC> struct GBody {
  const SGradArgs& ga;
  struct Dst {  // gtask reads the task's own row of X as well
    int row = -1;
    GDst o{nullptr, nullptr};
  };
  __device__ __forceinline__ Dst dst(int row, int slot) const { return Dst{row, task_dst(ga, row, slot)}; }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& d, int e0, int n, int c0, int cend, int lane) const {
    gtask<L, VEC, WIDE>(ga, d.row, d.o.z, d.o.p, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const { gtiny<L, VEC>(ga, first, c0, cend, lane); }
};

constexpr int kGradMinWaves = 4;  // 128 registers per lane

// the planned and the plan-free kernel (csr_schedule.h)
template <int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void softmax_grad_plan_kernel(SGradArgs ga) {
  csr_plan_walk<L, 1>(ga.p, ga.rowptr, GBody<L, VEC>{ga});
}
template <int L, int VEC, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void softmax_grad_window_kernel(SGradArgs ga) {
  csr_window_walk<L>(ga.p, ga.rowptr, GBody<L, VEC>{ga});
}

}  // namespace

hipError_t launch_softmax_backward_f32(const SGradArgs& a, int vec, hipStream_t stream) {
  return csr_dispatch(a.p, vec, [&](auto lv) {
    constexpr int L = decltype(lv)::L, VEC = decltype(lv)::VEC;
    return csr_launch(a, L, 1, softmax_grad_window_kernel<L, VEC, kGradMinWaves>, softmax_grad_plan_kernel<L, VEC, kGradMinWaves>,
                      fixup_kernel<F32, VEC>, stream);  // fp32 sums: the binary pass
  });
}

}  // namespace hcspmm
