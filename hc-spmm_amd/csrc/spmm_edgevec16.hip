// spmm_edgevec16.hip -- the per-entry feature-vector sum on fp16 / bf16 operands (the 16-bit dtypes of the typed edge entry points,
// DESIGN.md section 3.16b).  X and F hold 16-bit elements, Z and the partial slots are fp32:
//   Z[r][d] = sum over the entries e of row r of m(widen(X[col(e)][d]), widen(F[fi(e)][d])),  fi(e) = findex ? findex[e] : e
//   mul: fmaf(f, x, acc)    add_relu: t = fl32(x + f), acc + (t < 0 ? +0 : t)    copy: acc + f (X is not read)
// The widening is exact and the arithmetic behind it is the fp32 unit's, operation for operation: a NaN propagates, rows without
// entries give +0, and wherever the summation order does not depend on the lane count the bits are those of the fp32 launch on the
// widened operands.
//
// Lanes.  Rows sit on the dword grid (even width, even strides, 4-byte aligned bases), so a lane owns 8 columns (4 below 32
// columns per panel) and an entry costs it two 16-byte (8-byte) loads at lane_col-moved-back positions, the X row through col[e]
// and the F row through fi(e), F in 64-bit addressing: half the bytes of the fp32 unit per entry and column, and F is the stream
// that is read once per call with no reuse.  The loaded dwords stay RAW in the in-flight arrays (4 registers per 16-byte load) and
// are widened pair by pair where they are used: a bf16 pair by a shift and a mask, an fp16 pair by one conversion per half.
// kEVecU = 4 entries = eight loads are in flight per lane for mul / add_relu, kEVecCopyU = 8 entries for copy (one load each).
// The lane that loads col[e] loads findex[e] behind it (or takes e itself), one chunk ahead of the gathers, and both travel to
// the gathering lanes by shuffle; a lane past its task's end holds fi = -1 and takes nothing.
// Schedule and order: csr_schedule.h's walks; CSR order on ordinary, tiny and window rows, the xor-shuffle tree on wide tasks,
// fp32 partial slots of split rows added by the binary fix-up pass at the fp32 output's lanes.  No atomics.
#include "csr_schedule.h"

#include "hcspmm.h"

namespace hcspmm {
namespace {

constexpr int kEVecU = 4;         // entries in flight per lane, two loads each
constexpr int kEVecCopyU = 8;     // copy: one load per entry
constexpr int kEVecTiny = 2;      // tiny tasks per lane group: eight loads in flight
constexpr int kEVecMinWaves = 4;  // 128 registers per lane

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

// one column of one entry: the fp32 unit's step
template <int OP> __device__ __forceinline__ float evec_column(float acc, float x, float f) {
  if constexpr (OP == HCSPMM_EDGE_OP_MUL) {
    return __builtin_fmaf(f, x, acc);
  } else if constexpr (OP == HCSPMM_EDGE_OP_ADD_RELU) {
    const float t = __fadd_rn(x, f);
    return __fadd_rn(acc, t < 0.0f ? 0.0f : t);  // (written out: v_max_f32 drops a NaN in IEEE mode)
  } else {
    return __fadd_rn(acc, f);
  }
}

// one entry: VEC columns of the gathered X row and of the entry's F row as loaded, widened a dword at a time
template <typename E, int OP, int VEC>
__device__ __forceinline__ void edgevec16_step(typename AccT<VEC>::type& acc, const typename Lane<E, VEC>::raw_t& xr,
                                               const typename Lane<E, VEC>::raw_t& fr) {
#pragma unroll
  for (int w = 0; w < VEC / 2; ++w) {
    float x2[2] = {0.f, 0.f}, f2[2];
    if constexpr (OP != HCSPMM_EDGE_OP_COPY) widen_pair<E>(rword(xr, w), x2[0], x2[1]);
    widen_pair<E>(rword(fr, w), f2[0], f2[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) aset(acc, 2 * w + h, evec_column<OP>(aget(acc, 2 * w + h), x2[h], f2[h]));
  }
}

// One branch-free batch of UB entries: the loads back to back, kept raw; lanes past a task's end hold fi -1, re-read row 0 and
// take nothing
template <typename E, int OP, int VEC, int UB>
__device__ __forceinline__ void edgevec16_batch(const EVec16Args& ea, int csafe, bool cok, int myidx, int myfi, int src0,
                                                typename AccT<VEC>::type& acc) {
  typedef Lane<E, VEC> Ln;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(ea.p.X);
  int idx[UB], fi[UB];
  typename Ln::raw_t x[UB], f[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    idx[u] = OP == HCSPMM_EDGE_OP_COPY ? 0 : __shfl(myidx, src0 + u, 64);
    fi[u] = __shfl(myfi, src0 + u, 64);
  }
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    if constexpr (OP != HCSPMM_EDGE_OP_COPY) x[u] = Ln::load(X + (size_t)max(idx[u], 0) * ea.p.ldx + csafe);
    else x[u] = Ln::zero();
    f[u] = Ln::load(ea.F + (size_t)max(fi[u], 0) * ea.ldf + csafe);
  }
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && fi[u] >= 0) edgevec16_step<E, OP, VEC>(acc, x[u], f[u]);
}

// L lanes own the task = entries [e0, e0 + n); WIDE: the whole wave owns it and the 64/L lane-group sums are combined by the
// fixed xor-shuffle tree.  dz: the row of Z, dp: the partial slot (one of them; both null: a lane group without a task)
template <typename E, int OP, int L, int VEC, bool WIDE>
__device__ __forceinline__ void edgevec16_task(const EVec16Args& ea, float* dz, float* dp, int e0, int n, int c0, int cend,
                                               int lane) {
  typedef Lane<F32, VEC> Out;
  constexpr int UMAX = OP == HCSPMM_EDGE_OP_COPY ? kEVecCopyU : kEVecU;
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
          edgevec16_batch<E, OP, VEC, U>(ea, c, cok, myidx, myfi, gbase + j, acc);
          j += U;
        } else if (U >= 8 && left > U / 4) {
          edgevec16_batch<E, OP, VEC, (U >= 8 ? U / 2 : 1)>(ea, c, cok, myidx, myfi, gbase + j, acc);
          j += U / 2;
        } else if (U >= 4 && left > 1) {
          edgevec16_batch<E, OP, VEC, (U >= 8 ? U / 4 : 2)>(ea, c, cok, myidx, myfi, gbase + j, acc);
          j += (U >= 8 ? U / 4 : 2);
        } else {
          edgevec16_batch<E, OP, VEC, 1>(ea, c, cok, myidx, myfi, gbase + j, acc);
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
      if (dz != nullptr) Out::store(dz + c, acc);
      else if (dp != nullptr) Out::store_partial(dp + c, acc);
    }
  }
}

// destinations of a task descriptor (row | first entry | length | partial slot or -1)
struct EVecDst {
  float* z;
  float* p;
};
__device__ __forceinline__ EVecDst edgevec16_dst(const EVec16Args& ea, int row, int slot) {
  const PlanArgs& a = ea.p;
  EVecDst d{nullptr, nullptr};
  if (slot < 0) d.z = reinterpret_cast<float*>(a.Z) + (size_t)row * a.ldz;
  else d.p = a.partial + (size_t)slot * (size_t)a.D;
  return d;
}

// T tasks of at most two entries per lane group, column ids inline in the descriptor; the entry position (the F row, or the
// place in findex) comes from rowptr (a whole row) or the fix-up list (the last segment of a split row)
template <typename E, int OP, int L, int VEC, int T>
__device__ __forceinline__ void edgevec16_tiny(const EVec16Args& ea, int first, int c0, int cend, int lane) {
  typedef Lane<E, VEC> Ln;
  typedef Lane<F32, VEC> Out;
  typedef typename Ln::raw_t raw_t;
  const PlanArgs& a = ea.p;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(a.X);
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
    raw_t x0[T], x1[T], v0[T], v1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) x0[t] = x1[t] = v0[t] = v1[t] = Ln::zero();
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
      typename AccT<VEC>::type acc = azero<VEC>();
      if (d[t].y >= 0) edgevec16_step<E, OP, VEC>(acc, x0[t], v0[t]);
      if (d[t].w >= 0) edgevec16_step<E, OP, VEC>(acc, x1[t], v1[t]);
      if (cok && d[t].z >= 0) {
        const EVecDst o = d[t].x >= 0 ? edgevec16_dst(ea, d[t].x, -1) : edgevec16_dst(ea, 0, -(d[t].x + 1));
        if (o.z != nullptr) Out::store(o.z + c, acc);
        else Out::store_partial(o.p + c, acc);
      }
    }
  }
}

// what csr_schedule.h's walks call
template <typename E, int OP, int L, int VEC> struct EVec16Body {
  const EVec16Args& ea;
  typedef EVecDst Dst;
  __device__ __forceinline__ Dst dst(int row, int slot) const { return edgevec16_dst(ea, row, slot); }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    edgevec16_task<E, OP, L, VEC, WIDE>(ea, o.z, o.p, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    edgevec16_tiny<E, OP, L, VEC, kEVecTiny>(ea, first, c0, cend, lane);
  }
};

// the planned and the plan-free kernel (csr_schedule.h)
template <typename E, int OP, int L, int VEC>
__global__ __launch_bounds__(kThreads, kEVecMinWaves) void edgevec16_plan_kernel(EVec16Args ea) {
  csr_plan_walk<L, kEVecTiny>(ea.p, ea.rowptr, EVec16Body<E, OP, L, VEC>{ea});
}
template <typename E, int OP, int L, int VEC>
__global__ __launch_bounds__(kThreads, kEVecMinWaves) void edgevec16_window_kernel(EVec16Args ea) {
  csr_window_walk<L>(ea.p, ea.rowptr, EVec16Body<E, OP, L, VEC>{ea});
}

// Z is fp32 at any width served (D >= 4): the fix-up pass is the binary one at four floats per lane
template <typename E, int L, int VEC> hipError_t edgevec16_ops(const EVec16Args& a, hipStream_t stream) {
  switch (a.op) {
    case HCSPMM_EDGE_OP_MUL:
      return csr_launch(a, L, kEVecTiny, edgevec16_window_kernel<E, HCSPMM_EDGE_OP_MUL, L, VEC>,
                        edgevec16_plan_kernel<E, HCSPMM_EDGE_OP_MUL, L, VEC>, fixup_kernel<F32, 4>, stream);
    case HCSPMM_EDGE_OP_ADD_RELU:
      return csr_launch(a, L, kEVecTiny, edgevec16_window_kernel<E, HCSPMM_EDGE_OP_ADD_RELU, L, VEC>,
                        edgevec16_plan_kernel<E, HCSPMM_EDGE_OP_ADD_RELU, L, VEC>, fixup_kernel<F32, 4>, stream);
    case HCSPMM_EDGE_OP_COPY:
      return csr_launch(a, L, kEVecTiny, edgevec16_window_kernel<E, HCSPMM_EDGE_OP_COPY, L, VEC>,
                        edgevec16_plan_kernel<E, HCSPMM_EDGE_OP_COPY, L, VEC>, fixup_kernel<F32, 4>, stream);
    default: return hipErrorInvalidValue;
  }
}

// The unit's own lanes (csr_dispatch serves 4-element lanes and narrower): 8 elements per lane with L = pick_L of the panel
// (planned) or of D (plan-free) from 32 columns on, 4 elements per lane with L = 4 or 8 below
template <typename E> hipError_t edgevec16_dispatch(const EVec16Args& a, hipStream_t stream) {
  const int width = a.p.plan != nullptr ? a.p.panel_cols : a.p.D;
  if (a.p.D < 4 || (a.p.D & 1)) return hipErrorInvalidValue;
  if (a.p.D >= 32) {
    switch (pick_L(width, 8)) {
      case 4: return edgevec16_ops<E, 4, 8>(a, stream);
      case 8: return edgevec16_ops<E, 8, 8>(a, stream);
      case 16: return edgevec16_ops<E, 16, 8>(a, stream);
      case 32: return edgevec16_ops<E, 32, 8>(a, stream);
      default: return edgevec16_ops<E, 64, 8>(a, stream);
    }
  }
  return pick_L(width, 4) == 4 ? edgevec16_ops<E, 4, 4>(a, stream) : edgevec16_ops<E, 8, 4>(a, stream);
}

}  // namespace

hipError_t launch_edgevec16(const EVec16Args& a, int dtype, hipStream_t stream) {
  if (dtype == HCSPMM_DTYPE_F16) return edgevec16_dispatch<F16>(a, stream);
  if (dtype == HCSPMM_DTYPE_BF16) return edgevec16_dispatch<BF16>(a, stream);
  return hipErrorInvalidValue;
}

}  // namespace hcspmm
