// spmm_heads16.hip -- the multi-head weighted aggregation on fp16 / bf16 rows (the 16-bit dtypes of
// hcspmm_forward_weighted_heads_typed).  X holds 16-bit elements, the values are fp32 and head-major
// [heads][num_values], the sums are fp32:
//   Z[r][h*Dh + j] = sum over the entries e of row r of values[h*num_values + vi(e)] * widen(X[col(e)][h*Dh + j])
//   vi(e) = vindex ? vindex[e] : e,   acc = fmaf(v, x, acc)
// Z is fp32, or X's type rounded once from the fp32 sum (nearest even, a NaN stays a NaN).
//
// Lanes and heads.  Rows sit on the dword grid (even strides, 4-byte aligned bases).  A lane owns 8 columns (one 16-byte load per
// entry) when Dh % 8 == 0 and the panel has at least 32 columns, 4 columns (8-byte loads) otherwise; Dh % 4 == 0 and panels are
// multiples of 16 columns, so a lane's columns never leave one head and no lane is moved back.  Dh need not be a power of two: a
// lane derives its head from its first column, h = c / Dh, once per column pass.  One value per entry and lane then suffices.
// The loaded dwords stay RAW in the in-flight arrays and are widened pair by pair where they are used; U = 8 entries = eight
// gathers are in flight per lane.
//
// Values.  The lane that loads col[e] for a chunk loads vindex[e] behind it, one chunk ahead of the gathers, and both travel to
// the gathering lanes by shuffle.  Identity form (vindex a template argument: this build has no index load and no index
// shuffle): the entries of a batch are consecutive, so a lane takes the batch's values of its head as runs of four floats, one
// element-aligned 16-byte load per four entries instead of one 4-byte load per entry.  Indexed form: every gathering lane loads
// the value of its own head through the shuffled index.  (Sets of 2 or 4 adjacent lanes of a head that split a batch's entries and
// hand the values round by shuffle were built and measured: within 0.7 % of these per-lane loads either way, DESIGN.md 3.11b, so
// the simpler form stays.)
// Schedule and order: csr_schedule.h's walks; CSR order on ordinary, tiny and window rows, the fixed xor-shuffle tree on wide
// tasks; split rows go to fp32 partial slots, added by the binary fix-up pass (fp32 Z) or by heads16_fixup_kernel in slot order
// with one rounding (16-bit Z).  No atomics.
#include "csr_schedule.h"

#include "hcspmm.h"

namespace hcspmm {
namespace {

constexpr int kHeadsU = 8;         // entries (= gathers) in flight per lane
constexpr int kHeadsMinWaves = 4;  // 128 registers per lane
// tiny tasks per lane group: eight gathers in flight, four at the widest builds (registers)
template <int L> struct HeadsTinyT {
  static constexpr int value = L >= 32 ? 2 : 4;
};

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

// one entry: VEC columns of the gathered row as loaded, widened a dword at a time, times the head's value
template <typename E, int VEC>
__device__ __forceinline__ void heads16_step(typename AccT<VEC>::type& acc, const typename Lane<E, VEC>::raw_t& xr, float v) {
#pragma unroll
  for (int w = 0; w < VEC / 2; ++w) {
    float lo, hi;
    widen_pair<E>(rword(xr, w), lo, hi);
    aset(acc, 2 * w, __builtin_fmaf(v, lo, aget(acc, 2 * w)));
    aset(acc, 2 * w + 1, __builtin_fmaf(v, hi, aget(acc, 2 * w + 1)));
  }
}

// One branch-free batch of UB entries of a lane group: task positions [t0, t0 + UB), of which the first `nvalid` exist (<= 0:
// none).  e: the CSR position of t0 (identity form: its value index).  The gathers go out back to back and stay raw.
// hv: the slice of the lane's head, values + head * num_values
template <typename E, int VEC, int UB, bool IDX>
__device__ __forceinline__ void heads16_batch(const Heads16Args& ha, const float* hv, int csafe, bool cok, int myidx, int myvi,
                                              int src0, int e, int nvalid, typename AccT<VEC>::type& acc) {
  typedef Lane<E, VEC> Ln;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(ha.p.X);
  int idx[UB];
  float v[UB];
  typename Ln::raw_t x[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = __shfl(myidx, src0 + u, 64);
#pragma unroll
  for (int u = 0; u < UB; ++u) x[u] = Ln::load(X + (size_t)max(idx[u], 0) * ha.p.ldx + csafe);
  if constexpr (!IDX) {
    // consecutive positions: runs of four values of the lane's head
#pragma unroll
    for (int u = 0; u < UB; ++u) v[u] = 0.f;
    if (cok) {
      if constexpr (UB >= 4) {
#pragma unroll
        for (int k = 0; k < UB / 4; ++k) {
          if (nvalid >= 4 * k + 4) {
            const f32x4 r = *reinterpret_cast<const MemF32<4>::type*>(hv + e + 4 * k);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * k + i] = r[i];
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (4 * k + i < nvalid) v[4 * k + i] = hv[e + 4 * k + i];
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < UB; ++u)
          if (u < nvalid) v[u] = hv[e + u];
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int vi = __shfl(myvi, src0 + u, 64);
      v[u] = (cok && vi >= 0) ? hv[vi] : 0.f;
    }
  }
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && u < nvalid) heads16_step<E, VEC>(acc, x[u], v[u]);
}

// destinations of a task descriptor (row | first entry | length | partial slot or -1): the row of Z in its own type, or the slot
struct HeadsDst {
  void* z;
  float* p;
};
__device__ __forceinline__ HeadsDst heads16_dst(const Heads16Args& ha, int row, int slot) {
  const PlanArgs& a = ha.p;
  HeadsDst d{nullptr, nullptr};
  if (slot >= 0) d.p = a.partial + (size_t)slot * (size_t)a.D;
  else if (ha.z16) d.z = reinterpret_cast<unsigned short*>(a.Z) + (size_t)row * a.ldz;
  else d.z = reinterpret_cast<float*>(a.Z) + (size_t)row * a.ldz;
  return d;
}
template <typename E, int VEC>
__device__ __forceinline__ void heads16_store(const Heads16Args& ha, const HeadsDst& o, int c, const typename AccT<VEC>::type& acc) {
  if (o.p != nullptr) Lane<F32, VEC>::store_partial(o.p + c, acc);
  else if (o.z == nullptr) return;
  else if (ha.z16) Lane<E, VEC>::store(reinterpret_cast<unsigned short*>(o.z) + c, acc);  // one rounding
  else Lane<F32, VEC>::store(reinterpret_cast<float*>(o.z) + c, acc);
}

// L lanes own the task = entries [e0, e0 + n); WIDE: the whole wave owns it and the 64/L lane-group sums are combined by the
// fixed xor-shuffle tree.  A value-initialised o: a lane group without a task (n = 0)
template <typename E, int L, int VEC, bool IDX, bool WIDE>
__device__ __forceinline__ void heads16_task(const Heads16Args& ha, const HeadsDst& o, int e0, int n, int c0, int cend, int lane) {
  constexpr int U = (L < kHeadsU) ? L : kHeadsU;
  constexpr int STRIDE = WIDE ? 64 : L;
  const int* __restrict__ col = ha.p.col;
  const int* __restrict__ vindex = ha.vindex;
  const int s = lane & (L - 1);
  const int pos = WIDE ? lane : s;
  const int gbase = lane & ~(L - 1);
  const int goff = WIDE ? gbase : 0;  // the lane group's first position within a chunk
  int nmax = n;
  if (!WIDE) {
#pragma unroll
    for (int off = L; off < 64; off <<= 1) nmax = max(nmax, __shfl_xor(nmax, off, 64));
  }
  nmax = __builtin_amdgcn_readfirstlane(nmax);

  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const int c = pbase + s * VEC;  // (D, Dh and the panels are multiples of VEC: c + VEC <= cend wherever c < cend)
    const bool cok = c < cend;
    const int csafe = cok ? c : 0;
    const float* hv = ha.values + (size_t)(csafe / ha.dh) * (size_t)ha.num_values;  // the lane's head from its first column
    typename AccT<VEC>::type acc = azero<VEC>();
    int next = 0, nextv = -1;
    if (pos < n) {
      next = col[e0 + pos];
      if (IDX) nextv = vindex[e0 + pos];
    }
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next, myvi = nextv;
      const int en = e0 + base + STRIDE + pos;  // the next chunk's indices arrive under this chunk's gathers
      next = 0;
      nextv = -1;
      if (base + STRIDE + pos < n) {
        next = col[en];
        if (IDX) nextv = vindex[en];
      }
      const int cnt = min(L, nmax - base);
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
        const int t0 = base + goff + j;  // the batch's first position in the task
        if (left > U / 2) {
          heads16_batch<E, VEC, U, IDX>(ha, hv, csafe, cok, myidx, myvi, gbase + j, e0 + t0, n - t0, acc);
          j += U;
        } else if (U >= 8 && left > U / 4) {
          heads16_batch<E, VEC, (U >= 8 ? U / 2 : 1), IDX>(ha, hv, csafe, cok, myidx, myvi, gbase + j, e0 + t0, n - t0, acc);
          j += U / 2;
        } else if (U >= 4 && left > 1) {
          heads16_batch<E, VEC, (U >= 8 ? U / 4 : 2), IDX>(ha, hv, csafe, cok, myidx, myvi, gbase + j, e0 + t0, n - t0, acc);
          j += (U >= 8 ? U / 4 : 2);
        } else {
          heads16_batch<E, VEC, 1, IDX>(ha, hv, csafe, cok, myidx, myvi, gbase + j, e0 + t0, n - t0, acc);
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
    if (cok && (!WIDE || lane < L)) heads16_store<E, VEC>(ha, o, c, acc);
  }
}

// T tasks of at most two entries per lane group, column ids inline in the descriptor; the entry position (the value's, or the
// place in vindex) comes from rowptr (a whole row) or the fix-up list (the last segment of a split row)
template <typename E, int L, int VEC, bool IDX, int T>
__device__ __forceinline__ void heads16_tiny(const Heads16Args& ha, int first, int c0, int cend, int lane) {
  typedef Lane<E, VEC> Ln;
  typedef typename Ln::raw_t raw_t;
  const PlanArgs& a = ha.p;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(a.X);
  constexpr int R = 64 / L;
  const int g = lane / L, s = lane & (L - 1);
  const int4* tasks = reinterpret_cast<const int4*>(a.plan + a.off_tasks);
  int4 d[T];
  int v0i[T], v1i[T];
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
    if (d[t].y >= 0) e = d[t].x >= 0 ? ha.rowptr[d[t].x] : segment_entry(a, ha.rowptr, ha.segment_len, -(d[t].x + 1));
    v0i[t] = v1i[t] = 0;
    if (d[t].y >= 0) v0i[t] = IDX ? ha.vindex[e] : e;
    if (d[t].w >= 0) v1i[t] = IDX ? ha.vindex[e + 1] : e + 1;
  }
  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const int c = pbase + s * VEC;
    const bool cok = c < cend;
    const int csafe = cok ? c : 0;
    const float* hv = ha.values + (size_t)(csafe / ha.dh) * (size_t)ha.num_values;
    raw_t x0[T], x1[T];
    float w0[T], w1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      x0[t] = x1[t] = Ln::zero();
      w0[t] = w1[t] = 0.f;
    }
    if (any1) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        x0[t] = Ln::load(X + (size_t)max(d[t].y, 0) * a.ldx + csafe);
        if (d[t].y >= 0) w0[t] = hv[v0i[t]];
      }
    }
    if (any2) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        x1[t] = Ln::load(X + (size_t)max(d[t].w, 0) * a.ldx + csafe);
        if (d[t].w >= 0) w1[t] = hv[v1i[t]];
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      typename AccT<VEC>::type acc = azero<VEC>();
      if (d[t].y >= 0) heads16_step<E, VEC>(acc, x0[t], w0[t]);
      if (d[t].w >= 0) heads16_step<E, VEC>(acc, x1[t], w1[t]);
      if (cok && d[t].z >= 0) {
        const HeadsDst o = d[t].x >= 0 ? heads16_dst(ha, d[t].x, -1) : heads16_dst(ha, 0, -(d[t].x + 1));
        heads16_store<E, VEC>(ha, o, c, acc);
      }
    }
  }
}

// what csr_schedule.h's walks call
template <typename E, int L, int VEC, bool IDX> struct Heads16Body {
  const Heads16Args& ha;
  typedef HeadsDst Dst;
  __device__ __forceinline__ Dst dst(int row, int slot) const { return heads16_dst(ha, row, slot); }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    heads16_task<E, L, VEC, IDX, WIDE>(ha, o, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    heads16_tiny<E, L, VEC, IDX, HeadsTinyT<L>::value>(ha, first, c0, cend, lane);
  }
};

// the planned and the plan-free kernel (csr_schedule.h)
template <typename E, int L, int VEC, bool IDX>
__global__ __launch_bounds__(kThreads, kHeadsMinWaves) void heads16_plan_kernel(Heads16Args ha) {
  csr_plan_walk<L, HeadsTinyT<L>::value>(ha.p, ha.rowptr, Heads16Body<E, L, VEC, IDX>{ha});
}
template <typename E, int L, int VEC, bool IDX>
__global__ __launch_bounds__(kThreads, kHeadsMinWaves) void heads16_window_kernel(Heads16Args ha) {
  csr_window_walk<L>(ha.p, ha.rowptr, Heads16Body<E, L, VEC, IDX>{ha});
}

// The fix-up pass of a 16-bit Z: one wave per split row, a lane per four columns; the row's fp32 partial slots are added in slot
// order, eight loads in flight, and the sum is rounded once.  (fp32 Z takes the binary pass, fixup_kernel<F32, 4>.)
template <typename E>
__global__ __launch_bounds__(kThreads) void heads16_fixup_kernel(PlanArgs a) {
  typedef Lane<E, 4> Ln;
  unsigned short* Z = reinterpret_cast<unsigned short*>(a.Z);
  const int lane = threadIdx.x & 63;
  const int fi = (int)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (fi >= a.n_split_rows) return;
  const int4 f = reinterpret_cast<const int4*>(a.plan + a.off_fixups)[fi];
  const int row = f.x, s0 = f.y, ns = f.z;
  for (int c = lane * 4; c < a.D; c += 256) {  // (D % 4 == 0)
    const float* p = a.partial + (size_t)s0 * (size_t)a.D + c;
    f32x4 acc = azero<4>();
    int s = 0;
    for (; s + 8 <= ns; s += 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = Lane<F32, 4>::load_partial(p + (size_t)(s + u) * (size_t)a.D);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; s < ns; ++s) acc += Lane<F32, 4>::load_partial(p + (size_t)s * (size_t)a.D);
    Ln::store(Z + (size_t)row * a.ldz + c, acc);
  }
}

template <typename E, int L, int VEC, bool IDX> hipError_t heads16_launch(const Heads16Args& a, hipStream_t stream) {
  constexpr int T = HeadsTinyT<L>::value;
  if (a.z16)
    return csr_launch(a, L, T, heads16_window_kernel<E, L, VEC, IDX>, heads16_plan_kernel<E, L, VEC, IDX>, heads16_fixup_kernel<E>,
                      stream);
  return csr_launch(a, L, T, heads16_window_kernel<E, L, VEC, IDX>, heads16_plan_kernel<E, L, VEC, IDX>, fixup_kernel<F32, 4>, stream);
}

// The unit's lanes: 8 elements per lane with L = pick_L of the panel (planned) or of D (plan-free) when Dh % 8 == 0 and that
// width is at least 32 columns; else csr_dispatch's 4-element lanes
template <typename E, bool IDX> hipError_t heads16_dispatch(const Heads16Args& a, hipStream_t stream) {
  const int width = a.p.plan != nullptr ? a.p.panel_cols : a.p.D;
  if (a.dh <= 0 || a.dh % 4 != 0 || a.p.D % a.dh != 0) return hipErrorInvalidValue;
  if (a.p.plan != nullptr && width < a.p.D && width % 16 != 0) return hipErrorInvalidValue;
  if (a.dh % 8 == 0 && width >= 32) {
    switch (pick_L(width, 8)) {
      case 4: return heads16_launch<E, 4, 8, IDX>(a, stream);
      case 8: return heads16_launch<E, 8, 8, IDX>(a, stream);
      case 16: return heads16_launch<E, 16, 8, IDX>(a, stream);
      case 32: return heads16_launch<E, 32, 8, IDX>(a, stream);
      default: return heads16_launch<E, 64, 8, IDX>(a, stream);
    }
  }
  return csr_dispatch(a.p, 4, [&](auto lv) { return heads16_launch<E, decltype(lv)::L, 4, IDX>(a, stream); });
}

}  // namespace

hipError_t launch_heads16(const Heads16Args& a, int dtype, hipStream_t stream) {
  if (dtype == HCSPMM_DTYPE_F16) return a.vindex ? heads16_dispatch<F16, true>(a, stream) : heads16_dispatch<F16, false>(a, stream);
  if (dtype == HCSPMM_DTYPE_BF16) return a.vindex ? heads16_dispatch<BF16, true>(a, stream) : heads16_dispatch<BF16, false>(a, stream);
  return hipErrorInvalidValue;
}

}  // namespace hcspmm
