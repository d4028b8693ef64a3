// spmm_extremum16.hip -- max / min neighbour aggregation with its argmax on fp16 / bf16 features (the 16-bit dtypes of
// hcspmm_forward_extremum_typed):
//   Z[r][d] = the 16 bits of the winning X[col(e)][d] over the entries e of row r,  arg[r][d] = the winning e (int32)
// under extremum_common.h's order on the widened values: NaN above every number (max and min alike), then the larger (min: the
// smaller) value, -0 == +0, ties and NaN against NaN to the lower CSR position.  A maximum selects, so nothing is rounded.
//
// Lanes.  Rows sit on the dword grid (even width, even strides, 4-byte aligned bases): a lane owns 8 columns -- one 16-byte load
// per gathered row -- from 32 columns per panel on and 4 columns (8-byte loads) below, a lane whose columns would run past a
// ragged end moved back onto the last ones (lane_col; its duplicate stores carry the same winners).  Half the gathered bytes of
// the fp32 unit per column.  The in-flight loads of a batch stay RAW dwords (4 registers per 16-byte load); a dword is widened
// where it is used, both halves at once: a bf16 pair by a shift and a mask, an fp16 pair by one conversion per half.  min flips
// both sign bits of the dword with one xor before that, and the store flips the winner back.
// Compare.  The widened fp32 value is compared (option "widen", not an integer key: one or two operations to widen against
// six or more to build an ordered key, and the state stays (fp32 value, position) = 2 registers per column, 16 at 8 columns).
// A lane scans its entries in rising CSR position, so inside the scan a later entry wins only by being strictly better:
//   win = !(v <= best) && best == best        (v > best, or v is NaN and best is not)
// -- two compares, no position compare.  What the strict compare cannot see is a run of -inf (min: +inf) from the start: it
// never beats the initial -inf.  A scan that saw entries and took none saw only those, and settle() gives it its first entry.
// Across lane groups (wide tasks' xor-shuffle tree) and partial slots (fix-up) positions do not rise: the full order, xbeats.
// Split rows keep the fp32 unit's slots: fp32 values (the widened winners, still flipped for min), then int32 positions
// (hcspmm_extremum_workspace_bytes); the unit's own fix-up kernel combines them and stores 16-bit Z.
// Output bits.  bf16 narrows by a shift, exactly.  fp16 goes through the conversions, which quiet a signalling NaN: a column
// whose winner is a NaN re-reads the element it names (X[col[arg]][d]) -- a rare, one-element load.
// Schedule: csr_schedule.h's walks; tiny tasks XTinyT<L> per lane group, as the fp32 unit.  No atomics.
#include "csr_schedule.h"
#include "extremum_common.h"  // xbeats, xflip, kNone, XTinyT, the int32 lane vectors

namespace hcspmm {
namespace {

constexpr int kX16MinWaves = 4;  // 128 registers per lane

// the two 16-bit elements of a dword, widened (exact)
template <typename E> __device__ __forceinline__ void x16_widen(unsigned w, float& lo, float& hi);
template <> __device__ __forceinline__ void x16_widen<BF16>(unsigned w, float& lo, float& hi) {
  lo = __uint_as_float(w << 16);
  hi = __uint_as_float(w & 0xffff0000u);
}
template <> __device__ __forceinline__ void x16_widen<F16>(unsigned w, float& lo, float& hi) {
  lo = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
  hi = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
}
// a widened value back to its 16 bits (exact, but fp16 NaNs: x16_own_bits)
template <typename E> __device__ __forceinline__ unsigned x16_narrow(float f);
template <> __device__ __forceinline__ unsigned x16_narrow<BF16>(float f) { return __float_as_uint(f) >> 16; }
template <> __device__ __forceinline__ unsigned x16_narrow<F16>(float f) {
  return __builtin_bit_cast(unsigned short, (_Float16)f);
}

// best (flipped, widened) value and its entry of VEC columns
template <int VEC> struct X16State {
  float bv[VEC];
  int bp[VEC];
  __device__ __forceinline__ X16State() {
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      bv[q] = -__builtin_inff();
      bp[q] = kNone;
    }
  }
  // entry p comes after every entry this state has seen
  __device__ __forceinline__ void scan(float v, int p, int q) {
    if (!(v <= bv[q]) && bv[q] == bv[q]) {
      bv[q] = v;
      bp[q] = p;
    }
  }
  // any other pair: the full order
  __device__ __forceinline__ void take(float v, int p, int q) {
    if (xbeats(v, p, bv[q], bp[q])) {
      bv[q] = v;
      bp[q] = p;
    }
  }
  // after a scan that saw entries, `first` the first of them: columns that took none saw -inf only
  __device__ __forceinline__ void settle(int first) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) bp[q] = bp[q] == kNone ? first : bp[q];
  }
};

// one gathered row at entry e: VEC columns as loaded, a dword at a time
template <typename E, int VEC>
__device__ __forceinline__ void x16_step(X16State<VEC>& st, const typename Lane<E, VEC>::raw_t& r, int e, unsigned flip2) {
#pragma unroll
  for (int w = 0; w < VEC / 2; ++w) {
    float lo, hi;
    x16_widen<E>(rword(r, w) ^ flip2, lo, hi);
    st.scan(lo, e, 2 * w);
    st.scan(hi, e, 2 * w + 1);
  }
}

// the 16 bits of winner (v, p) at column c: +0 without an entry; an fp16 NaN is read again where it came from
template <typename E>
__device__ __forceinline__ unsigned x16_own_bits(const XArgs& xa, float v, int p, int c) {
  if (p == kNone) return 0u;
  unsigned h = x16_narrow<E>(xflip(v, xa.flip));
  if constexpr (std::is_same<E, F16>::value) {
    if (v != v) h = reinterpret_cast<const unsigned short*>(xa.p.X)[(size_t)xa.p.col[p] * xa.p.ldx + c];
  }
  return h;
}

template <int VEC> __device__ __forceinline__ void x16_store_ints(int* p, const int* v) {
#pragma unroll
  for (int h = 0; h < VEC; h += 4) {
    typename IntV<4>::type o;
#pragma unroll
    for (int q = 0; q < 4; ++q) iset(o, q, v[h + q]);
    istore<4>(p + h, o);
  }
}

// Result of a whole row (slot < 0, row >= 0): 16-bit Z and arg; or of one partial slot (slot >= 0): fp32 values and positions;
// row < 0 and slot < 0: a lane group without a task
template <typename E, int VEC>
__device__ __forceinline__ void x16_store(const XArgs& xa, int row, int slot, int c, const X16State<VEC>& st) {
  if (slot >= 0) {
    const size_t at = (size_t)slot * (size_t)xa.p.D + c;
#pragma unroll
    for (int h = 0; h < VEC; h += 4) {
      f32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = st.bv[h + q];
      Lane<F32, 4>::store_partial(xa.p.partial + at + h, o);
    }
    x16_store_ints<VEC>(xa.ppos + at, st.bp);
    return;
  }
  if (row < 0) return;
  typename Lane<E, VEC>::raw_t out;
  int pos[VEC];
#pragma unroll
  for (int w = 0; w < VEC / 2; ++w) {
    rset(out, w, x16_own_bits<E>(xa, st.bv[2 * w], st.bp[2 * w], c + 2 * w) |
                     (x16_own_bits<E>(xa, st.bv[2 * w + 1], st.bp[2 * w + 1], c + 2 * w + 1) << 16));
    pos[2 * w] = st.bp[2 * w] == kNone ? -1 : st.bp[2 * w];
    pos[2 * w + 1] = st.bp[2 * w + 1] == kNone ? -1 : st.bp[2 * w + 1];
  }
  __builtin_nontemporal_store(out, reinterpret_cast<typename MemU32<VEC / 2>::type*>(
                                       reinterpret_cast<unsigned short*>(xa.p.Z) + (size_t)row * xa.p.ldz + c));
  if (xa.arg != nullptr) x16_store_ints<VEC>(xa.arg + (size_t)row * xa.ldarg + c, pos);
}

// One branch-free batch of UB row gathers, kept raw: lanes past a task's end hold idx -1, re-read row 0 and take nothing
template <typename E, int VEC, int UB>
__device__ __forceinline__ void x16_batch(const XArgs& xa, int csafe, bool cok, int myidx, int src0, int ebase, unsigned flip2,
                                          X16State<VEC>& st) {
  typedef Lane<E, VEC> Ln;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(xa.p.X);
  int idx[UB];
  typename Ln::raw_t v[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = __shfl(myidx, src0 + u, 64);
#pragma unroll
  for (int u = 0; u < UB; ++u) v[u] = Ln::load(X + (size_t)max(idx[u], 0) * xa.p.ldx + csafe);
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (cok && idx[u] >= 0) x16_step<E, VEC>(st, v[u], ebase + u, flip2);
}

// L lanes own the task = entries [e0, e0 + n) (row < 0 and slot < 0: a lane group without a task); WIDE: the whole wave owns it,
// lane group g scanning entries g*L ... g*L + L - 1 of every 64, and the 64/L group winners meet in the fixed xor-shuffle tree
template <typename E, int L, int VEC, bool WIDE>
__device__ __forceinline__ void x16_task(const XArgs& xa, int row, int slot, int e0, int n, int c0, int cend, int lane) {
  constexpr int U = (L < HCSPMM_SPARSE_U) ? L : HCSPMM_SPARSE_U;
  constexpr int STRIDE = WIDE ? 64 : L;
  const int* __restrict__ col = xa.p.col;
  const unsigned flip2 = xa.flip | (xa.flip >> 16);
  const int s = lane & (L - 1);
  const int pos = WIDE ? lane : s;
  const int gbase = lane & ~(L - 1);
  const int first = WIDE ? gbase : 0;  // the first entry this lane group scans, if the task reaches it
  int nmax = n;
  if (!WIDE) {
#pragma unroll
    for (int off = L; off < 64; off <<= 1) nmax = max(nmax, __shfl_xor(nmax, off, 64));
  }
  nmax = __builtin_amdgcn_readfirstlane(nmax);

  for (int pbase = c0; pbase < cend; pbase += L * VEC) {
    const bool cok = pbase + s * VEC < cend;
    const int c = cok ? lane_col<VEC>(pbase + s * VEC, cend) : 0;
    X16State<VEC> st;
    int next = pos < n ? col[e0 + pos] : -1;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      next = base + STRIDE + pos < n ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      const int cnt = min(L, nmax - base);
      const int ebase = e0 + base + first;
      for (int j = 0; j < cnt;) {
        const int left = cnt - j;
        if (left > U / 2) {
          x16_batch<E, VEC, U>(xa, c, cok, myidx, gbase + j, ebase + j, flip2, st);
          j += U;
        } else if (U >= 8 && left > U / 4) {
          x16_batch<E, VEC, (U >= 8 ? U / 2 : 1)>(xa, c, cok, myidx, gbase + j, ebase + j, flip2, st);
          j += U / 2;
        } else if (U >= 4 && left > 1) {
          x16_batch<E, VEC, (U >= 8 ? U / 4 : 2)>(xa, c, cok, myidx, gbase + j, ebase + j, flip2, st);
          j += (U >= 8 ? U / 4 : 2);
        } else {
          x16_batch<E, VEC, 1>(xa, c, cok, myidx, gbase + j, ebase + j, flip2, st);
          j += 1;
        }
      }
    }
    if (first < n) st.settle(e0 + first);
    if (WIDE) {
#pragma unroll
      for (int off = L; off < 64; off <<= 1) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) st.take(__shfl_xor(st.bv[q], off, 64), __shfl_xor(st.bp[q], off, 64), q);
      }
    }
    if (cok && (!WIDE || lane < L)) x16_store<E, VEC>(xa, row, slot, c, st);
  }
}

// T tasks of at most two entries per lane group, column ids inline in the descriptor: 2 T raw loads in flight; the entry position
// comes from rowptr (a whole row) or the fix-up list (the last segment of a split row)
template <typename E, int L, int VEC, int T>
__device__ __forceinline__ void x16_tiny(const XArgs& xa, int first, int c0, int cend, int lane) {
  typedef Lane<E, VEC> Ln;
  const PlanArgs& a = xa.p;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(a.X);
  const unsigned flip2 = xa.flip | (xa.flip >> 16);
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
    if (d[t].y >= 0) e[t] = d[t].x >= 0 ? xa.rowptr[d[t].x] : segment_entry(a, xa.rowptr, xa.segment_len, -(d[t].x + 1));
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
      X16State<VEC> st;
      if (d[t].y >= 0) {
        x16_step<E, VEC>(st, v0[t], e[t], flip2);
        if (d[t].w >= 0) x16_step<E, VEC>(st, v1[t], e[t] + 1, flip2);
        st.settle(e[t]);
      }
      if (cok && d[t].z >= 0) x16_store<E, VEC>(xa, d[t].x, d[t].x >= 0 ? -1 : -(d[t].x + 1), c, st);
    }
  }
}

// what csr_schedule.h's walks call
template <typename E, int L, int VEC> struct X16Body {
  const XArgs& xa;
  typedef RowSlot Dst;  // x16_store finds the place
  __device__ __forceinline__ Dst dst(int row, int slot) const { return Dst{row, slot}; }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    x16_task<E, L, VEC, WIDE>(xa, o.row, o.slot, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    x16_tiny<E, L, VEC, XTinyT<L>::value>(xa, first, c0, cend, lane);
  }
};

// the planned and the plan-free kernel (csr_schedule.h)
template <typename E, int L, int VEC>
__global__ __launch_bounds__(kThreads, kX16MinWaves) void extremum16_plan_kernel(XArgs xa) {
  csr_plan_walk<L, XTinyT<L>::value>(xa.p, xa.rowptr, X16Body<E, L, VEC>{xa});
}
template <typename E, int L, int VEC>
__global__ __launch_bounds__(kThreads, kX16MinWaves) void extremum16_window_kernel(XArgs xa) {
  csr_window_walk<L>(xa.p, xa.rowptr, X16Body<E, L, VEC>{xa});
}

// Fix-up: Z[row] and arg[row] of a split row = the best of its partial (fp32 value, position) pairs -- one wave per row at four
// columns per lane (the slots are fp32 whatever the panel's lanes were), the 64/L lane groups taking every (64/L)-th slot, four
// slots in flight per lane, combined by the xor-shuffle tree; the winners are stored as 16-bit Z
template <typename E>
__global__ __launch_bounds__(kThreads) void extremum16_fixup_kernel(XArgs xa) {
  constexpr int VEC = 4;
  const PlanArgs& a = xa.p;
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
    const size_t at = (size_t)s0 * (size_t)a.D + c;
    X16State<VEC> st;
    int s = g;
    for (; s + 3 * R < ns; s += 4 * R) {
      f32x4 v[4];
      typename IntV<VEC>::type pp[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = Lane<F32, VEC>::load_partial(a.partial + at + (size_t)(s + u * R) * (size_t)a.D);
        pp[u] = iload<VEC>(xa.ppos + at + (size_t)(s + u * R) * (size_t)a.D);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) st.take(v[u][q], pp[u][q], q);
      }
    }
    for (; s < ns; s += R) {
      const f32x4 v = Lane<F32, VEC>::load_partial(a.partial + at + (size_t)s * (size_t)a.D);
      const typename IntV<VEC>::type pp = iload<VEC>(xa.ppos + at + (size_t)s * (size_t)a.D);
#pragma unroll
      for (int q = 0; q < VEC; ++q) st.take(v[q], pp[q], q);
    }
    for (int off = L; off < 64; off <<= 1) {
#pragma unroll
      for (int q = 0; q < VEC; ++q) st.take(__shfl_xor(st.bv[q], off, 64), __shfl_xor(st.bp[q], off, 64), q);
    }
    if (cok && g == 0) x16_store<E, VEC>(xa, row, -1, c, st);
  }
}

template <typename E, int L, int VEC> hipError_t x16_launch(const XArgs& a, hipStream_t stream) {
  return csr_launch(a, L, XTinyT<L>::value, extremum16_window_kernel<E, L, VEC>, extremum16_plan_kernel<E, L, VEC>,
                    extremum16_fixup_kernel<E>, stream);
}

// The unit's own dispatch (csr_dispatch serves 4-element lanes and narrower): 8 elements per lane and L = pick_L of the panel
// (planned) or of D (plan-free) from 32 columns on, 4 elements per lane with L = 4 or 8 below
template <typename E> hipError_t x16_dispatch(const XArgs& a, hipStream_t stream) {
  const int width = a.p.plan != nullptr ? a.p.panel_cols : a.p.D;
  if (a.p.D < 4 || ((a.p.D | width) & 1)) return hipErrorInvalidValue;
  if (width >= 32) {
    switch (pick_L(width, 8)) {
      case 4: return x16_launch<E, 4, 8>(a, stream);
      case 8: return x16_launch<E, 8, 8>(a, stream);
      case 16: return x16_launch<E, 16, 8>(a, stream);
      case 32: return x16_launch<E, 32, 8>(a, stream);
      default: return x16_launch<E, 64, 8>(a, stream);
    }
  }
  return pick_L(width, 4) == 4 ? x16_launch<E, 4, 4>(a, stream) : x16_launch<E, 8, 4>(a, stream);
}

}  // namespace

hipError_t launch_extremum16(const XArgs& a, int dtype, hipStream_t stream) {
  if (dtype == HCSPMM_DTYPE_F16) return x16_dispatch<F16>(a, stream);
  if (dtype == HCSPMM_DTYPE_BF16) return x16_dispatch<BF16>(a, stream);
  return hipErrorInvalidValue;
}

}  // namespace hcspmm
