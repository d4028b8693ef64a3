// spmm_multi16.hip -- sum, sum of squares, max and min of each row's neighbours with both argmaxes in ONE gather pass over fp16 /
// bf16 features (the 16-bit dtypes of hcspmm_forward_multi_typed):
//   Z_sum[r][d] = sum x_e    Z_sumsq[r][d] = sum fl(x_e * x_e)        fp32, x_e = the widened X[col(e)][d]
//   Z_max / Z_min[r][d] = the 16 bits of the winning X[col(e)][d]     arg_max / arg_min[r][d] = the winning e (int32)
// The sums follow spmm_multi.hip's contract (CSR order inside a lane group, the fixed xor-shuffle tree on wide tasks, slot order
// then the tree in the fix-up; the square rounded by __fmul_rn before it is added -- it is exact wherever it is representable, a
// 16-bit value has at most 11 significant bits), the extrema spmm_extremum16.hip's (extremum_common.h's order on the widened
// values, the winner's own bits stored, an fp16 NaN winner read again where it came from).  The sums stay fp32 in memory: an fp16
// sum of squares overflows on any hub, and sumsq / deg - mean^2 cancels on a 16-bit mean.
//
// Lanes.  Rows sit on the dword grid (even width, even strides, 4-byte aligned bases): a lane owns 8 columns -- one 16-byte load
// per gathered row -- from 32 columns per panel on and 4 columns (8-byte loads) below, a lane past a ragged end moved back onto
// the last ones (lane_col).  The loads of a batch stay RAW dwords and a dword is widened where it is used, both halves at once (a
// bf16 pair by a shift and a mask, an fp16 pair by one conversion per half); the one widened value feeds all four reductions.
// Registers.  The state is six vectors -- s, q, max value and entry, NEGATED-min value and entry -- 48 registers at 8 columns, so
// the budget is the unit's main design problem (the table is in DESIGN 3.17b; every build keeps eight raw loads in flight at four
// waves per SIMD or better without scratch).
// Compare.  A lane scans its entries in rising CSR position, so a later entry wins only by being strictly better:
//   win = !(v <= best) && best == best
// and a scan that saw entries and took none saw only -inf (min: +inf): settle() gives it its first entry.  Where positions do
// not rise -- the wide tasks' tree, the fix-up's slots -- the full order xbeats decides.
// Split rows keep spmm_multi.hip's six fp32 / int32 areas (hcspmm_multi_workspace_bytes); the unit's own fix-up combines them.
// One build computes all four; which are stored is a run-time matter (a null output is skipped).  No atomics.
#include "csr_schedule.h"
#include "extremum_common.h"  // xbeats, xflip, kNone, XTinyT, the int32 lane vectors

namespace hcspmm {
namespace {

constexpr int kM16MinWaves = 4;  // 128 registers per lane
constexpr unsigned kSign = 0x80000000u;

// Row gathers in flight per lane: the binary path's eight in every build.  At 8 columns that is 32 registers of raw loads next to
// the 48 of state, and it fits the 128 of four waves per SIMD once the scan has ONE batch shape and no branch (m16_task, scan)
template <int L> struct M16U {
  static constexpr int value = L < HCSPMM_SPARSE_U ? L : HCSPMM_SPARSE_U;
};

// the two 16-bit elements of a dword, widened (exact)
template <typename E> __device__ __forceinline__ void m16_widen(unsigned w, float& lo, float& hi);
template <> __device__ __forceinline__ void m16_widen<BF16>(unsigned w, float& lo, float& hi) {
  lo = __uint_as_float(w << 16);
  hi = __uint_as_float(w & 0xffff0000u);
}
template <> __device__ __forceinline__ void m16_widen<F16>(unsigned w, float& lo, float& hi) {
  lo = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
  hi = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
}
// a widened value back to its 16 bits (exact, but fp16 NaNs: m16_own_bits)
template <typename E> __device__ __forceinline__ unsigned m16_narrow(float f);
template <> __device__ __forceinline__ unsigned m16_narrow<BF16>(float f) { return __float_as_uint(f) >> 16; }
template <> __device__ __forceinline__ unsigned m16_narrow<F16>(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }

// per-lane state of VEC columns: the two sums, the best value and entry of the max, the best NEGATED value and entry of the min
template <int VEC> struct M16State {
  float s[VEC], q[VEC], xv[VEC], nv[VEC];
  int xp[VEC], np[VEC];
  __device__ __forceinline__ M16State() {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      s[i] = q[i] = 0.0f;
      xv[i] = nv[i] = -__builtin_inff();
      xp[i] = np[i] = kNone;
    }
  }
  // One gathered element at entry e, e after every entry this state has seen.  ok: the lane has this entry -- a condition on
  // each update, not a branch around the scan: behind a divergent branch the compiler keeps a second copy of the 48 state
  // registers.  Without the entry the sums take +0, which leaves them as they are (a sum never holds -0)
  __device__ __forceinline__ void scan(float v, int e, int i, bool ok) {
    {
#pragma clang fp contract(off)  // the square is rounded before it is added
      const float a = ok ? v : 0.0f;
      s[i] += a;
      q[i] += __fmul_rn(a, a);
    }
    if (ok && !(v <= xv[i]) && xv[i] == xv[i]) {
      xv[i] = v;
      xp[i] = e;
    }
    const float m = xflip(v, kSign);
    if (ok && !(m <= nv[i]) && nv[i] == nv[i]) {
      nv[i] = m;
      np[i] = e;
    }
  }
  // after a scan that saw entries, `first` the first of them: columns that took none saw -inf (min: +inf) only
  __device__ __forceinline__ void settle(int first) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      xp[i] = xp[i] == kNone ? first : xp[i];
      np[i] = np[i] == kNone ? first : np[i];
    }
  }
  // another partial result of the same row and column: the full order
  __device__ __forceinline__ void merge(float os, float oq, float mx, int mxp, float mn, int mnp, int i) {
    s[i] += os;
    q[i] += oq;
    if (xbeats(mx, mxp, xv[i], xp[i])) {
      xv[i] = mx;
      xp[i] = mxp;
    }
    if (xbeats(mn, mnp, nv[i], np[i])) {
      nv[i] = mn;
      np[i] = mnp;
    }
  }
  // column i against the same column of the lane `off` away
  __device__ __forceinline__ void meet(int off, int i) {
    merge(__shfl_xor(s[i], off, 64), __shfl_xor(q[i], off, 64), __shfl_xor(xv[i], off, 64), __shfl_xor(xp[i], off, 64),
          __shfl_xor(nv[i], off, 64), __shfl_xor(np[i], off, 64), i);
  }
};

// the 64 / L lane-group states of a wave into every group, by the fixed xor-shuffle tree.  A column's six shuffles and merges are
// kept together: issued level by level, the 48 shuffle results sit next to the 48 state registers and the wide builds spill
template <int L, int VEC> __device__ __forceinline__ void m16_tree(M16State<VEC>& st) {
#pragma unroll
  for (int off = L; off < 64; off <<= 1) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      st.meet(off, i);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// one gathered row at entry e: VEC columns as loaded, a dword at a time
template <typename E, int VEC>
__device__ __forceinline__ void m16_step(M16State<VEC>& st, const typename Lane<E, VEC>::raw_t& r, int e, bool ok) {
#pragma unroll
  for (int w = 0; w < VEC / 2; ++w) {
    float lo, hi;
    m16_widen<E>(rword(r, w), lo, hi);
    st.scan(lo, e, 2 * w, ok);
    st.scan(hi, e, 2 * w + 1, ok);
  }
}

// the 16 bits of the winner v at entry p, column c: +0 without an entry; an fp16 NaN is read again where it came from
template <typename E> __device__ __forceinline__ unsigned m16_own_bits(const M16Args& ma, float v, int p, int c) {
  if (p == kNone) return 0u;
  unsigned h = m16_narrow<E>(v);
  if constexpr (std::is_same<E, F16>::value) {
    if (v != v) h = reinterpret_cast<const unsigned short*>(ma.p.X)[(size_t)ma.p.col[p] * ma.p.ldx + c];
  }
  return h;
}

// VEC floats / ints to memory, 16 bytes at a time
template <int VEC, bool PARTIAL> __device__ __forceinline__ void m16_store_f32(float* p, const float* v) {
#pragma unroll
  for (int h = 0; h < VEC; h += 4) {
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = v[h + i];
    if (PARTIAL) Lane<F32, 4>::store_partial(p + h, o);
    else Lane<F32, 4>::store(p + h, o);
  }
}
template <int VEC> __device__ __forceinline__ void m16_store_ints(int* p, const int* v) {
#pragma unroll
  for (int h = 0; h < VEC; h += 4) {
    typename IntV<4>::type o;
#pragma unroll
    for (int i = 0; i < 4; ++i) iset(o, i, v[h + i]);
    istore<4>(p + h, o);
  }
}

// Result of a whole row (slot < 0, row >= 0): fp32 sums, 16-bit extrema, int32 args; or of one partial slot (slot >= 0): the six
// fp32 / int32 areas; row < 0 and slot < 0: a lane group without a task.  Rows without entries: +0 in the four values (the sums
// are +0 already), -1 in both args
template <typename E, int VEC>
__device__ __forceinline__ void m16_store(const M16Args& ma, int row, int slot, int c, const M16State<VEC>& st) {
  if (slot >= 0) {
    float* p = ma.p.partial + (size_t)slot * (size_t)ma.p.D + c;
    m16_store_f32<VEC, true>(p, st.s);
    m16_store_f32<VEC, true>(p + ma.area, st.q);
    m16_store_f32<VEC, true>(p + 2 * ma.area, st.xv);
    m16_store_ints<VEC>(reinterpret_cast<int*>(p + 3 * ma.area), st.xp);
    m16_store_f32<VEC, true>(p + 4 * ma.area, st.nv);
    m16_store_ints<VEC>(reinterpret_cast<int*>(p + 5 * ma.area), st.np);
    return;
  }
  if (row < 0) return;
  typedef typename MemU32<VEC / 2>::type mem_t;
  const size_t so = (size_t)row * ma.ldsum + c, zo = (size_t)row * ma.p.ldz + c, ao = (size_t)row * ma.ldarg + c;
  if (ma.zsum != nullptr) m16_store_f32<VEC, false>(ma.zsum + so, st.s);
  if (ma.zsumsq != nullptr) m16_store_f32<VEC, false>(ma.zsumsq + so, st.q);
  if (ma.zmax != nullptr) {
    typename Lane<E, VEC>::raw_t out;
#pragma unroll
    for (int w = 0; w < VEC / 2; ++w)
      rset(out, w, m16_own_bits<E>(ma, st.xv[2 * w], st.xp[2 * w], c + 2 * w) |
                       (m16_own_bits<E>(ma, st.xv[2 * w + 1], st.xp[2 * w + 1], c + 2 * w + 1) << 16));
    __builtin_nontemporal_store(out, reinterpret_cast<mem_t*>(reinterpret_cast<unsigned short*>(ma.zmax) + zo));
  }
  if (ma.zmin != nullptr) {
    typename Lane<E, VEC>::raw_t out;
#pragma unroll
    for (int w = 0; w < VEC / 2; ++w)
      rset(out, w, m16_own_bits<E>(ma, xflip(st.nv[2 * w], kSign), st.np[2 * w], c + 2 * w) |
                       (m16_own_bits<E>(ma, xflip(st.nv[2 * w + 1], kSign), st.np[2 * w + 1], c + 2 * w + 1) << 16));
    __builtin_nontemporal_store(out, reinterpret_cast<mem_t*>(reinterpret_cast<unsigned short*>(ma.zmin) + zo));
  }
  if (ma.amax != nullptr || ma.amin != nullptr) {
    int px[VEC], pn[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      px[i] = st.xp[i] == kNone ? -1 : st.xp[i];
      pn[i] = st.np[i] == kNone ? -1 : st.np[i];
    }
    if (ma.amax != nullptr) m16_store_ints<VEC>(ma.amax + ao, px);
    if (ma.amin != nullptr) m16_store_ints<VEC>(ma.amin + ao, pn);
  }
}

// One branch-free batch of UB row gathers, kept raw: lanes past a task's end hold idx -1, re-read row 0 and take nothing
template <typename E, int VEC, int UB>
__device__ __forceinline__ void m16_batch(const M16Args& ma, int csafe, bool cok, int myidx, int src0, int left, int ebase,
                                          M16State<VEC>& st) {
  typedef Lane<E, VEC> Ln;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(ma.p.X);
  int idx[UB];
  typename Ln::raw_t v[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) idx[u] = u < left ? __shfl(myidx, src0 + u, 64) : -1;
#pragma unroll
  for (int u = 0; u < UB; ++u) v[u] = Ln::load(X + (size_t)max(idx[u], 0) * ma.p.ldx + csafe);
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    m16_step<E, VEC>(st, v[u], ebase + u, cok && idx[u] >= 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// L lanes own the task = entries [e0, e0 + n) (row < 0 and slot < 0: a lane group without a task); WIDE: the whole wave owns it,
// lane group g scanning entries g*L ... g*L + L - 1 of every 64, and the 64/L group results meet in the fixed xor-shuffle tree
template <typename E, int L, int VEC, bool WIDE>
__device__ __forceinline__ void m16_task(const M16Args& ma, int row, int slot, int e0, int n, int c0, int cend, int lane) {
  constexpr int U = M16U<L>::value;
  constexpr int STRIDE = WIDE ? 64 : L;
  const int* __restrict__ col = ma.p.col;
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
    M16State<VEC> st;
    int next = pos < n ? col[e0 + pos] : -1;
    for (int base = 0; base < nmax; base += STRIDE) {
      const int myidx = next;
      next = base + STRIDE + pos < n ? col[e0 + base + STRIDE + pos] : -1;  // the next chunk's indices arrive under this chunk's gathers
      const int cnt = min(L, nmax - base);
      const int ebase = e0 + base + first;
      // one batch shape: a tail's missing entries are idx -1 like a shorter neighbour's (three batch sizes are three code paths
      // that meet at the loop's head, each with its own copy of the state)
      for (int j = 0; j < cnt; j += U) m16_batch<E, VEC, U>(ma, c, cok, myidx, gbase + j, cnt - j, ebase + j, st);
    }
    if (first < n) st.settle(e0 + first);
    if (WIDE) m16_tree<L, VEC>(st);
    // the store addresses are worked out here, behind the scan: hoisted above it they are up to seven 64-bit values per lane
    // next to the state, and every 8-column build spilled them
    int cs = c, rs = row;
    asm volatile("" : "+v"(cs), "+v"(rs));
    if (cok && (!WIDE || lane < L)) m16_store<E, VEC>(ma, rs, slot, cs, st);
  }
}

// T tasks of at most two entries per lane group, column ids inline in the descriptor: 2 T raw loads in flight; the entry position
// comes from rowptr (a whole row) or the fix-up list (the last segment of a split row)
template <typename E, int L, int VEC, int T>
__device__ __forceinline__ void m16_tiny(const M16Args& ma, int first, int c0, int cend, int lane) {
  typedef Lane<E, VEC> Ln;
  const PlanArgs& a = ma.p;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(a.X);
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
    if (d[t].y >= 0) e[t] = d[t].x >= 0 ? ma.rowptr[d[t].x] : segment_entry(a, ma.rowptr, ma.segment_len, -(d[t].x + 1));
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
      M16State<VEC> st;
      if (d[t].y >= 0) {
        m16_step<E, VEC>(st, v0[t], e[t], true);
        if (d[t].w >= 0) m16_step<E, VEC>(st, v1[t], e[t] + 1, true);
        st.settle(e[t]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (cok && d[t].z >= 0) m16_store<E, VEC>(ma, d[t].x, d[t].x >= 0 ? -1 : -(d[t].x + 1), c, st);
    }
  }
}

// what csr_schedule.h's walks call
template <typename E, int L, int VEC> struct M16Body {
  const M16Args& ma;
  typedef RowSlot Dst;  // m16_store finds the place
  __device__ __forceinline__ Dst dst(int row, int slot) const { return Dst{row, slot}; }
  template <bool WIDE> __device__ __forceinline__ void task(const Dst& o, int e0, int n, int c0, int cend, int lane) const {
    m16_task<E, L, VEC, WIDE>(ma, o.row, o.slot, e0, n, c0, cend, lane);
  }
  __device__ __forceinline__ void tiny(int first, int c0, int cend, int lane) const {
    m16_tiny<E, L, VEC, XTinyT<L>::value>(ma, first, c0, cend, lane);
  }
};

// the planned and the plan-free kernel (csr_schedule.h)
template <typename E, int L, int VEC>
__global__ __launch_bounds__(kThreads, kM16MinWaves) void multi16_plan_kernel(M16Args ma) {
  csr_plan_walk<L, XTinyT<L>::value>(ma.p, ma.rowptr, M16Body<E, L, VEC>{ma});
}
template <typename E, int L, int VEC>
__global__ __launch_bounds__(kThreads, kM16MinWaves) void multi16_window_kernel(M16Args ma) {
  csr_window_walk<L>(ma.p, ma.rowptr, M16Body<E, L, VEC>{ma});
}

// Fix-up: the six results of a split row from its partial slots -- one wave per row at four columns per lane (the slots are fp32
// whatever the panel's lanes were), the 64/L lane groups taking every (64/L)-th slot in slot order, two slots (twelve loads) in
// flight per lane, combined by the xor-shuffle tree; fp32 sums and 16-bit extrema are stored
template <typename E>
__global__ __launch_bounds__(kThreads) void multi16_fixup_kernel(M16Args ma) {
  constexpr int VEC = 4;
  typedef Lane<F32, VEC> Ln;
  const PlanArgs& a = ma.p;
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
    M16State<VEC> st;
    int s = g;
    for (; s + R < ns; s += 2 * R) {
      f32x4 vs[2], vq[2], vx[2], vn[2];
      typename IntV<VEC>::type px[2], pn[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float* p = at + (size_t)(s + u * R) * (size_t)a.D;
        vs[u] = Ln::load_partial(p);
        vq[u] = Ln::load_partial(p + ma.area);
        vx[u] = Ln::load_partial(p + 2 * ma.area);
        px[u] = iload<VEC>(reinterpret_cast<const int*>(p + 3 * ma.area));
        vn[u] = Ln::load_partial(p + 4 * ma.area);
        pn[u] = iload<VEC>(reinterpret_cast<const int*>(p + 5 * ma.area));
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) st.merge(vs[u][i], vq[u][i], vx[u][i], px[u][i], vn[u][i], pn[u][i], i);
      }
    }
    for (; s < ns; s += R) {
      const float* p = at + (size_t)s * (size_t)a.D;
      const f32x4 vs = Ln::load_partial(p), vq = Ln::load_partial(p + ma.area), vx = Ln::load_partial(p + 2 * ma.area),
                  vn = Ln::load_partial(p + 4 * ma.area);
      const typename IntV<VEC>::type px = iload<VEC>(reinterpret_cast<const int*>(p + 3 * ma.area)),
                                     pn = iload<VEC>(reinterpret_cast<const int*>(p + 5 * ma.area));
#pragma unroll
      for (int i = 0; i < VEC; ++i) st.merge(vs[i], vq[i], vx[i], px[i], vn[i], pn[i], i);
    }
    for (int off = L; off < 64; off <<= 1) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) st.meet(off, i);
    }
    if (cok && g == 0) m16_store<E, VEC>(ma, row, -1, c, st);
  }
}

template <typename E, int L, int VEC> hipError_t m16_launch(const M16Args& a, hipStream_t stream) {
  return csr_launch(a, L, XTinyT<L>::value, multi16_window_kernel<E, L, VEC>, multi16_plan_kernel<E, L, VEC>,
                    multi16_fixup_kernel<E>, stream);
}

// The unit's own dispatch (csr_dispatch serves 4-element lanes and narrower): 8 elements per lane and L = pick_L of the panel
// (planned) or of D (plan-free) from 32 columns on, 4 elements per lane with L = 4 or 8 below
template <typename E> hipError_t m16_dispatch(const M16Args& a, hipStream_t stream) {
  const int width = a.p.plan != nullptr ? a.p.panel_cols : a.p.D;
  if (a.p.D < 4 || ((a.p.D | width) & 1)) return hipErrorInvalidValue;
  if (width >= 32) {
    switch (pick_L(width, 8)) {
      case 4: return m16_launch<E, 4, 8>(a, stream);
      case 8: return m16_launch<E, 8, 8>(a, stream);
      case 16: return m16_launch<E, 16, 8>(a, stream);
      case 32: return m16_launch<E, 32, 8>(a, stream);
      default: return m16_launch<E, 64, 8>(a, stream);
    }
  }
  return pick_L(width, 4) == 4 ? m16_launch<E, 4, 4>(a, stream) : m16_launch<E, 8, 4>(a, stream);
}

}  // namespace

hipError_t launch_multi16(const M16Args& a, int dtype, hipStream_t stream) {
  if (dtype == HCSPMM_DTYPE_F16) return m16_dispatch<F16>(a, stream);
  if (dtype == HCSPMM_DTYPE_BF16) return m16_dispatch<BF16>(a, stream);
  return hipErrorInvalidValue;
}

}  // namespace hcspmm
