// sddmm_impl.h -- gfx950 device code of the kernels that produce and differentiate edge values (include/hcspmm.h
// hcspmm_sddmm, hcspmm_edge_softmax, hcspmm_edge_softmax_backward).  Instantiated by sddmm.hip.
//
//  * SDDMM  out[e] = <A[row(e)], B[col(e)]>: edge-parallel over contiguous CSR chunks, one chunk per wave, so a power-law
//    row is cut wherever the chunks fall and no entry needs a fix-up.  L lanes own one entry (64/L entries per wave step),
//    each lane VEC elements through the forward's element-aligned 16-byte lanes (spmm_impl.h Lane / lane_col); the row of
//    A stays in registers while a lane group's entries stay in one row.  Per entry: each lane sums its own elements in
//    column order with fmaf, then a fixed xor-butterfly over the L lanes -- a fixed order, so every call gives the same
//    bits; every entry is written by exactly one lane, no atomics.
//  * Edge softmax over [heads][E]: one thread per row up to kShortRow entries, one wave per row up to kBlockRow, the
//    whole workgroup beyond (a hub of 10^5 entries is 400 elements per thread).  Each row's result comes from one fixed
//    procedure whatever thread, wave or workgroup runs it: deterministic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_impl.h"

namespace hcspmm {

// ---------------------------------------------------------------- SDDMM
constexpr int kSddmmThreads = 256;
constexpr int kSddmmUnroll = 4;  // entries per lane group per step: four gathers in flight before the first reduction
constexpr int kSddmmSteps = 8;   // steps per wave: a chunk is 8 * 4 * (64 / L) entries (32 was measured: -10 % at L = 32, +21 % at L = 8)

// largest r with rowptr[r] <= e (rows without entries never win: the search looks for the LAST such row)
__device__ __forceinline__ int row_of(const int* __restrict__ rowptr, int N, long long e) {
  int lo = 0, hi = N;  // invariant: rowptr[lo] <= e < rowptr[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)rowptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

// acc += sum over the lane's own columns of a * b, in column order; a lane moved back by lane_col skips the columns its
// left neighbour owns, a lane past the row's end adds nothing
template <typename E, int VEC>
__device__ __forceinline__ float lane_dot(const typename Lane<E, VEC>::raw_t& a, const typename Lane<E, VEC>::raw_t& b, int skip,
                                          float acc) {
#pragma unroll
  for (int q = 0; q < VEC; ++q)
    if (q >= skip) acc = fmaf(Lane<E, VEC>::elem(a, q), Lane<E, VEC>::elem(b, q), acc);
  return acc;
}

template <typename E, int L, int VEC>
__global__ __launch_bounds__(kSddmmThreads) void sddmm_kernel(SddmmArgs a) {
  typedef typename E::T T;
  typedef Lane<E, VEC> LN;
  typedef typename LN::raw_t raw_t;
  constexpr int G = 64 / L;                          // lane groups (entries) per wave step
  constexpr long long kChunk = (long long)kSddmmSteps * kSddmmUnroll * G;
  const int lane = threadIdx.x & 63, g = lane / L, sub = lane % L;
  const long long wave = ((long long)blockIdx.x * kSddmmThreads + threadIdx.x) >> 6;
  const long long e0 = wave * kChunk;
  if (e0 >= a.E) return;
  const long long e1 = min(e0 + kChunk, a.E);
  const T* __restrict__ A = reinterpret_cast<const T*>(a.A);
  const T* __restrict__ B = reinterpret_cast<const T*>(a.B);
  const int D = a.D;
  // chunk 0 of this lane: columns [c, c + VEC) of the row (moved back onto the row's last VEC when they would run past it)
  const int c = sub * VEC, c0 = lane_col<VEC>(c, D), skip = c - c0;
  const bool live = c < D;
  const int n_chunks = (D + L * VEC - 1) / (L * VEC);  // > 1 only for L = 64 and D > 64 * VEC: later chunks read A again
  long long e = e0 + g;
  int r = row_of(a.rowptr, a.N, e < e1 ? e : e0);
  int next = a.rowptr[r + 1];
  int ra = -1;  // row whose chunk 0 sits in `ar`
  raw_t ar = LN::zero();
  for (; e < e1; e += G * kSddmmUnroll) {
    int rows[kSddmmUnroll], cols[kSddmmUnroll];
    raw_t bv[kSddmmUnroll], av[kSddmmUnroll];
#pragma unroll
    for (int u = 0; u < kSddmmUnroll; ++u) {  // rows (a cursor: a group's entries ascend) and column ids
      const long long eu = e + (long long)u * G;
      rows[u] = -1;
      if (eu < e1) {
        while (next <= eu) next = a.rowptr[++r + 1];
        rows[u] = r;
        cols[u] = a.col[eu];
      }
    }
#pragma unroll
    for (int u = 0; u < kSddmmUnroll; ++u) {  // the gathers, all in flight before any product
      bv[u] = LN::zero();
      av[u] = LN::zero();
      if (rows[u] >= 0 && live) {
        bv[u] = LN::load(B + (size_t)cols[u] * a.ldb + c0);
        const int prev = u == 0 ? ra : rows[u - 1];
        if (rows[u] != prev) av[u] = LN::load(A + (size_t)rows[u] * a.lda + c0);
      }
    }
    float acc[kSddmmUnroll];
#pragma unroll
    for (int u = 0; u < kSddmmUnroll; ++u) {
      acc[u] = 0.f;
      if (rows[u] < 0) continue;
      if (rows[u] != ra) {
        ar = av[u];
        ra = rows[u];
      }
      if (live) acc[u] = lane_dot<E, VEC>(ar, bv[u], skip, 0.f);
      for (int k = 1; k < n_chunks; ++k) {  // wide rows: chunk k of this lane, A re-read (an L1 / L2 hit)
        const int ck = (k * L + sub) * VEC;
        if (ck < D) {
          const int ck0 = lane_col<VEC>(ck, D);
          const raw_t ak = LN::load(A + (size_t)rows[u] * a.lda + ck0);
          const raw_t bk = LN::load(B + (size_t)cols[u] * a.ldb + ck0);
          acc[u] = lane_dot<E, VEC>(ak, bk, ck - ck0, acc[u]);
        }
      }
    }
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1)  // fixed butterfly: every lane of the group ends with the same bits
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u) acc[u] += __shfl_xor(acc[u], off, 64);
    if (sub == 0) {
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u)
        if (rows[u] >= 0) __builtin_nontemporal_store(acc[u], a.out + e + (long long)u * G);
    }
  }
}

template <typename E, int L, int VEC>
hipError_t launch_sddmm_LV(const SddmmArgs& a, hipStream_t stream) {
  constexpr long long kChunk = (long long)kSddmmSteps * kSddmmUnroll * (64 / L);
  const long long waves = (a.E + kChunk - 1) / kChunk;
  const long long blocks = (waves + kSddmmThreads / 64 - 1) / (kSddmmThreads / 64);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sddmm_kernel<E, L, VEC>), dim3((unsigned)blocks), dim3(kSddmmThreads), 0, stream, a);
  return hipGetLastError();
}

// lanes per entry: the fewest powers of two whose VEC-element accesses cover the row, at most a wave
inline int sddmm_L(int D, int vec) {
  const int need = (D + vec - 1) / vec;
  int L = 1;
  while (L < need && L < 64) L <<= 1;
  return L;
}

#define HCSPMM_SDDMM_DISPATCH(E, VEC, ARGS, STREAM)                     \
  switch (sddmm_L((ARGS).D, VEC)) {                                    \
    case 1: return launch_sddmm_LV<E, 1, VEC>(ARGS, STREAM);           \
    case 2: return launch_sddmm_LV<E, 2, VEC>(ARGS, STREAM);           \
    case 4: return launch_sddmm_LV<E, 4, VEC>(ARGS, STREAM);           \
    case 8: return launch_sddmm_LV<E, 8, VEC>(ARGS, STREAM);           \
    case 16: return launch_sddmm_LV<E, 16, VEC>(ARGS, STREAM);         \
    case 32: return launch_sddmm_LV<E, 32, VEC>(ARGS, STREAM);         \
    default: return launch_sddmm_LV<E, 64, VEC>(ARGS, STREAM);         \
  }

// ---------------------------------------------------------------- edge softmax
constexpr int kSoftmaxThreads = 256;
constexpr int kShortRow = 16;    // rows up to this length: one thread each
constexpr int kBlockRow = 2048;  // rows longer than this: the whole workgroup; in between: one wave each

// Forward of one row segment [b, b + n) of head slice x / out, by `nt` cooperating threads of which this is `t`.
// red(v, op) folds a per-thread value over the cooperating threads in a fixed order, the same value to all of them.
//   pass 1: m = max;  pass 2: s = sum exp(x - m);  pass 3: out = exp(x - m) / s  (exp_diff)
// Backward: pass 1: d = sum alpha * grad_alpha;  pass 2: out = alpha * (grad_alpha - d).
// exp(x - m) with the rounding error of the subtraction put back: d + t == x - m exactly (two-sum), exp(d + t) ~ exp(d) (1 + t).
// Without it, logits spread over +-80 lose up to 2^-17 of relative accuracy to the rounding of d alone.
__device__ __forceinline__ float exp_diff(float x, float m) {
  const float d = x - m;
  const float xs = d + m, ms = d - xs;
  const float t = (x - xs) - (m + ms);
  const float ed = expf(d);
  return fmaf(ed, t, ed);
}

template <bool BWD, typename Red>
__device__ __forceinline__ void softmax_row(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out,
                                            long long b, int n, int t, int nt, Red red) {
  if constexpr (!BWD) {
    float m = -INFINITY;
    for (int i = t; i < n; i += nt) m = fmaxf(m, x[b + i]);
    m = red(m, true);
    float s = 0.f;
    for (int i = t; i < n; i += nt) s += exp_diff(x[b + i], m);
    s = red(s, false);
    for (int i = t; i < n; i += nt) out[b + i] = exp_diff(x[b + i], m) / s;
  } else {
    float d = 0.f;
    for (int i = t; i < n; i += nt) d = fmaf(x[b + i], y[b + i], d);
    d = red(d, false);
    for (int i = t; i < n; i += nt) out[b + i] = x[b + i] * (y[b + i] - d);
  }
}

__device__ __forceinline__ float wave_fold(float v, bool is_max) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, 64);
    v = is_max ? fmaxf(v, o) : v + o;
  }
  return v;
}

// Workgroup b covers rows [256 b, 256 b + 256): short rows by their own thread, the others listed in LDS and taken by the
// waves in turn, or by the whole workgroup.  The lists' order depends on timing; no row's result does.
template <bool BWD>
__global__ __launch_bounds__(kSoftmaxThreads) void edge_softmax_kernel(SoftmaxArgs a) {
  __shared__ int wave_rows[kSoftmaxThreads], block_rows[kSoftmaxThreads];
  __shared__ int n_wave, n_block;
  __shared__ float part[kSoftmaxThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) n_wave = n_block = 0;
  __syncthreads();
  const int r = blockIdx.x * kSoftmaxThreads + tid;
  if (r < a.N) {
    const long long b = a.rowptr[r];
    const int n = a.rowptr[r + 1] - (int)b;
    if (n <= kShortRow) {
      for (int h = 0; h < a.heads; ++h) {
        const long long o = (long long)h * a.E;
        softmax_row<BWD>(a.x + o, a.y + o, a.out + o, b, n, 0, 1, [](float v, bool) { return v; });
      }
    } else if (n <= kBlockRow) {
      wave_rows[atomicAdd(&n_wave, 1)] = r;
    } else {
      block_rows[atomicAdd(&n_block, 1)] = r;
    }
  }
  __syncthreads();
  for (int i = wid; i < n_wave; i += kSoftmaxThreads / 64) {
    const int rr = wave_rows[i];
    const long long b = a.rowptr[rr];
    const int n = a.rowptr[rr + 1] - (int)b;
    for (int h = 0; h < a.heads; ++h) {
      const long long o = (long long)h * a.E;
      softmax_row<BWD>(a.x + o, a.y + o, a.out + o, b, n, lane, 64, wave_fold);
    }
  }
  for (int i = 0; i < n_block; ++i) {
    const int rr = block_rows[i];
    const long long b = a.rowptr[rr];
    const int n = a.rowptr[rr + 1] - (int)b;
    auto block_fold = [&](float v, bool is_max) {  // waves fold, then wave partials in wave order
      v = wave_fold(v, is_max);
      __syncthreads();  // (part[] of the previous fold has been read by every thread)
      if (lane == 0) part[wid] = v;
      __syncthreads();
      float w = part[0];
#pragma unroll
      for (int k = 1; k < kSoftmaxThreads / 64; ++k) w = is_max ? fmaxf(w, part[k]) : w + part[k];
      return w;
    };
    for (int h = 0; h < a.heads; ++h) {
      const long long o = (long long)h * a.E;
      softmax_row<BWD>(a.x + o, a.y + o, a.out + o, b, n, tid, kSoftmaxThreads, block_fold);
    }
  }
}

}  // namespace hcspmm
