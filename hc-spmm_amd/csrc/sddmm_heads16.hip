// sddmm_heads16.hip -- multi-head SDDMM on fp16 / bf16 rows (the 16-bit dtypes of hcspmm_sddmm_heads_typed; DESIGN.md section
// 3.11b):
//   out[h*E + e] = <A[row(e)][h*Dh : (h+1)*Dh], B[col(e)][h*Dh : (h+1)*Dh]>   for h < heads, fp32, head-major.
// The fp32 unit loops over the heads with the lanes of ONE head per entry; at Dh = 8 in 16 bits that is one lane per entry and
// head.  Here a lane group spans the entry's whole row, all heads * Dh columns: a lane owns 8 columns (4 when Dh % 8 != 0) inside
// one head, each B row is gathered once (a 64-column row is one 128-byte line), and the A row stays in registers while the
// group's entries stay in one row.  Per lane the products are summed with fmaf in column order; then a segmented reduction runs
// over the Dh / VEC lanes of each head -- an xor butterfly where that count is a power of two, else the head's first lane adds its
// neighbours' sums in lane order: both orders are fixed by (Dh, VEC) alone.  The head's first lane writes the result with a
// non-temporal store.  sddmm_impl.h's schedule: edge-parallel chunks per wave with a row cursor, so a chunk cut inside a hub row
// needs no fix-up.  Deterministic, no atomics; every entry and head is written exactly once.
#include "sddmm_impl.h"

#include "hcspmm.h"

namespace hcspmm {
namespace {

constexpr int kSH16MinWaves = 4;

// the lane's products in column order, the dwords widened pair by pair
template <typename E, int VEC>
__device__ __forceinline__ float heads16_dot(const typename Lane<E, VEC>::raw_t& a, const typename Lane<E, VEC>::raw_t& b) {
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < VEC; ++q) acc = fmaf(Lane<E, VEC>::elem(a, q), Lane<E, VEC>::elem(b, q), acc);
  return acc;
}

// a.D = heads * Dh (the whole row), L * VEC >= a.D
template <typename E, int L, int VEC>
__global__ __launch_bounds__(kSddmmThreads, kSH16MinWaves) void sddmm_heads16_kernel(SddmmArgs a, int dh) {
  typedef typename E::T T;
  typedef Lane<E, VEC> LN;
  typedef typename LN::raw_t raw_t;
  constexpr int G = 64 / L;
  constexpr long long kChunk = (long long)kSddmmSteps * kSddmmUnroll * G;
  const int lane = threadIdx.x & 63, g = lane / L, sub = lane % L;
  const long long wave = ((long long)blockIdx.x * kSddmmThreads + threadIdx.x) >> 6;
  const long long e0 = wave * kChunk;
  if (e0 >= a.E) return;
  const long long e1 = min(e0 + kChunk, a.E);
  const T* __restrict__ A = reinterpret_cast<const T*>(a.A);
  const T* __restrict__ B = reinterpret_cast<const T*>(a.B);
  const int c = sub * VEC;  // (D % VEC == 0: no lane is moved back)
  const bool live = c < a.D;
  const int lh = dh / VEC;                         // lanes per head
  const int head = live ? c / dh : 0;
  const bool first = live && c - head * dh == 0;   // the head's first lane
  const bool pow2 = (lh & (lh - 1)) == 0;
  float* __restrict__ oh = a.out + (long long)head * a.E;
  long long e = e0 + g;
  int r = row_of(a.rowptr, a.N, e < e1 ? e : e0);
  int next = a.rowptr[r + 1];
  int ra = -1;  // row whose A columns sit in `ar`
  raw_t ar = LN::zero();
  for (; e < e1; e += G * kSddmmUnroll) {
    int rows[kSddmmUnroll], cols[kSddmmUnroll];
    raw_t bv[kSddmmUnroll], av[kSddmmUnroll];
#pragma unroll
    for (int u = 0; u < kSddmmUnroll; ++u) {  // rows (a cursor: a group's entries ascend) and column ids
      const long long eu = e + (long long)u * G;
      rows[u] = -1;
      cols[u] = 0;
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
        bv[u] = LN::load(B + (size_t)cols[u] * a.ldb + c);
        const int prev = u == 0 ? ra : rows[u - 1];
        if (rows[u] != prev) av[u] = LN::load(A + (size_t)rows[u] * a.lda + c);
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
      if (live) acc[u] = heads16_dot<E, VEC>(ar, bv[u]);
    }
    if (pow2) {  // heads start at multiples of lh lanes: the butterfly stays inside the head
      for (int off = lh >> 1; off > 0; off >>= 1)
#pragma unroll
        for (int u = 0; u < kSddmmUnroll; ++u) acc[u] += __shfl_xor(acc[u], off, 64);
    } else {  // lane order: ((s0 + s1) + s2) + ...
      float sum[kSddmmUnroll];
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u) sum[u] = acc[u];
      for (int t = 1; t < lh; ++t)
#pragma unroll
        for (int u = 0; u < kSddmmUnroll; ++u) sum[u] += __shfl(acc[u], (lane + t) & 63, 64);
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u) acc[u] = sum[u];
    }
    if (first) {
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u)
        if (rows[u] >= 0) __builtin_nontemporal_store(acc[u], oh + e + (long long)u * G);
    }
  }
}

template <typename E, int L, int VEC>
hipError_t launch_sddmm_heads16_LV(const SddmmArgs& a, int dh, hipStream_t stream) {
  constexpr long long kChunk = (long long)kSddmmSteps * kSddmmUnroll * (64 / L);
  const long long waves = (a.E + kChunk - 1) / kChunk;
  const long long blocks = (waves + kSddmmThreads / 64 - 1) / (kSddmmThreads / 64);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sddmm_heads16_kernel<E, L, VEC>), dim3((unsigned)blocks), dim3(kSddmmThreads), 0, stream, a, dh);
  return hipGetLastError();
}

template <typename E, int VEC> hipError_t sddmm_heads16_L(const SddmmArgs& a, int dh, hipStream_t stream) {
  switch (sddmm_L(a.D, VEC)) {
    case 1: return launch_sddmm_heads16_LV<E, 1, VEC>(a, dh, stream);
    case 2: return launch_sddmm_heads16_LV<E, 2, VEC>(a, dh, stream);
    case 4: return launch_sddmm_heads16_LV<E, 4, VEC>(a, dh, stream);
    case 8: return launch_sddmm_heads16_LV<E, 8, VEC>(a, dh, stream);
    case 16: return launch_sddmm_heads16_LV<E, 16, VEC>(a, dh, stream);
    case 32: return launch_sddmm_heads16_LV<E, 32, VEC>(a, dh, stream);
    default: return launch_sddmm_heads16_LV<E, 64, VEC>(a, dh, stream);
  }
}

template <typename E> hipError_t sddmm_heads16_dispatch(const SddmmArgs& a, int heads, hipStream_t stream) {
  if (heads <= 0 || a.D % heads != 0) return hipErrorInvalidValue;
  const int dh = a.D / heads;
  if (dh % 4 != 0) return hipErrorInvalidValue;
  const int vec = dh % 8 == 0 ? 8 : 4;
  if (a.D > 64 * vec) return hipErrorInvalidValue;  // one lane group per row
  return vec == 8 ? sddmm_heads16_L<E, 8>(a, dh, stream) : sddmm_heads16_L<E, 4>(a, dh, stream);
}

}  // namespace

bool sddmm_heads16_supported(int D, int heads) {
  if (heads <= 0 || D <= 0 || D % heads != 0 || (D / heads) % 4 != 0) return false;
  return D <= 64 * ((D / heads) % 8 == 0 ? 8 : 4);
}

hipError_t launch_sddmm_heads16(const SddmmArgs& a, int heads, int dtype, hipStream_t stream) {
  if (dtype == HCSPMM_DTYPE_F16) return sddmm_heads16_dispatch<F16>(a, heads, stream);
  if (dtype == HCSPMM_DTYPE_BF16) return sddmm_heads16_dispatch<BF16>(a, heads, stream);
  return hipErrorInvalidValue;
}

}  // namespace hcspmm
