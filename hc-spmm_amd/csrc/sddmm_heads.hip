// sddmm_heads.hip -- multi-head SDDMM (hcspmm_sddmm_heads), fp32:
//   out[h*E + e] = <A[row(e)][h*Dh : (h+1)*Dh], B[col(e)][h*Dh : (h+1)*Dh]>   for h < heads.
// sddmm_kernel (sddmm_impl.h) over the column slice of one head, with the heads as an inner loop: a wave walks its CSR chunk
// once, loads each entry's row and column id once for every head, and per head runs the lane sums and the xor-butterfly
// that hcspmm_sddmm runs on that slice (same L, vector width and per-lane column order), so every head's result has the
// bits of hcspmm_sddmm on the slice views.  Deterministic, no atomics.
#include "sddmm_impl.h"

namespace hcspmm {
namespace {

template <typename E, int L, int VEC>
__global__ __launch_bounds__(kSddmmThreads) void sddmm_heads_kernel(SddmmArgs a, int heads) {
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
  const int D = a.D;  // columns per head
  const int c = sub * VEC, c0 = lane_col<VEC>(c, D), skip = c - c0;
  const bool live = c < D;
  const int n_chunks = (D + L * VEC - 1) / (L * VEC);
  long long e = e0 + g;
  int r = row_of(a.rowptr, a.N, e < e1 ? e : e0);
  int next = a.rowptr[r + 1];
  for (; e < e1; e += G * kSddmmUnroll) {
    int rows[kSddmmUnroll], cols[kSddmmUnroll];
#pragma unroll
    for (int u = 0; u < kSddmmUnroll; ++u) {  // rows and column ids: once for all heads
      const long long eu = e + (long long)u * G;
      rows[u] = -1;
      if (eu < e1) {
        while (next <= eu) next = a.rowptr[++r + 1];
        rows[u] = r;
        cols[u] = a.col[eu];
      }
    }
    for (int h = 0; h < heads; ++h) {
      const T* __restrict__ Ah = A + (size_t)h * D;
      const T* __restrict__ Bh = B + (size_t)h * D;
      raw_t bv[kSddmmUnroll], av[kSddmmUnroll];
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u) {
        bv[u] = LN::zero();
        av[u] = u > 0 ? av[u - 1] : LN::zero();
        if (rows[u] >= 0 && live) {
          bv[u] = LN::load(Bh + (size_t)cols[u] * a.ldb + c0);
          if (u == 0 || rows[u] != rows[u - 1]) av[u] = LN::load(Ah + (size_t)rows[u] * a.lda + c0);
        }
      }
      float acc[kSddmmUnroll];
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u) {
        acc[u] = 0.f;
        if (rows[u] < 0) continue;
        if (live) acc[u] = lane_dot<E, VEC>(av[u], bv[u], skip, 0.f);
        for (int k = 1; k < n_chunks; ++k) {
          const int ck = (k * L + sub) * VEC;
          if (ck < D) {
            const int ck0 = lane_col<VEC>(ck, D);
            const raw_t ak = LN::load(Ah + (size_t)rows[u] * a.lda + ck0);
            const raw_t bk = LN::load(Bh + (size_t)cols[u] * a.ldb + ck0);
            acc[u] = lane_dot<E, VEC>(ak, bk, ck - ck0, acc[u]);
          }
        }
      }
#pragma unroll
      for (int off = L / 2; off > 0; off >>= 1)
#pragma unroll
        for (int u = 0; u < kSddmmUnroll; ++u) acc[u] += __shfl_xor(acc[u], off, 64);
      if (sub == 0) {
        float* __restrict__ oh = a.out + (long long)h * a.E;
#pragma unroll
        for (int u = 0; u < kSddmmUnroll; ++u)
          if (rows[u] >= 0) __builtin_nontemporal_store(acc[u], oh + e + (long long)u * G);
      }
    }
  }
}

template <typename E, int L, int VEC>
hipError_t launch_sddmm_heads_LV(const SddmmArgs& a, int heads, hipStream_t stream) {
  constexpr long long kChunk = (long long)kSddmmSteps * kSddmmUnroll * (64 / L);
  const long long waves = (a.E + kChunk - 1) / kChunk;
  const long long blocks = (waves + kSddmmThreads / 64 - 1) / (kSddmmThreads / 64);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sddmm_heads_kernel<E, L, VEC>), dim3((unsigned)blocks), dim3(kSddmmThreads), 0, stream, a, heads);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_sddmm_heads_f32(const SddmmArgs& a, int heads, int vec, hipStream_t stream) {
  if (vec != 4 || heads <= 0) return hipErrorInvalidValue;  // (Dh % 4 == 0: every slice takes 16-byte lanes)
  switch (sddmm_L(a.D, 4)) {
    case 1: return launch_sddmm_heads_LV<F32, 1, 4>(a, heads, stream);
    case 2: return launch_sddmm_heads_LV<F32, 2, 4>(a, heads, stream);
    case 4: return launch_sddmm_heads_LV<F32, 4, 4>(a, heads, stream);
    case 8: return launch_sddmm_heads_LV<F32, 8, 4>(a, heads, stream);
    case 16: return launch_sddmm_heads_LV<F32, 16, 4>(a, heads, stream);
    case 32: return launch_sddmm_heads_LV<F32, 32, 4>(a, heads, stream);
    default: return launch_sddmm_heads_LV<F32, 64, 4>(a, heads, stream);
  }
}

}  // namespace hcspmm
