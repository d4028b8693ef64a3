// update_kernels_h16.hip -- the dense half of a layer on fp16 / bf16 operands (fp32: update_kernels.hip):
//   out[N x H] = in[N x D] * W[D x H]      16-bit `in`, W of that type or fp32 (rounded once as it is staged), fp32 accumulation
//   dW[D x H]  = A^T[D x N] * B[N x H]     16-bit A and B, fp32 dW
// Both on v_mfma_f32_16x16x32_{f16,bf16}: lane (i = l & 15, kq = l >> 4) supplies 8 k-consecutive 16-bit elements of row i
// (A operand) or of column i (B operand), k = 8*kq .. 8*kq + 7, and receives C[4*kq + r][i] in accumulator register r.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hcspmm.h"
#include "spmm_kernels.h"

namespace hcspmm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u16_u32x4 __attribute__((ext_vector_type(4)));
// rows on the dword grid only: a 16-byte piece of a row is addressed with 4-byte alignment (all gfx950 needs)
typedef unsigned int u16_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned int u16_u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef unsigned int u16_u32x2_a8 __attribute__((ext_vector_type(2), aligned(8)));
typedef float u16_f32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef float u16_f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct H16 {
  typedef _Float16 T;
  typedef _Float16 V8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x4 mfma(V8 a, V8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
struct B16 {
  typedef __bf16 T;
  typedef __bf16 V8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x4 mfma(V8 a, V8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// fp32 -> 16 bits, round to nearest even, NaN stays NaN (the hardware conversions; what torch's .to() gives)
template <typename E> __device__ __forceinline__ unsigned int bits16(float v) {
  const typename E::T h = static_cast<typename E::T>(v);
  return (unsigned int)__builtin_bit_cast(unsigned short, h);
}

// eight 16-bit elements at p, of which the first `nvalid` (even) exist: one 16-byte load, or -- FULL8 = false, the tail of a row
// whose width is no multiple of 8 -- the dwords that exist.  Nothing outside the row is read; the rest is zero.
template <bool FULL8> __device__ __forceinline__ u16_u32x4 load_row8(const unsigned short* p, int nvalid) {
  u16_u32x4 v = {0u, 0u, 0u, 0u};
  if (nvalid >= 8) {
    v = *reinterpret_cast<const u16_u32x4_a4*>(p);
  } else if constexpr (!FULL8) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (2 * j < nvalid) v[j] = reinterpret_cast<const unsigned int*>(p)[j];
  }
  return v;
}

// ------------------------------------------------------------------------------------------
// out = in * W.  One wave per 16-row tile, kU16Waves waves per workgroup, workgroups stride over the tiles.
//  * W is staged once per workgroup into LDS in 16 bits and in the B-operand shape: LDS row t*16 + n holds column T*n + t of W,
//    k-consecutive, zero-padded to whole 32-row k-steps and to 16*T columns; a lane's B operand of (k-step kk, tile t) is the 16
//    bytes at row t*16 + n, element 32*kk + 8*kq.  Row stride Dp + 8 elements = 4 (mod 8) dwords: the 16 lanes of a quarter
//    wave hit 16 different 4-dword bank groups.
//  * lane (i, kq) loads in[row i][32*kk + 8*kq .. +8) as one 16-byte load: the A operand of k-step kk as it arrives.
//  * kU16Steps k-steps of loads are in flight; the next chunk (of this tile or of the wave's next tile) is requested before the
//    MFMAs of the current one, so a tile's load latency hides behind the previous tile's products and stores.
//  * tile t holds columns T*n + t, so a lane's T results of a row are T consecutive columns: one vector store (fp32), or T/2
//    packed dwords (16-bit output on the dword grid).  Full rows of whole vectors leave non-temporally; masked or unpacked
//    pieces take cached stores so that the L2 assembles whole lines (the fp32 kernel's finding).
// ------------------------------------------------------------------------------------------
constexpr int kU16Waves = 8;
constexpr int kU16Steps = 4;       // k-steps per chunk: 4 x 16 bytes per lane, twice (current + requested)
constexpr int kU16GridCap = 512;   // x 8 waves: the wave count of the fp32 streaming launch (one resident round)
constexpr size_t kU16LdsBudget = 160 * 1024;

template <bool FULL8>
__device__ __forceinline__ void load_chunk(u16_u32x4 (&a)[kU16Steps], const unsigned short* in, long long ld_in, int N, int D,
                                           int r0, int k0, int i, int kq) {
  const int row = r0 + i;
  const unsigned short* p = in + (long long)(row < N ? row : 0) * ld_in;
#pragma unroll
  for (int u = 0; u < kU16Steps; ++u) {
    const int k = k0 + 32 * u + 8 * kq;
    a[u] = load_row8<FULL8>(p + (k < D ? k : 0), row < N ? D - k : 0);
  }
}

template <typename E, int T, bool OUT16, bool FULL8>
__global__ __launch_bounds__(kU16Waves * 64) void update16_kernel(const unsigned short* __restrict__ in, long long ld_in,
                                                                  const void* __restrict__ Wv, int w_f32, long long ldr,
                                                                  long long ldc, void* __restrict__ outv, long long ld_out,
                                                                  int N, int D, int H, int n_tiles, int pack) {
  extern __shared__ __attribute__((aligned(16))) unsigned short s_w16[];  // [16*T][KS]
  const int Dp = (D + 31) & ~31;
  const int KS = Dp + 8;
  for (int e = threadIdx.x; e < Dp * 16 * T; e += kU16Waves * 64) {
    const int k = e / (16 * T), c = e - k * (16 * T);
    unsigned int b = 0;
    if (k < D && c < H) {
      const long long at = (long long)k * ldr + (long long)c * ldc;
      b = w_f32 ? bits16<E>(static_cast<const float*>(Wv)[at]) : (unsigned int)static_cast<const unsigned short*>(Wv)[at];
    }
    s_w16[((c % T) * 16 + c / T) * KS + k] = (unsigned short)b;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int stride = (int)gridDim.x * kU16Waves;
  int ti = (int)blockIdx.x * kU16Waves + wave;
  if (ti >= n_tiles) return;
  u16_u32x4 cur[kU16Steps], nxt[kU16Steps];
  load_chunk<FULL8>(cur, in, ld_in, N, D, ti * 16, 0, i, kq);
  for (; ti < n_tiles; ti += stride) {
    const int r0 = ti * 16;
    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < D; k0 += 32 * kU16Steps) {
      const bool more = k0 + 32 * kU16Steps < D;
      if (more)
        load_chunk<FULL8>(nxt, in, ld_in, N, D, r0, k0 + 32 * kU16Steps, i, kq);
      else if (ti + stride < n_tiles)
        load_chunk<FULL8>(nxt, in, ld_in, N, D, r0 + 16 * stride, 0, i, kq);
#pragma unroll
      for (int u = 0; u < kU16Steps; ++u) {
        if (k0 + 32 * u < D) {
          const typename E::V8 av = __builtin_bit_cast(typename E::V8, cur[u]);
          const unsigned short* wp = s_w16 + i * KS + k0 + 32 * u + 8 * kq;
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const u16_u32x4 bw = *reinterpret_cast<const u16_u32x4*>(wp + t * 16 * KS);
            acc[t] = E::mfma(av, __builtin_bit_cast(typename E::V8, bw), acc[t]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kU16Steps; ++u) cur[u] = nxt[u];
    }
    const bool whole = H == 16 * T;  // every lane's T columns exist
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = r0 + 4 * kq + r;
      if (orow >= N) continue;
      if constexpr (OUT16) {
        unsigned short* o = static_cast<unsigned short*>(outv) + (long long)orow * ld_out + T * i;
        if (T % 2 == 0 && pack && whole) {  // T/2 dwords
          unsigned int d[(T + 1) / 2];
#pragma unroll
          for (int t = 0; t + 1 < T; t += 2) d[t / 2] = bits16<E>(acc[t][r]) | (bits16<E>(acc[t + 1][r]) << 16);
          if constexpr (T == 2) __builtin_nontemporal_store(d[0], reinterpret_cast<unsigned int*>(o));
          if constexpr (T == 4) __builtin_nontemporal_store(u16_u32x2_a4{d[0], d[1]}, reinterpret_cast<u16_u32x2_a4*>(o));
          if constexpr (T == 6) {
            __builtin_nontemporal_store(u16_u32x2_a4{d[0], d[1]}, reinterpret_cast<u16_u32x2_a4*>(o));
            __builtin_nontemporal_store(d[2], reinterpret_cast<unsigned int*>(o) + 2);
          }
          if constexpr (T == 8) __builtin_nontemporal_store(u16_u32x4_a4{d[0], d[1], d[2], d[3]}, reinterpret_cast<u16_u32x4_a4*>(o));
        } else {
#pragma unroll
          for (int t = 0; t < T; ++t)
            if (T * i + t < H) o[t] = (unsigned short)bits16<E>(acc[t][r]);
        }
      } else {
        float* o = static_cast<float*>(outv) + (long long)orow * ld_out + T * i;
        if (whole) {
#pragma unroll
          for (int t = 0; t + 3 < T; t += 4)
            __builtin_nontemporal_store(f32x4{acc[t][r], acc[t + 1][r], acc[t + 2][r], acc[t + 3][r]}, reinterpret_cast<u16_f32x4_a4*>(o + t));
          constexpr int t4 = T & ~3;
          if constexpr (T - t4 >= 2)
            __builtin_nontemporal_store(u16_f32x2_a4{acc[t4][r], acc[t4 + 1][r]}, reinterpret_cast<u16_f32x2_a4*>(o + t4));
          if constexpr (T % 2 == 1) __builtin_nontemporal_store(acc[T - 1][r], o + T - 1);
        } else {
#pragma unroll
          for (int t = 0; t < T; ++t)
            if (T * i + t < H) o[t] = acc[t][r];
        }
      }
    }
  }
}

size_t update16_lds_bytes(int D, int H) {
  return (size_t)(16 * ((H + 15) / 16)) * (size_t)(((D + 31) & ~31) + 8) * sizeof(unsigned short);
}

bool update16_supported(int D, int H) {
  return D >= 2 && D % 2 == 0 && H >= 1 && H <= 128 && update16_lds_bytes(D, H) <= kU16LdsBudget;
}

template <typename E, int T>
static hipError_t launch_u16(const Update16Args& a, hipStream_t stream) {
  const int n_tiles = (a.N + 15) / 16;
  int grid = (n_tiles + kU16Waves - 1) / kU16Waves;
  if (grid > kU16GridCap) grid = kU16GridCap;
  const size_t lds = update16_lds_bytes(a.D, a.H);
  // 16-bit outputs leave as packed dwords when their rows are on the dword grid
  const int pack = a.out16 && a.ld_out % 2 == 0 && (reinterpret_cast<uintptr_t>(a.out) & 3) == 0;
#define HCSPMM_U16_GO(OUT16_, FULL8_)                                                                                              \
  hipLaunchKernelGGL((update16_kernel<E, T, OUT16_, FULL8_>), dim3(grid), dim3(kU16Waves * 64), lds, stream,                       \
                     static_cast<const unsigned short*>(a.in), a.ld_in, a.W, a.w_f32, a.ldr, a.ldc, a.out, a.ld_out, a.N, a.D, a.H, \
                     n_tiles, pack)
  const bool full8 = a.D % 8 == 0;
  if (a.out16) {
    if (full8) HCSPMM_U16_GO(true, true); else HCSPMM_U16_GO(true, false);
  } else {
    if (full8) HCSPMM_U16_GO(false, true); else HCSPMM_U16_GO(false, false);
  }
#undef HCSPMM_U16_GO
  return hipGetLastError();
}

template <typename E>
static hipError_t launch_u16_t(const Update16Args& a, hipStream_t stream) {
  switch ((a.H + 15) / 16) {
    case 1: return launch_u16<E, 1>(a, stream);
    case 2: return launch_u16<E, 2>(a, stream);
    case 3: return launch_u16<E, 3>(a, stream);
    case 4: return launch_u16<E, 4>(a, stream);
    case 5: return launch_u16<E, 5>(a, stream);
    case 6: return launch_u16<E, 6>(a, stream);
    case 7: return launch_u16<E, 7>(a, stream);
    default: return launch_u16<E, 8>(a, stream);
  }
}

hipError_t launch_update16(const Update16Args& a, int dtype, hipStream_t stream) {
  if (a.N <= 0) return hipSuccess;
  if (!update16_supported(a.D, a.H)) return hipErrorInvalidValue;
  return dtype == HCSPMM_DTYPE_F16 ? launch_u16_t<H16>(a, stream) : launch_u16_t<B16>(a, stream);
}

// ------------------------------------------------------------------------------------------
// dW = A^T * B.  K runs along the rows, so a lane's 8 k-consecutive operand elements are 8 rows of one column: rows cannot feed
// the MFMA as they arrive.  K is split over the grid as in weight_grad_partial_kernel; per step a wave brings 32 rows of A and
// of B into its own LDS tile (16-byte row pieces, DT + HT of them per lane, the next step's requested before this step's
// products) and reads the operands back transposed with 2-byte LDS reads packed into the operand registers.  All DT x HT
// accumulator tiles stay in registers; the waves are folded through LDS in wave order, one fp32 partial per workgroup, and
// weight_grad_reduce_kernel adds the partials in workgroup order.  Rows past the workgroup's block are zero in LDS.
// Tile row stride 16*(DT + HT) + 4 elements = 2 (mod 4) dwords: the four row groups kq of a transposed read fall into four
// different bank octets; rows stay 8-byte aligned for the writes.
// ------------------------------------------------------------------------------------------
constexpr int kWg16Waves = 4;

// a wave's own LDS writes must be visible to its own (cross-lane) reads: program order on the LDS pipe + no compiler motion
__device__ __forceinline__ void wave_lds_fence16() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename E, int DT, int HT>
__global__ __launch_bounds__(kWg16Waves * 64) void weight_grad16_partial_kernel(const unsigned short* __restrict__ A, long long lda,
                                                                                const unsigned short* __restrict__ B, long long ldb,
                                                                                float* __restrict__ partial, int N, int D, int H,
                                                                                int rows_per_wg) {
  constexpr int LS = 16 * (DT + HT) + 4;
  constexpr int kTileWords = kWg16Waves * 32 * LS / 2, kFoldWords = DT * HT * 256;
  __shared__ __attribute__((aligned(16))) unsigned int s_mem[kTileWords > kFoldWords ? kTileWords : kFoldWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  unsigned short* tile = reinterpret_cast<unsigned short*>(s_mem) + wave * 32 * LS;
  const long long r_begin = (long long)blockIdx.x * rows_per_wg;
  const long long r_end = min((long long)N, r_begin + rows_per_wg);
  f32x4 acc[DT][HT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) acc[dt][ht] = f32x4{0.f, 0.f, 0.f, 0.f};
  u16_u32x4 ga[DT], gb[HT];
  // piece m of a lane: 16-byte piece l + 64*m of the step's 32 x 16*DT (32 x 16*HT) block, row-major
  auto request = [&](long long r0) {
#pragma unroll
    for (int m = 0; m < DT; ++m) {
      const int c = lane + 64 * m, rr = c / (2 * DT), k = 8 * (c - rr * (2 * DT));
      const long long row = r0 + rr;
      const bool ok = row < r_end && k < D;
      ga[m] = load_row8<false>(A + (ok ? row * lda + k : 0), ok ? D - k : 0);
    }
#pragma unroll
    for (int m = 0; m < HT; ++m) {
      const int c = lane + 64 * m, rr = c / (2 * HT), k = 8 * (c - rr * (2 * HT));
      const long long row = r0 + rr;
      const bool ok = row < r_end && k < H;
      gb[m] = load_row8<false>(B + (ok ? row * ldb + k : 0), ok ? H - k : 0);
    }
  };
  // a wave's tile is its own: between its writes and its transposed reads stands a wave-level fence only, and the four waves
  // run their steps independently until the fold
  const int steps = rows_per_wg / (32 * kWg16Waves);
  request(r_begin + 32 * wave);
  for (int s = 0; s < steps; ++s) {
#pragma unroll
    for (int m = 0; m < DT; ++m) {
      const int c = lane + 64 * m, rr = c / (2 * DT), k = 8 * (c - rr * (2 * DT));
      u16_u32x2_a8* w = reinterpret_cast<u16_u32x2_a8*>(tile + rr * LS + k);
      w[0] = u16_u32x2_a8{ga[m][0], ga[m][1]};
      w[1] = u16_u32x2_a8{ga[m][2], ga[m][3]};
    }
#pragma unroll
    for (int m = 0; m < HT; ++m) {
      const int c = lane + 64 * m, rr = c / (2 * HT), k = 8 * (c - rr * (2 * HT));
      u16_u32x2_a8* w = reinterpret_cast<u16_u32x2_a8*>(tile + rr * LS + 16 * DT + k);
      w[0] = u16_u32x2_a8{gb[m][0], gb[m][1]};
      w[1] = u16_u32x2_a8{gb[m][2], gb[m][3]};
    }
    if (s + 1 < steps) request(r_begin + 32 * ((long long)(s + 1) * kWg16Waves + wave));
    wave_lds_fence16();
    const unsigned short* tp = tile + 8 * kq * LS + i;  // rows 8*kq .. +8 of column i
    typename E::V8 bop[HT];
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
      u16_u32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[j] = (unsigned int)tp[(2 * j) * LS + 16 * (DT + ht)] | ((unsigned int)tp[(2 * j + 1) * LS + 16 * (DT + ht)] << 16);
      bop[ht] = __builtin_bit_cast(typename E::V8, v);
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      u16_u32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (unsigned int)tp[(2 * j) * LS + 16 * dt] | ((unsigned int)tp[(2 * j + 1) * LS + 16 * dt] << 16);
      const typename E::V8 aop = __builtin_bit_cast(typename E::V8, v);
#pragma unroll
      for (int ht = 0; ht < HT; ++ht) acc[dt][ht] = E::mfma(aop, bop[ht], acc[dt][ht]);
    }
    wave_lds_fence16();  // the tile is rewritten by the next step
  }
  __syncthreads();  // the fold's buffer lies over the tiles
  // fold the waves in wave order (fixed => deterministic), one wave at a time through one accumulator-sized buffer
  float* s_red = reinterpret_cast<float*>(s_mem);
  for (int w = 1; w < kWg16Waves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int ht = 0; ht < HT; ++ht)
#pragma unroll
          for (int r = 0; r < 4; ++r) s_red[(dt * HT + ht) * 256 + r * 64 + lane] = acc[dt][ht][r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int ht = 0; ht < HT; ++ht)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[dt][ht][r] += s_red[(dt * HT + ht) * 256 + r * 64 + lane];
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* out = partial + (size_t)blockIdx.x * (size_t)D * (size_t)H;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int ht = 0; ht < HT; ++ht)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int d = 16 * dt + 4 * kq + r, h = 16 * ht + i;  // accumulator register r of lane (kq, i) is C[4*kq + r][i]
          if (d < D && h < H) out[d * H + h] = acc[dt][ht][r];
        }
  }
}

template <typename E, int DT, int HT>
static hipError_t launch_wg16(const unsigned short* A, long long lda, const unsigned short* B, long long ldb, float* out,
                              float* partial, long long N, int D, int H, hipStream_t stream) {
  // a workgroup's block is whole steps of its four waves (128 rows): no more groups than such blocks, so that none stages nothing
  // (`partial` is sized for weight_grad_groups(N), at least as many)
  constexpr int kBlock = 32 * kWg16Waves;
  const int G = (int)min((long long)weight_grad_groups(N), (N + kBlock - 1) / kBlock);
  long long rows = (N + G - 1) / G;
  rows = (rows + kBlock - 1) / kBlock * kBlock;
  hipLaunchKernelGGL((weight_grad16_partial_kernel<E, DT, HT>), dim3(G), dim3(kWg16Waves * 64), 0, stream, A, lda, B, ldb, partial,
                     (int)N, D, H, (int)rows);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_weight_grad_reduce(partial, out, G, D * H, stream);
}

template <typename E>
static hipError_t launch_wg16_e(const unsigned short* A, long long lda, const unsigned short* B, long long ldb, float* out,
                                float* partial, long long N, int D, int H, hipStream_t stream) {
  const int dt = (D + 15) / 16, ht = (H + 15) / 16;
#define HCSPMM_WG16_CASE(DT_, HT_) \
  if (dt == DT_ && ht == HT_) return launch_wg16<E, DT_, HT_>(A, lda, B, ldb, out, partial, N, D, H, stream);
  HCSPMM_WG16_CASE(1, 1) HCSPMM_WG16_CASE(2, 1) HCSPMM_WG16_CASE(3, 1) HCSPMM_WG16_CASE(4, 1) HCSPMM_WG16_CASE(5, 1)
  HCSPMM_WG16_CASE(6, 1) HCSPMM_WG16_CASE(7, 1) HCSPMM_WG16_CASE(8, 1)
  HCSPMM_WG16_CASE(1, 2) HCSPMM_WG16_CASE(2, 2) HCSPMM_WG16_CASE(3, 2) HCSPMM_WG16_CASE(4, 2) HCSPMM_WG16_CASE(5, 2)
  HCSPMM_WG16_CASE(6, 2) HCSPMM_WG16_CASE(7, 2) HCSPMM_WG16_CASE(8, 2)
  HCSPMM_WG16_CASE(1, 3) HCSPMM_WG16_CASE(2, 3) HCSPMM_WG16_CASE(3, 3) HCSPMM_WG16_CASE(4, 3) HCSPMM_WG16_CASE(5, 3)
  HCSPMM_WG16_CASE(6, 3) HCSPMM_WG16_CASE(7, 3) HCSPMM_WG16_CASE(8, 3)
  HCSPMM_WG16_CASE(1, 4) HCSPMM_WG16_CASE(2, 4) HCSPMM_WG16_CASE(3, 4) HCSPMM_WG16_CASE(4, 4) HCSPMM_WG16_CASE(5, 4)
  HCSPMM_WG16_CASE(6, 4) HCSPMM_WG16_CASE(7, 4) HCSPMM_WG16_CASE(8, 4)
#undef HCSPMM_WG16_CASE
  return hipErrorInvalidValue;
}

// every (ceil(D/16) <= 8) x (ceil(H/16) <= 4): up to 32 accumulator tiles, which the 16-bit operands' registers leave room for
bool weight_grad16_supported(int D, int H) { return D > 0 && H > 0 && (D + 15) / 16 <= 8 && (H + 15) / 16 <= 4; }

hipError_t launch_weight_grad16(const void* A, long long lda, const void* B, long long ldb, int dtype, float* out, float* partial,
                                long long N, int D, int H, hipStream_t stream) {
  const unsigned short* a = static_cast<const unsigned short*>(A);
  const unsigned short* b = static_cast<const unsigned short*>(B);
  return dtype == HCSPMM_DTYPE_F16 ? launch_wg16_e<H16>(a, lda, b, ldb, out, partial, N, D, H, stream)
                                   : launch_wg16_e<B16>(a, lda, b, ldb, out, partial, N, D, H, stream);
}

}  // namespace hcspmm
