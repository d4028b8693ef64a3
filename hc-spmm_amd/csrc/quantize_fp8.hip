// quantize_fp8.hip -- per-row quantiser of fp32 features to OCP e4m3fn codes with one fp32 scale per row
// (hcspmm_quantize_fp8; the storage hcspmm_forward_fp8 reads).  For row r:
//   amax = max |x| over the row's finite entries;  s[r] = amax / 448 (IEEE division), 1 when amax == 0 (or nothing is finite),
//   raised to 2^-126 when the quotient is not a normal number; a caller's scale vector replaces the computed one;
//   code = rne_e4m3(clamp(x / s[r], -448, 448)) with an IEEE division: +-inf saturates to +-448, NaN gives the NaN code
//   (0x7f, with x's sign bit).
// One kernel, a row held in registers: G lanes (a power of two, 16 columns per lane at most) own a row and read it with 16-byte
// loads, fold |x| with a shuffle tree, divide, and narrow two values per v_cvt_pk_fp8_f32 -- four codes per lane and store.
// Rows wider than 16 * 64 columns re-read the columns past that in the second pass (they are L2 hits).
#include <hip/hip_runtime.h>
#include <float.h>

#include "spmm_kernels.h"

namespace hcspmm {
namespace {

typedef float q_f32x4 __attribute__((ext_vector_type(4), aligned(4)));  // element-aligned: any fp32 row stride

constexpr int kQuantChunks = 4;  // 16-byte chunks of a row a lane keeps in registers

__device__ __forceinline__ float finite_abs_max(float amax, const q_f32x4& v) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float a = __builtin_fabsf(v[q]);
    if (a < __builtin_inff()) amax = __builtin_fmaxf(amax, a);  // (false for NaN and inf)
  }
  return amax;
}

// four codes of four values, byte q = element q
__device__ __forceinline__ unsigned codes_of(const q_f32x4& v, float scale) {
  float t[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) t[q] = __builtin_fminf(__builtin_fmaxf(__fdiv_rn(v[q], scale), -448.0f), 448.0f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], w, true);
  unsigned u = (unsigned)w;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (v[q] != v[q]) {  // NaN: the min / max above dropped it
      const unsigned code = 0x7fu | ((__float_as_uint(v[q]) >> 24) & 0x80u);
      u = (u & ~(0xffu << (8 * q))) | (code << (8 * q));
    }
  }
  return u;
}

__global__ __launch_bounds__(256) void quantize_fp8_kernel(const float* __restrict__ X, long long rows, long long ldx, int D,
                                                           const float* __restrict__ scale_in, unsigned char* __restrict__ Xq,
                                                           long long ldq, float* __restrict__ scale_out, int G) {
  const int lane = threadIdx.x & 63;
  const int R = 64 / G, g = lane / G, s = lane & (G - 1);
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * R + g;
  const bool rok = r < rows;
  const float* xr = X + (rok ? r : 0) * ldx;
  q_f32x4 v[kQuantChunks];
  float amax = 0.0f;
#pragma unroll
  for (int k = 0; k < kQuantChunks; ++k) {
    const int c = (s + k * G) * 4;
    v[k] = q_f32x4{0.f, 0.f, 0.f, 0.f};
    if (rok && c < D) v[k] = *reinterpret_cast<const q_f32x4*>(xr + c);
  }
  float scale;
  if (scale_in != nullptr) {
    scale = rok ? scale_in[r] : 1.0f;
  } else {
#pragma unroll
    for (int k = 0; k < kQuantChunks; ++k) amax = finite_abs_max(amax, v[k]);
    if (rok) {
      for (int c = (s + kQuantChunks * G) * 4; c < D; c += G * 4) amax = finite_abs_max(amax, *reinterpret_cast<const q_f32x4*>(xr + c));
    }
    for (int off = 1; off < G; off <<= 1) amax = __builtin_fmaxf(amax, __shfl_xor(amax, off, 64));
    scale = __fdiv_rn(amax, 448.0f);
    if (amax == 0.0f) scale = 1.0f;
    else if (scale < FLT_MIN) scale = FLT_MIN;
  }
  if (!rok) return;
  unsigned char* qr = Xq + r * ldq;
#pragma unroll
  for (int k = 0; k < kQuantChunks; ++k) {
    const int c = (s + k * G) * 4;
    if (c < D) *reinterpret_cast<unsigned*>(qr + c) = codes_of(v[k], scale);
  }
  for (int c = (s + kQuantChunks * G) * 4; c < D; c += G * 4)
    *reinterpret_cast<unsigned*>(qr + c) = codes_of(*reinterpret_cast<const q_f32x4*>(xr + c), scale);
  if (s == 0 && scale_out != nullptr) scale_out[r] = scale;
}

}  // namespace

hipError_t launch_quantize_fp8(const float* X, long long rows, long long ldx, int D, const float* scale_in, unsigned char* Xq,
                               long long ldq, float* scale_out, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  int G = 1;  // lanes per row: one 16-byte chunk per lane up to 256 columns, then up to kQuantChunks and beyond
  while (G < 64 && G * 4 < D) G <<= 1;
  const long long waves = (rows + 64 / G - 1) / (64 / G);
  const long long blocks = (waves + 3) / 4;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(quantize_fp8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, X, rows, ldx, D, scale_in, Xq, ldq,
                     scale_out, G);
  return hipGetLastError();
}

}  // namespace hcspmm
