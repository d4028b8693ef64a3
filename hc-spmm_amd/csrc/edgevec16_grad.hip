// edgevec16_grad.hip -- gradient of the per-entry feature-vector sum with respect to F on fp16 / bf16 operands (the 16-bit dtypes
// of the typed edge entry points).  gZ, X, F and the output gF all hold the 16-bit type:
//   mul:      gF[e] = round_once(widen(gZ[row(e)]) * widen(X[col(e)]))   (the fp32 product of two 16-bit values is exact; nearest
//                                                                         even, NaN stays NaN)
//   add_relu: gF[e] = gZ[row(e)]'s own bits where fl32(widen(X[col(e)]) + widen(F[e])) > 0 (the forward's add), else +0
//   copy:     gF[e] = gZ[row(e)]'s bits
// Edge-parallel over contiguous CSR chunks, one chunk per wave, like the fp32 unit and sddmm_kernel (sddmm_impl.h): a power-law
// row is cut wherever the chunks fall.  L lanes own one entry (64/L entries per wave step), each lane 8 columns from 32 columns
// on and 4 below, through the dword-aligned lanes (Lane / lane_col); a lane group's entries ascend, so its row is a cursor over
// rowptr and only the chunk's first entry is searched for.  The up to twelve loads of a step (kGrad16Unroll entries x gZ, X, F)
// are in flight, raw, before any store; every row of gF belongs to one lane group, which stores it once, non-temporally (a lane
// moved back by lane_col stores its neighbour's bits again); no atomics.  F and gF are addressed in 64 bits.
#include "sddmm_impl.h"

#include "hcspmm.h"

namespace hcspmm {
namespace {

constexpr int kGrad16Threads = 256;
constexpr int kGrad16Unroll = 4;  // entries per lane group per step
constexpr int kGrad16Steps = 8;   // steps per wave (sddmm_kernel's chunk)
constexpr int kGrad16MinWaves = 4;

// the result dword of one pair of columns
template <typename E, int OP> __device__ __forceinline__ unsigned grad16_word(unsigned gz, unsigned x, unsigned f) {
  if constexpr (OP == HCSPMM_EDGE_OP_COPY) {
    return gz;
  } else if constexpr (OP == HCSPMM_EDGE_OP_MUL) {
    const float lo = __fmul_rn(widen<E>((unsigned short)(gz & 0xffffu)), widen<E>((unsigned short)(x & 0xffffu)));
    const float hi = __fmul_rn(widen<E>((unsigned short)(gz >> 16)), widen<E>((unsigned short)(x >> 16)));
    return (unsigned)narrow<E>(lo) | ((unsigned)narrow<E>(hi) << 16);
  } else {
    const float lo = __fadd_rn(widen<E>((unsigned short)(x & 0xffffu)), widen<E>((unsigned short)(f & 0xffffu)));
    const float hi = __fadd_rn(widen<E>((unsigned short)(x >> 16)), widen<E>((unsigned short)(f >> 16)));
    return (lo > 0.0f ? gz & 0xffffu : 0u) | (hi > 0.0f ? gz & 0xffff0000u : 0u);
  }
}

template <typename E, int OP, int L, int VEC>
__global__ __launch_bounds__(kGrad16Threads, kGrad16MinWaves) void edgevec16_grad_kernel(EVec16GradArgs a) {
  typedef Lane<E, VEC> LN;
  typedef typename LN::raw_t raw_t;
  constexpr int G = 64 / L;
  constexpr long long kChunk = (long long)kGrad16Steps * kGrad16Unroll * G;
  const int lane = threadIdx.x & 63, g = lane / L, sub = lane % L;
  const long long wave = ((long long)blockIdx.x * kGrad16Threads + threadIdx.x) >> 6;
  const long long e0 = wave * kChunk;
  if (e0 >= a.E) return;
  const long long e1 = min(e0 + kChunk, a.E);
  const int D = a.D;
  const int n_chunks = (D + L * VEC - 1) / (L * VEC);  // > 1 only for L = 64 and D > 64 * VEC
  long long e = e0 + g;
  int r = row_of(a.rowptr, a.N, e < e1 ? e : e0);
  int next = a.rowptr[r + 1];
  for (; e < e1; e += G * kGrad16Unroll) {
    int rows[kGrad16Unroll], cols[kGrad16Unroll];
#pragma unroll
    for (int u = 0; u < kGrad16Unroll; ++u) {  // rows (a cursor: a group's entries ascend) and column ids
      const long long eu = e + (long long)u * G;
      rows[u] = -1;
      cols[u] = 0;
      if (eu < e1) {
        while (next <= eu) next = a.rowptr[++r + 1];
        rows[u] = r;
        if (OP != HCSPMM_EDGE_OP_COPY) cols[u] = a.col[eu];
      }
    }
    for (int k = 0; k < n_chunks; ++k) {
      const int ck = (k * L + sub) * VEC;
      if (ck >= D) continue;
      const int c = lane_col<VEC>(ck, D);
      raw_t gz[kGrad16Unroll], x[kGrad16Unroll], f[kGrad16Unroll];
#pragma unroll
      for (int u = 0; u < kGrad16Unroll; ++u) {  // the loads, all in flight before any store
        gz[u] = x[u] = f[u] = LN::zero();
        if (rows[u] >= 0) {
          const size_t eu = (size_t)(e + (long long)u * G);
          gz[u] = LN::load(a.gZ + (size_t)rows[u] * a.ldg + c);
          if constexpr (OP != HCSPMM_EDGE_OP_COPY) x[u] = LN::load(a.X + (size_t)cols[u] * a.ldx + c);
          if constexpr (OP == HCSPMM_EDGE_OP_ADD_RELU) f[u] = LN::load(a.F + eu * a.ldf + c);
        }
      }
#pragma unroll
      for (int u = 0; u < kGrad16Unroll; ++u) {
        if (rows[u] < 0) continue;
        raw_t out;
#pragma unroll
        for (int w = 0; w < VEC / 2; ++w) rset(out, w, grad16_word<E, OP>(rword(gz[u], w), rword(x[u], w), rword(f[u], w)));
        __builtin_nontemporal_store(out, reinterpret_cast<typename MemU32<VEC / 2>::type*>(
                                             a.gF + (size_t)(e + (long long)u * G) * a.ldgf + c));
      }
    }
  }
}

template <typename E, int OP, int L, int VEC>
hipError_t grad16_launch(const EVec16GradArgs& a, hipStream_t stream) {
  constexpr long long kChunk = (long long)kGrad16Steps * kGrad16Unroll * (64 / L);
  const long long waves = (a.E + kChunk - 1) / kChunk;
  const long long blocks = (waves + kGrad16Threads / 64 - 1) / (kGrad16Threads / 64);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((edgevec16_grad_kernel<E, OP, L, VEC>), dim3((unsigned)blocks), dim3(kGrad16Threads), 0, stream, a);
  return hipGetLastError();
}

// 8 elements per lane from 32 columns on (L = 4 ... 64), 4 below (L = 1 ... 8)
template <typename E, int OP>
hipError_t grad16_op(const EVec16GradArgs& a, hipStream_t stream) {
  if (a.D < 4 || (a.D & 1)) return hipErrorInvalidValue;
  if (a.D >= 32) {
    switch (sddmm_L(a.D, 8)) {
      case 4: return grad16_launch<E, OP, 4, 8>(a, stream);
      case 8: return grad16_launch<E, OP, 8, 8>(a, stream);
      case 16: return grad16_launch<E, OP, 16, 8>(a, stream);
      case 32: return grad16_launch<E, OP, 32, 8>(a, stream);
      default: return grad16_launch<E, OP, 64, 8>(a, stream);
    }
  }
  switch (sddmm_L(a.D, 4)) {
    case 1: return grad16_launch<E, OP, 1, 4>(a, stream);
    case 2: return grad16_launch<E, OP, 2, 4>(a, stream);
    case 4: return grad16_launch<E, OP, 4, 4>(a, stream);
    default: return grad16_launch<E, OP, 8, 4>(a, stream);
  }
}

template <typename E> hipError_t grad16_dtype(const EVec16GradArgs& a, hipStream_t stream) {
  switch (a.op) {
    case HCSPMM_EDGE_OP_MUL: return grad16_op<E, HCSPMM_EDGE_OP_MUL>(a, stream);
    case HCSPMM_EDGE_OP_ADD_RELU: return grad16_op<E, HCSPMM_EDGE_OP_ADD_RELU>(a, stream);
    case HCSPMM_EDGE_OP_COPY: return grad16_op<E, HCSPMM_EDGE_OP_COPY>(a, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_edgevec16_grad(const EVec16GradArgs& a, int dtype, hipStream_t stream) {
  if (dtype == HCSPMM_DTYPE_F16) return grad16_dtype<F16>(a, stream);
  if (dtype == HCSPMM_DTYPE_BF16) return grad16_dtype<BF16>(a, stream);
  return hipErrorInvalidValue;
}

}  // namespace hcspmm
