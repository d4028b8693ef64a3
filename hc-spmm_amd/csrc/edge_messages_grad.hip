// edge_messages_grad.hip -- gradient of the edge-feature messages with respect to F (hcspmm_edge_messages_grad, DESIGN.md
// section 3.16), fp32:
//   mul: gF[e] = gZ[row(e)] * X[col(e)]    add_relu: gF[e] = (X[col(e)] + F[e] > 0) ? gZ[row(e)] : +0    copy: gF[e] = gZ[row(e)]
// Edge-parallel over contiguous CSR chunks, one chunk per wave, like sddmm_kernel (sddmm_impl.h): a power-law row is cut
// wherever the chunks fall, so a hub costs what its entries cost.  L lanes own one entry (64/L entries per wave step), each
// lane VEC columns through the element-aligned 16-byte lanes (Lane / lane_col); a lane group's entries ascend, so its row
// is a cursor over rowptr and only the chunk's first entry is searched for.  Every row of gF belongs to one lane group,
// which stores it once, non-temporally (a lane moved back by lane_col stores its neighbour's bits again, as the forward
// does); no atomics.  gF and F are addressed in 64 bits.
#include "sddmm_impl.h"

#include "hcspmm.h"

namespace hcspmm {
namespace {

constexpr int kGradThreads = 256;
constexpr int kGradUnroll = 4;  // entries per lane group per step: up to twelve 16-byte loads in flight per lane
constexpr int kGradSteps = 8;   // steps per wave (sddmm_kernel's chunk)

template <int OP, int L, int VEC>
__global__ __launch_bounds__(kGradThreads) void edge_messages_grad_kernel(EdgeMsgGradArgs a) {
  typedef Lane<F32, VEC> LN;
  typedef typename AccT<VEC>::type vec_t;
  constexpr int G = 64 / L;
  constexpr long long kChunk = (long long)kGradSteps * kGradUnroll * G;
  const int lane = threadIdx.x & 63, g = lane / L, sub = lane % L;
  const long long wave = ((long long)blockIdx.x * kGradThreads + threadIdx.x) >> 6;
  const long long e0 = wave * kChunk;
  if (e0 >= a.E) return;
  const long long e1 = min(e0 + kChunk, a.E);
  const int D = a.D;
  const int n_chunks = (D + L * VEC - 1) / (L * VEC);  // > 1 only for L = 64 and D > 64 * VEC
  long long e = e0 + g;
  int r = row_of(a.rowptr, a.N, e < e1 ? e : e0);
  int next = a.rowptr[r + 1];
  for (; e < e1; e += G * kGradUnroll) {
    int rows[kGradUnroll], cols[kGradUnroll];
#pragma unroll
    for (int u = 0; u < kGradUnroll; ++u) {  // rows (a cursor: a group's entries ascend) and column ids
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
      vec_t gz[kGradUnroll], x[kGradUnroll], f[kGradUnroll];
#pragma unroll
      for (int u = 0; u < kGradUnroll; ++u) {  // the loads, all in flight before any store
        gz[u] = x[u] = f[u] = azero<VEC>();
        if (rows[u] >= 0) {
          const size_t eu = (size_t)(e + (long long)u * G);
          gz[u] = LN::load(a.gZ + (size_t)rows[u] * a.ldg + c);
          if constexpr (OP != HCSPMM_EDGE_OP_COPY) x[u] = LN::load(a.X + (size_t)cols[u] * a.ldx + c);
          if constexpr (OP == HCSPMM_EDGE_OP_ADD_RELU) f[u] = LN::load(a.F + eu * a.ldf + c);
        }
      }
#pragma unroll
      for (int u = 0; u < kGradUnroll; ++u) {
        if (rows[u] < 0) continue;
        vec_t out;
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          if constexpr (OP == HCSPMM_EDGE_OP_MUL) aset(out, q, aget(gz[u], q) * aget(x[u], q));
          else if constexpr (OP == HCSPMM_EDGE_OP_ADD_RELU) aset(out, q, aget(x[u], q) + aget(f[u], q) > 0.0f ? aget(gz[u], q) : 0.0f);
          else aset(out, q, aget(gz[u], q));
        }
        LN::store(a.gF + (size_t)(e + (long long)u * G) * a.ldgf + c, out);
      }
    }
  }
}

template <int OP, int L, int VEC>
hipError_t launch_grad_LV(const EdgeMsgGradArgs& a, hipStream_t stream) {
  constexpr long long kChunk = (long long)kGradSteps * kGradUnroll * (64 / L);
  const long long waves = (a.E + kChunk - 1) / kChunk;
  const long long blocks = (waves + kGradThreads / 64 - 1) / (kGradThreads / 64);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((edge_messages_grad_kernel<OP, L, VEC>), dim3((unsigned)blocks), dim3(kGradThreads), 0, stream, a);
  return hipGetLastError();
}

template <int OP>
hipError_t launch_grad_op(const EdgeMsgGradArgs& a, int vec, hipStream_t stream) {
  const int L = sddmm_L(a.D, vec);
  if (vec == 4) {
    switch (L) {
      case 1: return launch_grad_LV<OP, 1, 4>(a, stream);
      case 2: return launch_grad_LV<OP, 2, 4>(a, stream);
      case 4: return launch_grad_LV<OP, 4, 4>(a, stream);
      case 8: return launch_grad_LV<OP, 8, 4>(a, stream);
      case 16: return launch_grad_LV<OP, 16, 4>(a, stream);
      case 32: return launch_grad_LV<OP, 32, 4>(a, stream);
      default: return launch_grad_LV<OP, 64, 4>(a, stream);
    }
  }
  if (a.D > 2 * vec) return hipErrorInvalidValue;  // (pick_vec: 2 for D = 2, 3; 1 for D = 1)
  if (vec == 2) return L == 1 ? launch_grad_LV<OP, 1, 2>(a, stream) : launch_grad_LV<OP, 2, 2>(a, stream);
  return launch_grad_LV<OP, 1, 1>(a, stream);
}

}  // namespace

hipError_t launch_edge_messages_grad_f32(const EdgeMsgGradArgs& a, int vec, hipStream_t stream) {
  switch (a.op) {
    case HCSPMM_EDGE_OP_MUL: return launch_grad_op<HCSPMM_EDGE_OP_MUL>(a, vec, stream);
    case HCSPMM_EDGE_OP_ADD_RELU: return launch_grad_op<HCSPMM_EDGE_OP_ADD_RELU>(a, vec, stream);
    case HCSPMM_EDGE_OP_COPY: return launch_grad_op<HCSPMM_EDGE_OP_COPY>(a, vec, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace hcspmm
