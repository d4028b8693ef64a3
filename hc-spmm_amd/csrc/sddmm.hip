// sddmm.hip -- instantiations of the SDDMM and edge softmax kernels (sddmm_impl.h holds the device code): fp32, fp16 and
// bf16 operands for the SDDMM, fp32 accumulation and output throughout.
#include "sddmm_impl.h"

namespace hcspmm {

hipError_t launch_sddmm_f32(const SddmmArgs& a, int vec, hipStream_t stream) {
  if (vec == 4) { HCSPMM_SDDMM_DISPATCH(F32, 4, a, stream) }
  if (a.D > 4 * vec) return hipErrorInvalidValue;  // (8-byte and single-element lanes serve D <= 3)
  if (vec == 2) return launch_sddmm_LV<F32, 2, 2>(a, stream);
  return launch_sddmm_LV<F32, 1, 1>(a, stream);
}

template <typename E>
static hipError_t sddmm16(const SddmmArgs& a, int vec, hipStream_t stream) {
  if (vec == 8) { HCSPMM_SDDMM_DISPATCH(E, 8, a, stream) }
  if (vec == 4) { HCSPMM_SDDMM_DISPATCH(E, 4, a, stream) }
  HCSPMM_SDDMM_DISPATCH(E, 1, a, stream)
}

hipError_t launch_sddmm_f16(const SddmmArgs& a, int vec, hipStream_t stream) { return sddmm16<F16>(a, vec, stream); }
hipError_t launch_sddmm_bf16(const SddmmArgs& a, int vec, hipStream_t stream) { return sddmm16<BF16>(a, vec, stream); }

hipError_t launch_edge_softmax(const SoftmaxArgs& a, bool backward, hipStream_t stream) {
  if (a.N == 0 || a.E == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((a.N + kSoftmaxThreads - 1) / kSoftmaxThreads);
  if (backward) hipLaunchKernelGGL(edge_softmax_kernel<true>, dim3(blocks), dim3(kSoftmaxThreads), 0, stream, a);
  else hipLaunchKernelGGL(edge_softmax_kernel<false>, dim3(blocks), dim3(kSoftmaxThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace hcspmm
