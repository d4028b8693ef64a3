// graph_build.h -- graphs built on the device (include/hcspmm.h hcspmm_sample_* and hcspmm_transpose_graph_device): the
// launchers of sample_neighbors.hip and transpose_device.hip, and the exclusive scan both use.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace hcspmm {

// ---- the sampler (sample_neighbors.hip) ----
// Rows up to kSampleWaveRowMax entries that are longer than the fanout are selected by one wave holding
// kSampleWaveRowMax / 64 keys per lane; longer ones by their workgroup (HCSPMM_SAMPLE_WAVE_ROW_MAX in hcspmm.h).
constexpr int kSampleKeysPerLane = 8;
constexpr int kSampleWaveRowMax = 64 * kSampleKeysPerLane;

size_t sample_workspace_bytes(long long N);
hipError_t launch_sample_row_pointers(const int32_t* rowptr, long long N, int fanout, int32_t* rowptr_s, void* workspace,
                                      hipStream_t stream);
hipError_t launch_sample_neighbors(const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_s, long long N, int fanout,
                                   uint64_t seed, int32_t* col_s, int32_t* entry_s, hipStream_t stream);

// ---- the transpose (transpose_device.hip) ----
size_t transpose_workspace_bytes(long long M, long long E);
hipError_t launch_transpose_graph(const int32_t* rowptr, const int32_t* col, long long N, long long M, long long E,
                                  int32_t* rowptr_t, int32_t* col_t, int32_t* entry_t, void* workspace, hipStream_t stream);

// ---- exclusive scan of n int32 values: out[i] = value(0) + ... + value(i - 1) ----
// Three launches: the sum of every tile of kScanTile values, a one-workgroup scan of those sums, and the tiles again.
// `value` is a functor (long long i) -> int, evaluated twice per i; out may alias what it reads at the same index.
// sums: kScanTile-th of n ints of workspace (scan_workspace_ints).
constexpr int kScanThreads = 256, kScanItems = 8, kScanTile = kScanThreads * kScanItems;

inline long long scan_tiles(long long n) { return (n + kScanTile - 1) / kScanTile; }
inline size_t scan_workspace_ints(long long n) { return (size_t)scan_tiles(n); }

#ifdef __HIPCC__
// sum over the workgroup's 256 threads -> (exclusive prefix of this thread, total), through wave shuffles and four LDS words
__device__ inline int block_exclusive_scan(int v, int* s_wave /* [kScanThreads / 64] */, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  __syncthreads();  // (s_wave may still be read from the call before)
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    const int t = s_wave[w];
    if (w < wave) before += t;
    all += t;
  }
  *total = all;
  return before + incl - v;
}

template <class V>
__global__ __launch_bounds__(kScanThreads) void scan_tile_sums_kernel(V value, long long n, int* __restrict__ sums) {
  __shared__ int s_wave[kScanThreads / 64];
  const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
  int v = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k)
    if (i0 + k < n) v += value(i0 + k);
  int total;
  block_exclusive_scan(v, s_wave, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

template <class V>
__global__ __launch_bounds__(kScanThreads) void scan_sums_kernel(int* __restrict__ sums, long long tiles) {
  __shared__ int s_wave[kScanThreads / 64];
  int carry = 0;
  for (long long b = 0; b < tiles; b += kScanThreads) {  // uniform
    const long long i = b + threadIdx.x;
    const int v = i < tiles ? sums[i] : 0;
    int total;
    const int ex = block_exclusive_scan(v, s_wave, &total);
    if (i < tiles) sums[i] = carry + ex;
    carry += total;
  }
}

template <class V>
__global__ __launch_bounds__(kScanThreads) void scan_tiles_kernel(V value, long long n, const int* __restrict__ sums,
                                                                  int* out) {
  __shared__ int s_wave[kScanThreads / 64];
  const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
  int x[kScanItems];
  int v = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    x[k] = i0 + k < n ? value(i0 + k) : 0;
    v += x[k];
  }
  int total;
  int run = sums[blockIdx.x] + block_exclusive_scan(v, s_wave, &total);
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (i0 + k < n) out[i0 + k] = run;
    run += x[k];
  }
}

template <class V>
hipError_t exclusive_scan(V value, long long n, int* out, int* sums, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const long long tiles = scan_tiles(n);
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scan_tile_sums_kernel<V>, dim3((unsigned)tiles), dim3(kScanThreads), 0, stream, value, n, sums);
  hipLaunchKernelGGL(scan_sums_kernel<V>, dim3(1), dim3(kScanThreads), 0, stream, sums, tiles);
  hipLaunchKernelGGL(scan_tiles_kernel<V>, dim3((unsigned)tiles), dim3(kScanThreads), 0, stream, value, n, (const int*)sums, out);
  return hipGetLastError();
}
#endif  // __HIPCC__

}  // namespace hcspmm
