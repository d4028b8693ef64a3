// transpose_device.hip -- A^T of a CSR graph built on the device (include/hcspmm.h hcspmm_transpose_graph_device): the outputs
// of the host counting sort hcspmm_transpose_graph, element for element, with no host read.
//
// A stable least-significant-digit radix sort of the pairs (column_index[e], e) by column, eight bits per pass over the bits
// that num_cols - 1 has: stability is the contract -- within a row of A^T the entries keep ascending e -- and an LSD sort has it
// by construction.  Per pass: a digit histogram per tile of kSortTile entries (LDS counters), one exclusive scan of the
// [digit][tile] table (graph_build.h), and a scatter in which a wave walks its tile 64 entries at a time: a lane's rank among
// the lanes of the same digit comes from eight ballots, the digit's running position from LDS.  No atomics on global memory;
// the result does not depend on the launch shape.  The passes alternate between the workspace and the output arrays so that
// the last one leaves the sorted columns in column_index_t (scratch until then) and the sorted e in entry_index_t; then
//   row_pointers_t[j] = number of sorted columns below j (a binary search per j), and
//   column_index_t[q] = the row of A that holds entry_index_t[q] (a binary search in row_pointers, as hcspmm_edge_to_row_device).
// column_index is trusted, as the plan-free kernels trust it, but never used as an address: a digit is eight bits of it, and a
// position comes from the counts of those digits, so every write lands inside the E-element arrays whatever the ids are.
#include <hip/hip_runtime.h>

#include "graph_build.h"

namespace hcspmm {
namespace {

constexpr int kSortTile = 2048;  // entries per tile: 32 steps of one wave

__global__ __launch_bounds__(256) void radix_hist_kernel(const int32_t* __restrict__ keys, long long E, int shift,
                                                         int* __restrict__ table, long long tiles) {
  __shared__ unsigned int s_hist[256];
  s_hist[threadIdx.x] = 0u;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kSortTile;
  for (int i = threadIdx.x; i < kSortTile; i += 256) {
    const long long idx = base + i;
    if (idx < E) atomicAdd(&s_hist[((uint32_t)keys[idx] >> shift) & 255u], 1u);
  }
  __syncthreads();
  table[(long long)threadIdx.x * tiles + blockIdx.x] = (int)s_hist[threadIdx.x];
}

struct TableValue {
  const int* table;
  __device__ int operator()(long long i) const { return table[i]; }
};

// vals_in == nullptr: the first pass, whose values are the positions themselves
__global__ __launch_bounds__(64) void radix_scatter_kernel(const int32_t* __restrict__ keys_in, const int32_t* __restrict__ vals_in,
                                                           long long E, int shift, const int* __restrict__ table,
                                                           long long tiles, int32_t* __restrict__ keys_out,
                                                           int32_t* __restrict__ vals_out) {
  __shared__ int s_pos[256];  // where the next entry of each digit goes
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += 64) s_pos[d] = table[(long long)d * tiles + blockIdx.x];
  __syncthreads();
  const long long base = (long long)blockIdx.x * kSortTile;
  for (int c = 0; c < kSortTile && base + c < E; c += 64) {  // uniform
    const long long idx = base + c + lane;
    const bool valid = idx < E;
    const int32_t key = valid ? keys_in[idx] : 0;
    const unsigned int d = ((uint32_t)key >> shift) & 255u;
    unsigned long long peers = __ballot(valid);  // the valid lanes with this lane's digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    const int pos = s_pos[d] + rank;
    __syncthreads();
    if (valid && rank == 0) s_pos[d] += __popcll(peers);  // one lane per digit
    __syncthreads();
    if (valid && pos >= 0 && pos < E) {  // (always, by the counts; the compare costs nothing)
      keys_out[pos] = key;
      vals_out[pos] = vals_in ? vals_in[idx] : (int32_t)idx;
    }
  }
}

__global__ __launch_bounds__(256) void transposed_row_pointers_kernel(const int32_t* __restrict__ sorted_cols, long long E, long long M,
                                                                      int32_t* __restrict__ rowptr_t) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j <= M; j += stride) {
    long long lo = 0, hi = E;  // the first position whose column is not below j
    while (lo < hi) {
      const long long mid = lo + ((hi - lo) >> 1);
      if ((long long)sorted_cols[mid] < j) lo = mid + 1;
      else hi = mid;
    }
    rowptr_t[j] = (int32_t)lo;
  }
}

__global__ __launch_bounds__(256) void entry_rows_kernel(const int32_t* __restrict__ rowptr, int N, const int32_t* __restrict__ entries,
                                                         long long E, int32_t* __restrict__ rows) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < E; q += stride) {
    const long long e = entries[q];
    int lo = 0, hi = N;  // invariant: rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if ((long long)rowptr[mid] <= e) lo = mid;
      else hi = mid;
    }
    rows[q] = lo;
  }
}

inline long long sort_tiles(long long E) { return (E + kSortTile - 1) / kSortTile; }

inline int sort_passes(long long M) {
  int bits = 1;
  while (bits < 32 && (1ll << bits) < M) ++bits;
  return (bits + 7) / 8;
}

inline unsigned grid_for(long long n) {
  long long blocks = (n + 255) / 256;
  return (unsigned)(blocks < 1 ? 1 : blocks > 65536 ? 65536 : blocks);
}

}  // namespace

// [E] keys and [E] values of the passes that do not land in the outputs, the [256][tiles] table and its scan's tile sums
size_t transpose_workspace_bytes(long long M, long long E) {
  if (M < 0 || E <= 0) return 0;
  const long long table = 256 * sort_tiles(E);
  return ((size_t)2 * (size_t)E + (size_t)table + scan_workspace_ints(table)) * sizeof(int32_t);
}

hipError_t launch_transpose_graph(const int32_t* rowptr, const int32_t* col, long long N, long long M, long long E,
                                  int32_t* rowptr_t, int32_t* col_t, int32_t* entry_t, void* workspace, hipStream_t stream) {
  if (E > 0) {
    const long long tiles = sort_tiles(E);
    int32_t* ws_keys = reinterpret_cast<int32_t*>(workspace);
    int32_t* ws_vals = ws_keys + E;
    int* table = ws_vals + E;
    int* sums = table + 256 * tiles;
    const int passes = sort_passes(M);
    const int32_t *keys_in = col, *vals_in = nullptr;
    for (int p = 0; p < passes; ++p) {
      const bool to_outputs = ((passes - 1 - p) & 1) == 0;  // the last pass lands in the outputs, the ones before alternate
      int32_t* keys_out = to_outputs ? col_t : ws_keys;
      int32_t* vals_out = to_outputs ? entry_t : ws_vals;
      hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, keys_in, E, 8 * p, table, tiles);
      hipError_t e = exclusive_scan(TableValue{table}, 256 * tiles, table, sums, stream);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)tiles), dim3(64), 0, stream, keys_in, vals_in, E, 8 * p,
                         (const int*)table, tiles, keys_out, vals_out);
      keys_in = keys_out;
      vals_in = vals_out;
    }
  }
  hipLaunchKernelGGL(transposed_row_pointers_kernel, dim3(grid_for(M + 1)), dim3(256), 0, stream, (const int32_t*)col_t, E, M,
                     rowptr_t);
  if (E > 0)
    hipLaunchKernelGGL(entry_rows_kernel, dim3(grid_for(E)), dim3(256), 0, stream, rowptr, (int)N, (const int32_t*)entry_t, E, col_t);
  return hipGetLastError();
}

}  // namespace hcspmm
