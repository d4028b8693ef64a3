// sample_neighbors.hip -- fanout-limited neighbour sampling on the device (include/hcspmm.h hcspmm_sample_row_pointers_device,
// hcspmm_sample_neighbors_device).
//
//   fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16           (uint32 arithmetic)
//   key(e, seed) = fmix32(fmix32((uint32)e * 0x9E3779B1 + (uint32)seed) + (uint32)(seed >> 32))
//
// A row with deg <= fanout keeps every entry; a longer one the `fanout` entries with the smallest keys, in ascending CSR
// position e.  For one seed, key is a bijection of e (an odd multiply, additions and the invertible fmix32), so there are no
// ties and the fanout-th smallest key T of a row is a threshold: kept = (key <= T).  Keys are recomputed wherever they are
// needed and never stored; nothing depends on the launch shape, and there are no atomics on global memory.
//
// row_pointers_s is the exclusive scan of min(deg, fanout) (graph_build.h exclusive_scan): it does not depend on the seed.
//
// sample_neighbors_kernel: a workgroup of four waves owns 256 consecutive rows, a wave 64 of them (one per lane).
//   copy rows  (deg <= fanout)                       the wave walks the OUTPUT positions of its 64 rows, 64 at a time: a
//              position finds its row by a binary search over the lanes' row_pointers_s (shuffles), so reads and writes are
//              coalesced however short the rows are;
//   wave rows  (fanout < deg <= kSampleWaveRowMax)   one row at a time, kSampleKeysPerLane keys per lane in registers: T by a
//              bitwise radix select from the top bit down (ballots and popcounts), then a ballot-prefix compaction in e order;
//              the kept column ids are loaded at the end of a row and stored after the NEXT row's selection, so a wave does
//              not wait a memory round trip per row;
//   hub rows   (longer)                              the whole workgroup, after its waves are done: T by four passes of
//              8-bit digit histograms in LDS (32-bit counters, keys recomputed in every pass), then the kept entries of each
//              256-entry chunk are placed behind those of the chunks before it.
// No class assumes a maximum degree: a row falls through to the next class by its own length.
#include <hip/hip_runtime.h>

#include "graph_build.h"

namespace hcspmm {
namespace {

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ uint32_t sample_key(int e, uint32_t seed_lo, uint32_t seed_hi) {
  return fmix32(fmix32((uint32_t)e * 0x9E3779B1u + seed_lo) + seed_hi);
}

struct KeptDegree {  // the scan's values: min(deg, fanout) for i < N, 0 for the closing element
  const int32_t* rowptr;
  long long N;
  int fanout;
  __device__ int operator()(long long i) const {
    if (i >= N) return 0;
    const int deg = rowptr[i + 1] - rowptr[i];
    return deg < fanout ? (deg > 0 ? deg : 0) : fanout;
  }
};

__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) {
  return __popcll(m & ((1ull << lane) - 1ull));
}

constexpr int kSampleThreads = 256;

__global__ __launch_bounds__(kSampleThreads) void sample_neighbors_kernel(const int32_t* __restrict__ rowptr,
                                                                           const int32_t* __restrict__ col,
                                                                           const int32_t* __restrict__ rowptr_s, long long N,
                                                                           int fanout, uint32_t seed_lo, uint32_t seed_hi,
                                                                           int32_t* __restrict__ col_s,
                                                                           int32_t* __restrict__ entry_s) {
  __shared__ unsigned long long s_hub[kSampleThreads / 64];  // per wave: its lanes whose rows are left to the workgroup
  __shared__ unsigned int s_hist[256];
  __shared__ int s_wave[kSampleThreads / 64];
  __shared__ unsigned int s_pick[2];  // the digit the threshold takes in this pass, and the rank left inside it
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long block_row0 = (long long)blockIdx.x * kSampleThreads;
  const long long r = block_row0 + wave * 64 + lane;
  const long long rc = r < N ? r : N, rn = r + 1 < N ? r + 1 : N;  // rows past the end: empty, at the end of the output
  const int e0 = rowptr[rc];
  int deg = rowptr[rn] - e0;
  if (deg < 0) deg = 0;
  const int out0 = rowptr_s[rc], out1 = rowptr_s[rn];

  // ---- copy rows: the wave's output positions, 64 at a time ----
  const int wave_out0 = __shfl(out0, 0, 64), wave_out1 = __shfl(out1, 63, 64);
  for (int pb = wave_out0; pb < wave_out1; pb += 64) {  // uniform
    const int p = pb + lane;
    const bool live = p < wave_out1;
    int lo = 0, hi = 64;  // the last lane whose row starts at or before p: invariant out0[lo] <= p < out0[hi] (out0[64] = wave_out1)
#pragma unroll
    for (int it = 0; it < 6; ++it) {
      const int mid = (lo + hi) >> 1;
      const int v = __shfl(out0, mid, 64);
      if (v <= p) lo = mid;
      else hi = mid;
    }
    const int row_e0 = __shfl(e0, lo, 64), row_deg = __shfl(deg, lo, 64), row_out0 = __shfl(out0, lo, 64);
    const int k = p - row_out0;
    if (live && row_deg <= fanout && k < row_deg) {
      const int e = row_e0 + k;
      col_s[p] = col[e];
      entry_s[p] = e;
    }
  }

  // ---- wave rows: kSampleKeysPerLane keys per lane, bitwise radix select ----
  const bool sampled = deg > fanout;
  unsigned long long todo = __ballot(sampled && deg <= kSampleWaveRowMax);
  int pend_p[kSampleKeysPerLane], pend_col[kSampleKeysPerLane];  // kept entries whose column id is still in flight: position, id
#pragma unroll
  for (int j = 0; j < kSampleKeysPerLane; ++j) pend_p[j] = -1, pend_col[j] = 0;
  while (todo) {  // uniform
    const int l = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int row_e0 = __builtin_amdgcn_readlane(e0, l), row_deg = __builtin_amdgcn_readlane(deg, l),
              row_out0 = __builtin_amdgcn_readlane(out0, l), row_out1 = __builtin_amdgcn_readlane(out1, l);
    const int nj = (row_deg + 63) >> 6;  // the 64-entry slices this row has (uniform): the others are skipped
    uint32_t key[kSampleKeysPerLane];
    unsigned int cand = 0;  // bit j: entry j * 64 + lane exists and still matches the threshold's bits found so far
#pragma unroll
    for (int j = 0; j < kSampleKeysPerLane; ++j) {
      key[j] = 0u;
      if (j < nj) {
        const int i = j * 64 + lane;
        key[j] = sample_key(row_e0 + i, seed_lo, seed_hi);
        if (i < row_deg) cand |= 1u << j;
      }
    }
    const unsigned int valid = cand;
    int k = fanout;  // the threshold is the k-th smallest key among the candidates
    uint32_t T = 0;
    for (int b = 31; b >= 0; --b) {
      int zeros = 0;  // candidates whose bit b is 0
#pragma unroll
      for (int j = 0; j < kSampleKeysPerLane; ++j)
        if (j < nj) zeros += __popcll(__ballot(((cand >> j) & 1u) && !((key[j] >> b) & 1u)));
      const bool one = k > zeros;
      if (one) {
        k -= zeros;
        T |= 1u << b;
      }
      unsigned int keep = 0;
#pragma unroll
      for (int j = 0; j < kSampleKeysPerLane; ++j)
        if (j < nj && (((key[j] >> b) & 1u) != 0) == one) keep |= 1u << j;
      cand &= keep;
    }
    // the column ids of the row before, loaded at its end, are stored now: their latency ran under this row's selection
#pragma unroll
    for (int j = 0; j < kSampleKeysPerLane; ++j)
      if (pend_p[j] >= 0) col_s[pend_p[j]] = pend_col[j];
    int base = row_out0;
#pragma unroll
    for (int j = 0; j < kSampleKeysPerLane; ++j) {
      pend_p[j] = -1;
      if (j < nj) {
        const bool kept = ((valid >> j) & 1u) && key[j] <= T;
        const unsigned long long m = __ballot(kept);
        const int p = base + lanes_below(m, lane);
        if (kept && p < row_out1) {  // (p < row_out1 always, for the row_pointers_s of this fanout)
          const int e = row_e0 + j * 64 + lane;
          pend_p[j] = p;
          pend_col[j] = col[e];
          entry_s[p] = e;
        }
        base += __popcll(m);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kSampleKeysPerLane; ++j)
    if (pend_p[j] >= 0) col_s[pend_p[j]] = pend_col[j];

  // ---- hub rows: the workgroup, one row at a time ----
  const unsigned long long hubs = __ballot(sampled && deg > kSampleWaveRowMax);
  if (lane == 0) s_hub[wave] = hubs;
  __syncthreads();
  for (int w = 0; w < kSampleThreads / 64; ++w) {  // uniform over the workgroup from here on
    unsigned long long m = s_hub[w];
    while (m) {
      const int l = __builtin_ctzll(m);
      m &= m - 1;
      const long long row = block_row0 + w * 64 + l;
      const int row_e0 = rowptr[row], row_deg = rowptr[row + 1] - row_e0;
      const int row_out0 = rowptr_s[row], row_out1 = rowptr_s[row + 1];
      // the threshold T, eight bits per pass from the top: histogram of the next digit over the keys that match T so far
      uint32_t T = 0;
      unsigned int k = (unsigned int)fanout;
      for (int shift = 24; shift >= 0; shift -= 8) {
        __syncthreads();  // (s_hist and s_pick of the pass before have been read)
        s_hist[threadIdx.x] = 0u;
        __syncthreads();
        for (int i = threadIdx.x; i < row_deg; i += kSampleThreads) {
          const uint32_t key = sample_key(row_e0 + i, seed_lo, seed_hi);
          if (shift == 24 || (key >> (shift + 8)) == (T >> (shift + 8))) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        const int c = (int)s_hist[threadIdx.x];
        int total;
        const unsigned int before = (unsigned int)block_exclusive_scan(c, s_wave, &total);
        if (before < k && k <= before + (unsigned int)c) {  // exactly one digit: the k-th smallest candidate lies in it
          s_pick[0] = threadIdx.x;
          s_pick[1] = k - before;
        }
        __syncthreads();
        T |= s_pick[0] << shift;
        k = s_pick[1];
      }
      // the kept entries in e order: chunk after chunk of 256, a chunk's entries behind those of the chunks before it
      int base = row_out0;
      for (int i0 = 0; i0 < row_deg; i0 += kSampleThreads) {
        const int i = i0 + threadIdx.x;
        const bool kept = i < row_deg && sample_key(row_e0 + i, seed_lo, seed_hi) <= T;
        const unsigned long long bm = __ballot(kept);
        __syncthreads();  // (s_wave of the chunk before has been read)
        if (lane == 0) s_wave[wave] = __popcll(bm);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int v = 0; v < kSampleThreads / 64; ++v) {
          const int t = s_wave[v];
          if (v < wave) before += t;
          all += t;
        }
        const int p = base + before + lanes_below(bm, lane);
        if (kept && p < row_out1) {
          const int e = row_e0 + i;
          col_s[p] = col[e];
          entry_s[p] = e;
        }
        base += all;
      }
    }
  }
}

}  // namespace

size_t sample_workspace_bytes(long long N) { return N < 0 ? 0 : scan_workspace_ints(N + 1) * sizeof(int32_t); }

hipError_t launch_sample_row_pointers(const int32_t* rowptr, long long N, int fanout, int32_t* rowptr_s, void* workspace,
                                      hipStream_t stream) {
  return exclusive_scan(KeptDegree{rowptr, N, fanout}, N + 1, rowptr_s, reinterpret_cast<int*>(workspace), stream);
}

hipError_t launch_sample_neighbors(const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_s, long long N, int fanout,
                                   uint64_t seed, int32_t* col_s, int32_t* entry_s, hipStream_t stream) {
  if (N <= 0) return hipSuccess;
  const long long blocks = (N + kSampleThreads - 1) / kSampleThreads;
  hipLaunchKernelGGL(sample_neighbors_kernel, dim3((unsigned)blocks), dim3(kSampleThreads), 0, stream, rowptr, col, rowptr_s, N,
                     fanout, (uint32_t)seed, (uint32_t)(seed >> 32), col_s, entry_s);
  return hipGetLastError();
}

}  // namespace hcspmm
