// update_kernels.hip -- the "update" half of the fused aggregate+update operators:
//   out[N x H] = agg[N x D] * W[D x H]      (fp32 in, fp32 MFMA, k-ascending fma chain)
// Replaces the second stage of the reference's fused kernels (hybrid_all_kernel.cu:1807-1837 in
// _32_fused, and the same block in _64_fused / _final_fused / _GIN_final_fused), which multiply
// the aggregated 16-row tile by the weight matrix with WMMA tf32.  Here: one wave per 16 rows,
// v_mfma_f32_16x16x4_f32, any D and H, arbitrary element strides for W (so the transposed view
// the reference's backward passes, GNN_model.py:98,120, is consumed without a copy).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "spmm_kernels.h"

namespace hcspmm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

#ifndef HCSPMM_UPD_GRID_CAP
#define HCSPMM_UPD_GRID_CAP 1024  // one resident round of the streaming update; 512: 5-20 % slower, 2048 / 4096: -6 ... +3 % (profiles/r03/ab_update_grid.log)
#endif
constexpr int kUpdWaves = 4;
constexpr int kMaxTiles = 8;  // 16-column output tiles kept in registers per pass (128 columns)

__global__ __launch_bounds__(kUpdWaves * 64) void dense_update_kernel(const float* __restrict__ in,
                                                                      const float* __restrict__ W, long long ldr,
                                                                      long long ldc, float* __restrict__ out, int N,
                                                                      int D, int H, const int* __restrict__ tile_list,
                                                                      int n_tiles) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ti = (int)blockIdx.x * kUpdWaves + wave;
  if (ti >= n_tiles) return;
  const int r0 = (tile_list ? tile_list[ti] : ti) * 16;
  if (r0 >= N) return;
  const int i = lane & 15, kq = lane >> 4;
  const int row = r0 + i;
  const bool rok = row < N;
  const float* arow = in + (size_t)(rok ? row : 0) * (size_t)D;
  for (int h0 = 0; h0 < H; h0 += 16 * kMaxTiles) {
    const int ntiles = min(kMaxTiles, (H - h0 + 15) / 16);
    f32x4 acc[kMaxTiles];
#pragma unroll
    for (int t = 0; t < kMaxTiles; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < D; k0 += 4) {
      const int k = k0 + kq;
      const bool kok = k < D;
      const float av = (rok && kok) ? arow[k] : 0.0f;
#pragma unroll
      for (int t = 0; t < kMaxTiles; ++t) {
        if (t < ntiles) {
          const int n = h0 + t * 16 + i;  // B operand: lane (k = kq, n = lane & 15)
          const float bv = (kok && n < H) ? W[(long long)k * ldr + (long long)n * ldc] : 0.0f;
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kMaxTiles; ++t) {
      if (t < ntiles) {
        const int n = h0 + t * 16 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int orow = r0 + 4 * kq + r;
          if (orow < N && n < H) out[(size_t)orow * (size_t)H + n] = acc[t][r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Streaming variant for the shapes GNN layers use (H = 16*T, T <= 4; D % 16 == 0; 16-byte aligned
// rows): the kernel is bound by reading agg once, so
//  * W is staged in LDS once per workgroup and the workgroup strides over many 64-row tiles;
//  * a lane loads agg with 16-byte accesses: lane (i = l & 15, kq = l >> 4) takes
//    agg[row i][16*kk + 4*kq .. +4), and the q-th of its four floats feeds k-step q -- the k order
//    inside a 16-chunk is a fixed permutation, applied to the W rows as well;
//  * tile t of a k-step multiplies by W columns T*j + t, so the T results of a lane are T
//    consecutive output columns and leave as one vector store.
// The accumulation order per output element is a fixed permutation of k (deterministic).
// ------------------------------------------------------------------------------------------
// PAD: H is not 16*T -- the staged weights are zero-padded to 16*T columns, the stores masked.  DPAD: D is even but not a
// multiple of 16 (the reference's default 22 classes as the INPUT width): rows of agg are read in 8-byte pairs, the staged
// weights zero-padded to whole 16-row chunks.
// vectors of `out` (and the 8-byte pairs of a DPAD `in`) are addressed with ELEMENT alignment: a caller's output matrix that is
// only 4-byte aligned, or rows of an odd width, still take one 8- / 16-byte store (gfx950 needs dword alignment only)
typedef float upd_f32x2 __attribute__((ext_vector_type(2), aligned(4)));
typedef float upd_f32x4 __attribute__((ext_vector_type(4), aligned(4)));

template <int T, bool PAD, bool DPAD = false>
__global__ __launch_bounds__(kUpdWaves * 64) void dense_update_stream_kernel(const float* __restrict__ in,
                                                                             const float* __restrict__ W,
                                                                             long long ldr, long long ldc,
                                                                             float* __restrict__ out, int N, int D,
                                                                             int Hreal, const int* __restrict__ tile_list,
                                                                             int n_tiles) {
  extern __shared__ __attribute__((aligned(16))) float s_w[];  // [D][HS], HS = 16*T + 4 (row stride = 4 mod 8 words)
  constexpr int H = 16 * T;
  constexpr int HS = H + 4;
  const int Dp = DPAD ? (D + 15) / 16 * 16 : D;
  for (int i = threadIdx.x; i < Dp * H; i += kUpdWaves * 64) {
    const int k = i / H, h = i - k * H;
    s_w[k * HS + h] = ((!PAD || h < Hreal) && (!DPAD || k < D)) ? W[(long long)k * ldr + (long long)h * ldc] : 0.0f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  for (int ti = (int)blockIdx.x * kUpdWaves + wave; ti < n_tiles; ti += (int)gridDim.x * kUpdWaves) {
    const int r0 = (tile_list ? tile_list[ti] : ti) * 16;
    const int row = r0 + i;
    const bool rok = row < N;
    const f32x4* arow = reinterpret_cast<const f32x4*>(in + (size_t)(rok ? row : 0) * (size_t)D) + kq;
    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < D; k0 += 64) {  // four 16-chunks of agg in flight
      f32x4 a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (DPAD) {
          typedef float f32x2 __attribute__((ext_vector_type(2)));
          const int k = k0 + 16 * u + 4 * kq;  // columns k .. k + 3 of this lane's row, as two pairs (D is even)
          const float* ap = in + (size_t)(rok ? row : 0) * (size_t)D + k;
          if (rok && k < D) {
            const f32x2 lo = *reinterpret_cast<const upd_f32x2*>(ap);
            a[u][0] = lo[0];
            a[u][1] = lo[1];
          }
          if (rok && k + 2 < D) {
            const f32x2 hi = *reinterpret_cast<const upd_f32x2*>(ap + 2);
            a[u][2] = hi[0];
            a[u][3] = hi[1];
          }
        } else {
          if (rok && k0 + 16 * u < D) a[u] = arow[(k0 >> 2) + 4 * u];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (k0 + 16 * u < D) {
          const float* wrow = s_w + (k0 + 16 * u + 4 * kq) * HS + T * i;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int t = 0; t < T; ++t)
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][q], wrow[q * HS + t], acc[t], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = r0 + 4 * kq + r;
      if (orow < N) {
        float* o = out + (size_t)orow * (size_t)(PAD ? Hreal : H) + T * i;
        // written once, not read by this operator: non-temporal stores (1-4 % on the two-launch form, 9 % on the all-dense
        // graph at D = 32: profiles/r03/ab_fused_rows.log)
        if constexpr (PAD) {
          // pieces of T floats that do not fill 16-byte units: plain (cached) stores, so that the L2 assembles whole lines
          // before they leave (as non-temporal scalar stores the (32, 96) shape ran 3x slower)
          if constexpr (T % 2 == 0) {
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            if ((Hreal & 1) == 0) {  // 8-byte aligned pairs
#pragma unroll
              for (int t = 0; t < T; t += 2)
                if (T * i + t < Hreal) *reinterpret_cast<upd_f32x2*>(o + t) = f32x2{acc[t][r], acc[t + 1][r]};
              continue;
            }
          }
#pragma unroll
          for (int t = 0; t < T; ++t)
            if (T * i + t < Hreal) o[t] = acc[t][r];
        } else if constexpr (T == 2) {
          typedef float f32x2 __attribute__((ext_vector_type(2)));
          __builtin_nontemporal_store(f32x2{acc[0][r], acc[1][r]}, reinterpret_cast<upd_f32x2*>(o));
        } else if constexpr (T == 4) {
          __builtin_nontemporal_store(f32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]}, reinterpret_cast<upd_f32x4*>(o));
        } else {
#pragma unroll
          for (int t = 0; t < T; ++t) __builtin_nontemporal_store(acc[t][r], o + t);
        }
      }
    }
  }
}

// The same product for a scattered set of rows: the sparse-path rows the row-tile fused launch (fused_rows.hip) leaves out.
// Item j of the list is one of the n_wide longest tasks (a whole row when its slot is < 0), a fix-up entry (a split or
// column-sliced row, complete after the fix-up pass) or a slice descriptor (a sliced row that fell into ONE piece keeps a
// direct store: row >= 0 and slot < 0); everything else in those lists is skipped.  16 items per wave step; lane i reads
// row(item i), the store addresses of rows 4*kq + r come from that lane by shuffle.  Same k order as above => same bits.
template <int T>
__global__ __launch_bounds__(kUpdWaves * 64) void dense_update_rows_kernel(const float* __restrict__ in,
                                                                           const float* __restrict__ W, long long ldr,
                                                                           long long ldc, float* __restrict__ out, int D, int Hreal,
                                                                           const int* __restrict__ plan, int off_tasks,
                                                                           int n_wide, int off_fixups, int n_split_rows,
                                                                           int off_slice_tasks, int n_slice_tasks) {
  extern __shared__ __attribute__((aligned(16))) float s_w[];
  constexpr int H = 16 * T;
  constexpr int HS = H + 4;
  const int Dp = (D + 15) & ~15;  // (D off the 16-column grid: zero rows in the staged weights, masked loads of the row's tail)
  for (int i = threadIdx.x; i < Dp * H; i += kUpdWaves * 64) {
    const int k = i / H, h = i - k * H;
    s_w[k * HS + h] = (h < Hreal && k < D) ? W[(long long)k * ldr + (long long)h * ldc] : 0.0f;  // (zero columns / rows, masked stores)
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int n_items = n_wide + n_split_rows + n_slice_tasks;
  const int n_tiles = (n_items + 15) / 16;
  const int4* tasks = reinterpret_cast<const int4*>(plan + off_tasks);
  const int4* fixups = reinterpret_cast<const int4*>(plan + off_fixups);
  const int4* slices = reinterpret_cast<const int4*>(plan + off_slice_tasks);
  for (int ti = (int)blockIdx.x * kUpdWaves + wave; ti < n_tiles; ti += (int)gridDim.x * kUpdWaves) {
    const int j = ti * 16 + i;
    int row = -1;
    if (j < n_wide) {
      const int4 t = tasks[j];
      row = t.w < 0 ? t.x : -1;
    } else if (j < n_wide + n_split_rows) {
      row = fixups[j - n_wide].x;
    } else if (j < n_items) {
      const int4 t = slices[j - n_wide - n_split_rows];
      row = (t.x >= 0 && t.w < 0) ? t.x : -1;
    }
    if (__builtin_amdgcn_ballot_w64(row >= 0) == 0) continue;  // wave-uniform
    const bool rok = row >= 0;
    const float* arow = in + (size_t)(rok ? row : 0) * (size_t)D + 4 * kq;
    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < D; k0 += 64) {
      f32x4 a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int k = k0 + 16 * u + 4 * kq;  // columns k .. k + 3 of this lane's row
        if (rok && k + 3 < D) {
          a[u] = *reinterpret_cast<const upd_f32x4*>(arow + k0 + 16 * u);
        } else if (rok && k < D) {  // the row's tail
#pragma unroll
          for (int q = 0; q < 3; ++q)
            if (k + q < D) a[u][q] = arow[k0 + 16 * u + q];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (k0 + 16 * u < D) {
          const float* wrow = s_w + (k0 + 16 * u + 4 * kq) * HS + T * i;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int t = 0; t < T; ++t)
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][q], wrow[q * HS + t], acc[t], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = __shfl(row, 4 * kq + r, 64);
      if (orow >= 0) {
        float* o = out + (size_t)orow * (size_t)Hreal + T * i;
#pragma unroll
        for (int t = 0; t < T; ++t)
          if (T * i + t < Hreal) o[t] = acc[t][r];
      }
    }
  }
}

template <int T>
static hipError_t launch_rows(const float* in, const float* W, long long ldr, long long ldc, float* out, int D, int H,
                              const int* plan, int off_tasks, int n_wide, int off_fixups, int n_split_rows,
                              int off_slice_tasks, int n_slice_tasks, hipStream_t stream) {
  const size_t lds = (size_t)((D + 15) / 16 * 16) * (16 * T + 4) * sizeof(float);
  const long long n_tiles = ((long long)n_wide + n_split_rows + n_slice_tasks + 15) / 16;
  int grid = (int)((n_tiles + kUpdWaves - 1) / kUpdWaves);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL((dense_update_rows_kernel<T>), dim3(grid), dim3(kUpdWaves * 64), lds, stream, in, W, ldr, ldc, out, D, H,
                     plan, off_tasks, n_wide, off_fixups, n_split_rows, off_slice_tasks, n_slice_tasks);
  return hipGetLastError();
}

template <int T, bool PAD, bool DPAD = false>
static hipError_t launch_stream(const float* in, const float* W, long long ldr, long long ldc, float* out, int N, int D, int H,
                                const int* tile_list, int n_tiles, hipStream_t stream) {
  const size_t lds = (size_t)(DPAD ? (D + 15) / 16 * 16 : D) * (16 * T + 4) * sizeof(float);
  int grid = (n_tiles + kUpdWaves - 1) / kUpdWaves;
  if (grid > HCSPMM_UPD_GRID_CAP) grid = HCSPMM_UPD_GRID_CAP;  // W is staged once per workgroup: stride over the row tiles
  hipLaunchKernelGGL((dense_update_stream_kernel<T, PAD, DPAD>), dim3(grid), dim3(kUpdWaves * 64), lds, stream, in, W, ldr, ldc,
                     out, N, D, H, tile_list, n_tiles);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Weight gradient of the update GEMM:  dW[D x H] = A^T[D x N] * B[N x H]  with K = N rows (hundreds of
// thousands) and a tiny output.  The reference does it with torch.mm(X.t(), dY) (GNN_model.py:79,101,124,...);
// the library GEMM picked for that shape on MI355X runs ONE output tile over the whole K (253 us at N = 233 K,
// 40 % of a GCN epoch, profiles/r01/gnn_epoch_kernels.log).  Here K is split over the grid: each workgroup
// streams a contiguous block of rows once through fp32 MFMA (lane (i, kq) supplies A[row0 + kq][16*dt + i] as the
// A operand and B[row0 + kq][16*ht + i] as the B operand of a 16x16x4 step), keeps all D x H / 256 output tiles in
// registers, folds its four waves through LDS in a fixed order and writes one partial; a second small kernel
// adds the partials in workgroup order.  Deterministic, bound by reading A and B once.
// ------------------------------------------------------------------------------------------
constexpr int kWgUnroll = 4;  // k-steps (of 4 rows) whose loads are in flight together per wave

template <int DT, int HT>
__global__ __launch_bounds__(kUpdWaves * 64) void weight_grad_partial_kernel(const float* __restrict__ A, long long lda,
                                                                             const float* __restrict__ B, long long ldb,
                                                                             float* __restrict__ partial, int N, int D,
                                                                             int H, int rows_per_wg) {
  __shared__ float s_red[(kUpdWaves - 1) * DT * HT * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const long long r_begin = (long long)blockIdx.x * rows_per_wg;
  const long long r_end = min((long long)N, r_begin + rows_per_wg);
  f32x4 acc[DT][HT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) acc[dt][ht] = f32x4{0.f, 0.f, 0.f, 0.f};
  // wave w takes the k-steps w, w + 4, ... of the block; kWgUnroll of them per iteration
  for (long long r0 = r_begin + 4 * wave; r0 < r_end; r0 += 16 * kWgUnroll) {
    float a[kWgUnroll][DT], b[kWgUnroll][HT];
#pragma unroll
    for (int u = 0; u < kWgUnroll; ++u) {
      const long long row = r0 + 16 * u + kq;
      const bool ok = row < r_end;
      const float* ar = A + (ok ? row : r_begin) * lda;
      const float* br = B + (ok ? row : r_begin) * ldb;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) a[u][dt] = (ok && 16 * dt + i < D) ? ar[16 * dt + i] : 0.0f;
#pragma unroll
      for (int ht = 0; ht < HT; ++ht) b[u][ht] = (ok && 16 * ht + i < H) ? br[16 * ht + i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kWgUnroll; ++u)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int ht = 0; ht < HT; ++ht)
          acc[dt][ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][dt], b[u][ht], acc[dt][ht], 0, 0, 0);
  }
  // fold the four waves in wave order (fixed => deterministic)
  if (wave > 0) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int ht = 0; ht < HT; ++ht)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_red[(((wave - 1) * DT + dt) * HT + ht) * 256 + r * 64 + lane] = acc[dt][ht][r];
  }
  __syncthreads();
  if (wave == 0) {
    float* out = partial + (size_t)blockIdx.x * (size_t)D * (size_t)H;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int ht = 0; ht < HT; ++ht)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[dt][ht][r];
#pragma unroll
          for (int w = 0; w < kUpdWaves - 1; ++w) v += s_red[((w * DT + dt) * HT + ht) * 256 + r * 64 + lane];
          const int d = 16 * dt + 4 * kq + r, h = 16 * ht + i;  // accumulator register r of lane (kq, i) is C[4*kq + r][i]
          if (d < D && h < H) out[d * H + h] = v;
        }
  }
}

// out[e] = sum over the G partials, in workgroup order; 64 elements per workgroup, its four waves take alternate
// partials (eight loads in flight each) and are folded through LDS in wave order.
__global__ __launch_bounds__(kUpdWaves * 64) void weight_grad_reduce_kernel(const float* __restrict__ partial,
                                                                            float* __restrict__ out, int G, int DH) {
  __shared__ float s_red[kUpdWaves * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = (int)blockIdx.x * 64 + lane;
  float acc = 0.0f;
  if (e < DH) {
    int g = wave;
    for (; g + 7 * kUpdWaves < G; g += 8 * kUpdWaves) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(g + u * kUpdWaves) * (size_t)DH + e];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; g < G; g += kUpdWaves) acc += partial[(size_t)g * (size_t)DH + e];
  }
  s_red[wave * 64 + lane] = acc;
  __syncthreads();
  if (wave == 0 && e < DH) out[e] = ((s_red[lane] + s_red[64 + lane]) + s_red[128 + lane]) + s_red[192 + lane];
}

int weight_grad_groups(long long N) {  // workgroups of the streaming pass: two per CU, at least 64 rows each
  static const int cap = [] {
    const char* e = getenv("HCSPMM_WG_GROUPS");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? v : 512;
  }();
  long long g = (N + 63) / 64;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

bool weight_grad_supported(int D, int H) {
  const int dt = (D + 15) / 16, ht = (H + 15) / 16;
  return D > 0 && H > 0 && dt <= 8 && ht <= 4 && dt * ht <= 16;
}

template <int DT, int HT>
static hipError_t launch_wg(const float* A, long long lda, const float* B, long long ldb, float* out, float* partial,
                            long long N, int D, int H, hipStream_t stream) {
  const int G = weight_grad_groups(N);
  int rows = (int)((N + G - 1) / G);
  rows = (rows + 15) / 16 * 16;
  hipLaunchKernelGGL((weight_grad_partial_kernel<DT, HT>), dim3(G), dim3(kUpdWaves * 64), 0, stream, A, lda, B, ldb,
                     partial, (int)N, D, H, rows);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(weight_grad_reduce_kernel, dim3((D * H + 63) / 64), dim3(kUpdWaves * 64), 0, stream, partial, out, G,
                     D * H);
  return hipGetLastError();
}

hipError_t launch_weight_grad_reduce(const float* partial, float* out, int G, int DH, hipStream_t stream) {
  hipLaunchKernelGGL(weight_grad_reduce_kernel, dim3((DH + 63) / 64), dim3(kUpdWaves * 64), 0, stream, partial, out, G, DH);
  return hipGetLastError();
}

hipError_t launch_weight_grad(const float* A, long long lda, const float* B, long long ldb, float* out, float* partial,
                              long long N, int D, int H, hipStream_t stream) {
  const int dt = (D + 15) / 16, ht = (H + 15) / 16;
#define HCSPMM_WG_CASE(DT_, HT_) \
  if (dt == DT_ && ht == HT_) return launch_wg<DT_, HT_>(A, lda, B, ldb, out, partial, N, D, H, stream);
  HCSPMM_WG_CASE(1, 1) HCSPMM_WG_CASE(2, 1) HCSPMM_WG_CASE(3, 1) HCSPMM_WG_CASE(4, 1) HCSPMM_WG_CASE(5, 1) HCSPMM_WG_CASE(6, 1)
  HCSPMM_WG_CASE(7, 1) HCSPMM_WG_CASE(8, 1)
  HCSPMM_WG_CASE(1, 2) HCSPMM_WG_CASE(2, 2) HCSPMM_WG_CASE(3, 2) HCSPMM_WG_CASE(4, 2) HCSPMM_WG_CASE(5, 2) HCSPMM_WG_CASE(6, 2)
  HCSPMM_WG_CASE(7, 2) HCSPMM_WG_CASE(8, 2)
  HCSPMM_WG_CASE(1, 3) HCSPMM_WG_CASE(2, 3) HCSPMM_WG_CASE(3, 3) HCSPMM_WG_CASE(4, 3) HCSPMM_WG_CASE(5, 3)
  HCSPMM_WG_CASE(1, 4) HCSPMM_WG_CASE(2, 4) HCSPMM_WG_CASE(3, 4) HCSPMM_WG_CASE(4, 4)
#undef HCSPMM_WG_CASE
  return hipErrorInvalidValue;
}

// Shapes of the LDS-staged streaming kernel: rows of agg in 16-byte pieces (D a multiple of 16, 16-byte aligned), H up to
// 128.  H = 16, 32, 48, 64 with a 16-byte aligned `out` take vector stores (and are what the fused tile launches reproduce
// bit for bit); any other H -- the reference's default 22 classes, a 96-column input layer -- pads the staged weights to the
// next multiple of 16 columns and masks the stores.  (Round 2 sent those to the any-shape kernel below: 1.5-2.4 TB/s against
// 4.5-5 here: 550 -> ~230 us for (32, 22) on the RD-sized graph.)
static bool update_streams_exact(const float* in, const float* out, int D, int H) {
  const bool aligned16 = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  return aligned16 && D % 16 == 0 && H % 16 == 0 && H <= 64 && (size_t)D * (H + 4) * sizeof(float) <= 64 * 1024;
}

bool dense_update_streams(const float* in, const float* out, int D, int H) { return update_streams_exact(in, out, D, H); }

static bool update_streams_padded(const float* in, int D, int H) {
  const int Hp = (H + 15) / 16 * 16;
  return (reinterpret_cast<uintptr_t>(in) & 15) == 0 && D % 16 == 0 && H > 0 && H <= 128 &&
         (size_t)D * (Hp + 4) * sizeof(float) <= 64 * 1024;
}

hipError_t launch_dense_update(const float* in, const float* W, long long ldr, long long ldc, float* out, int N,
                               int D, int H, const int* tile_list, int n_tiles, hipStream_t stream) {
  if (N <= 0 || H <= 0) return hipSuccess;
  if (!tile_list) n_tiles = (N + 15) / 16;
  if (n_tiles <= 0) return hipSuccess;
  if (update_streams_exact(in, out, D, H)) {
    switch (H / 16) {
      case 1: return launch_stream<1, false>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      case 2: return launch_stream<2, false>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      case 3: return launch_stream<3, false>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      default: return launch_stream<4, false>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
    }
  }
  if (update_streams_padded(in, D, H)) {
    switch ((H + 15) / 16) {
      case 1: return launch_stream<1, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      case 2: return launch_stream<2, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      case 3: return launch_stream<3, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      case 4: return launch_stream<4, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      case 5: return launch_stream<5, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      case 6: return launch_stream<6, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      case 7: return launch_stream<7, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      default: return launch_stream<8, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
    }
  }
  // an even input width that is not a multiple of 16 (22 classes): 8-byte loads of agg, H up to 64
  if ((reinterpret_cast<uintptr_t>(in) & 7) == 0 && D % 2 == 0 && D >= 2 && H <= 64 &&
      (size_t)((D + 15) / 16 * 16) * ((H + 15) / 16 * 16 + 4) * sizeof(float) <= 64 * 1024) {
    switch ((H + 15) / 16) {
      case 1: return launch_stream<1, true, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      case 2: return launch_stream<2, true, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      case 3: return launch_stream<3, true, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
      default: return launch_stream<4, true, true>(in, W, ldr, ldc, out, N, D, H, tile_list, n_tiles, stream);
    }
  }
  const int grid = (n_tiles + kUpdWaves - 1) / kUpdWaves;
  hipLaunchKernelGGL(dense_update_kernel, dim3(grid), dim3(kUpdWaves * 64), 0, stream, in, W, ldr, ldc, out, N, D, H,
                     tile_list, n_tiles);
  return hipGetLastError();
}

hipError_t launch_dense_update_leftover(const float* in, const float* W, long long ldr, long long ldc, float* out, int N,
                                        int D, int H, const int* plan, int off_tasks, int n_wide, int off_fixups,
                                        int n_split_rows, int off_slice_tasks, int n_slice_tasks, hipStream_t stream) {
  if (N <= 0 || (long long)n_wide + n_split_rows + n_slice_tasks <= 0) return hipSuccess;
  const int T = (H + 15) / 16;  // output tiles; a width in between is zero-padded to the tile (the row-tile form's shapes)
  if (D < 1 || D > 128 || H < 1 || H > 64 || T == 3) return hipErrorInvalidValue;
#define HCSPMM_ROWS_CASE(T_) \
  return launch_rows<T_>(in, W, ldr, ldc, out, D, H, plan, off_tasks, n_wide, off_fixups, n_split_rows, off_slice_tasks, n_slice_tasks, stream);
  if (T == 4) { HCSPMM_ROWS_CASE(4) }
  if (T == 2) { HCSPMM_ROWS_CASE(2) }
  HCSPMM_ROWS_CASE(1)
#undef HCSPMM_ROWS_CASE
}

}  // namespace hcspmm
