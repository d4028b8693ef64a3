// gat_attention.hip -- GAT attention on the stored entries (include/hcspmm.h hcspmm_gat_attention*, DESIGN.md section
// 3.10): per head h, for entry e of row r with column c,
//   z = s_dst[r][h] + s_src[c][h],  l = LeakyReLU(z),  alpha[h][e] = softmax of l over row r's entries,
// and its backward, without storing z or l.  Scores are node-major [rows][heads], alpha and the gradients of the logits
// head-major [heads][E].
//
//  * Rows are walked by the edge softmax's scheme (sddmm_impl.h): one thread per row up to kShortRow entries, one wave up
//    to kBlockRow, the whole workgroup beyond, with its fold order.  Each head's sums are those of hcspmm_edge_softmax on
//    the stored l, term for term, so alpha has its bits; the heads of a group (up to 4) share each column-id load and the
//    row's s_dst.
//  * Backward, launch 1: per row d = sum alpha * grad_alpha, g = alpha (grad_alpha - d) LeakyReLU'(z) written to
//    grad_scores, and grad_s_dst = the row's sum of g.  Launch 2: grad_s_src[c] = sum over row c of g[perm[e']] (the
//    transpose of a pattern-symmetric graph in A's CSR order).  Fixed orders throughout, no atomics: deterministic.
#include "sddmm_impl.h"

namespace hcspmm {
namespace {



// z and l exactly as torch rounds them: the product z * slope stays a rounded product, never fused into exp_diff's x - m
// (hipcc contracts by default; a fused l would move alpha off the stored-logit softmax's bits)
__device__ __forceinline__ float gat_z(float sd, float ss) {
#pragma clang fp contract(off)
  return sd + ss;
}
__device__ __forceinline__ float gat_leaky(float z, float slope) {
#pragma clang fp contract(off)
  return z > 0.f ? z : z * slope;
}

// folds of HG per-head values over the threads that share a row -- per head, the edge softmax's own folds
struct ThreadFold {
  template <int HG>
  __device__ __forceinline__ void operator()(float (&)[HG], bool) const {}
};
struct WaveFold {
  template <int HG>
  __device__ __forceinline__ void operator()(float (&v)[HG], bool is_max) const {
#pragma unroll
    for (int j = 0; j < HG; ++j) v[j] = wave_fold(v[j], is_max);
  }
};
template <int HG>
struct BlockFold {  // waves fold, then wave partials in wave order (edge_softmax_kernel's block_fold, all heads at once)
  float (*part)[kSoftmaxThreads / 64];
  int lane, wid;
  __device__ __forceinline__ void operator()(float (&v)[HG], bool is_max) const {
#pragma unroll
    for (int j = 0; j < HG; ++j) v[j] = wave_fold(v[j], is_max);
    __syncthreads();  // (part[] of the previous fold has been read by every thread)
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < HG; ++j) part[j][wid] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < HG; ++j) {
      float w = part[j][0];
#pragma unroll
      for (int k = 1; k < kSoftmaxThreads / 64; ++k) w = is_max ? fmaxf(w, part[j][k]) : w + part[j][k];
      v[j] = w;
    }
  }
};

// Workgroup b covers rows [256 b, 256 b + 256) as edge_softmax_kernel does: short rows by their own thread, the others
// listed in LDS and taken by the waves in turn, or by the whole workgroup.  row(r, b, n, t, nt, h0, fold) runs the heads
// [h0, h0 + HG) of row r (entries [b, b + n)) as thread t of nt.
template <int HG, typename Row>
__device__ __forceinline__ void walk_rows(const int* __restrict__ rowptr, int N, int heads, Row row) {
  __shared__ int wave_rows[kSoftmaxThreads], block_rows[kSoftmaxThreads];
  __shared__ int n_wave, n_block;
  __shared__ float part[HG][kSoftmaxThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) n_wave = n_block = 0;
  __syncthreads();
  const int r = blockIdx.x * kSoftmaxThreads + tid;
  if (r < N) {
    const long long b = rowptr[r];
    const int n = rowptr[r + 1] - (int)b;
    if (n <= kShortRow) {
      for (int h0 = 0; h0 < heads; h0 += HG) row(r, b, n, 0, 1, h0, ThreadFold());
    } else if (n <= kBlockRow) {
      wave_rows[atomicAdd(&n_wave, 1)] = r;
    } else {
      block_rows[atomicAdd(&n_block, 1)] = r;
    }
  }
  __syncthreads();
  for (int i = wid; i < n_wave; i += kSoftmaxThreads / 64) {
    const int rr = wave_rows[i];
    const long long b = rowptr[rr];
    const int n = rowptr[rr + 1] - (int)b;
    for (int h0 = 0; h0 < heads; h0 += HG) row(rr, b, n, lane, 64, h0, WaveFold());
  }
  const BlockFold<HG> block_fold{part, lane, wid};
  for (int i = 0; i < n_block; ++i) {
    const int rr = block_rows[i];
    const long long b = rowptr[rr];
    const int n = rowptr[rr + 1] - (int)b;
    for (int h0 = 0; h0 < heads; h0 += HG) row(rr, b, n, tid, kSoftmaxThreads, h0, block_fold);
  }
}

// The kernels below run heads [h0, h0 + HG) with HG dividing heads (gat_group): every group is whole, no head is masked.

// forward: alpha = softmax of l over the row, per head (edge_softmax_kernel<false> on the stored l, bit for bit)
template <int HG>
__global__ __launch_bounds__(kSoftmaxThreads) void gat_attention_kernel(GatArgs a) {
  const int H = a.heads;
  walk_rows<HG>(a.rowptr, a.N, H, [&](int r, long long b, int n, int t, int nt, int h0, auto fold) {
    float* __restrict__ out = a.out + (long long)h0 * a.E + b;
    float sd[HG], m[HG], s[HG];
#pragma unroll
    for (int j = 0; j < HG; ++j) {
      sd[j] = a.s_dst[(long long)r * H + h0 + j];
      m[j] = -INFINITY;
      s[j] = 0.f;
    }
    for (int i = t; i < n; i += nt) {  // pass 1: m = max l
      const float* ss = a.s_src + (long long)a.col[b + i] * H + h0;
#pragma unroll
      for (int j = 0; j < HG; ++j) m[j] = fmaxf(m[j], gat_leaky(gat_z(sd[j], ss[j]), a.slope));
    }
    fold(m, true);
    for (int i = t; i < n; i += nt) {  // pass 2: s = sum exp(l - m)
      const float* ss = a.s_src + (long long)a.col[b + i] * H + h0;
#pragma unroll
      for (int j = 0; j < HG; ++j) s[j] += exp_diff(gat_leaky(gat_z(sd[j], ss[j]), a.slope), m[j]);
    }
    fold(s, false);
    for (int i = t; i < n; i += nt) {  // pass 3: alpha = exp(l - m) / s
      const float* ss = a.s_src + (long long)a.col[b + i] * H + h0;
      float sv[HG];  // (all gathers before the first store: out may alias s_src as far as the compiler knows)
#pragma unroll
      for (int j = 0; j < HG; ++j) sv[j] = ss[j];
#pragma unroll
      for (int j = 0; j < HG; ++j) out[j * a.E + i] = exp_diff(gat_leaky(gat_z(sd[j], sv[j]), a.slope), m[j]) / s[j];
    }
  });
}

// backward, launch 1: g = alpha (grad_alpha - d) LeakyReLU'(z) and grad_s_dst = the row's sum of g
template <int HG>
__global__ __launch_bounds__(kSoftmaxThreads) void gat_attention_rows_kernel(GatArgs a) {
  const int H = a.heads;
  walk_rows<HG>(a.rowptr, a.N, H, [&](int r, long long b, int n, int t, int nt, int h0, auto fold) {
    const long long o = (long long)h0 * a.E + b;
    const float* __restrict__ al = a.alpha + o;
    const float* __restrict__ ga = a.grad_alpha + o;
    float* __restrict__ out = a.out + o;
    float sd[HG], d[HG], acc[HG];
#pragma unroll
    for (int j = 0; j < HG; ++j) {
      sd[j] = a.s_dst[(long long)r * H + h0 + j];
      d[j] = acc[j] = 0.f;
    }
    for (int i = t; i < n; i += nt) {  // pass 1: d = sum alpha * grad_alpha (the edge softmax backward's order)
#pragma unroll
      for (int j = 0; j < HG; ++j) d[j] = fmaf(al[j * a.E + i], ga[j * a.E + i], d[j]);
    }
    fold(d, false);
    for (int i = t; i < n; i += nt) {  // pass 2: g, and its row sum
      const float* ss = a.s_src + (long long)a.col[b + i] * H + h0;
      float sv[HG], av[HG], gv[HG];  // (all loads before the first store, as in the forward's pass 3)
#pragma unroll
      for (int j = 0; j < HG; ++j) {
        sv[j] = ss[j];
        av[j] = al[j * a.E + i];
        gv[j] = ga[j * a.E + i];
      }
#pragma unroll
      for (int j = 0; j < HG; ++j) {
        const float gl = av[j] * (gv[j] - d[j]);  // gradient of l: edge_softmax_backward's bits
        const float g = gat_z(sd[j], sv[j]) > 0.f ? gl : gl * a.slope;
        out[j * a.E + i] = g;
        acc[j] += g;
      }
    }
    fold(acc, false);
    if (t == 0) {
#pragma unroll
      for (int j = 0; j < HG; ++j) a.grad_s_dst[(long long)r * H + h0 + j] = acc[j];
    }
  });
}

// backward, launch 2: grad_s_src[c] = sum over the entries e' of row c of A^T of g[perm[e']]
template <int HG>
__global__ __launch_bounds__(kSoftmaxThreads) void gat_attention_cols_kernel(GatArgs a) {
  const int H = a.heads;
  walk_rows<HG>(a.rowptr_t, a.n_t, H, [&](int r, long long b, int n, int t, int nt, int h0, auto fold) {
    const float* __restrict__ g = a.out + (long long)h0 * a.E;
    float acc[HG];
#pragma unroll
    for (int j = 0; j < HG; ++j) acc[j] = 0.f;
    for (int i = t; i < n; i += nt) {
      const int p = a.perm[b + i];
#pragma unroll
      for (int j = 0; j < HG; ++j) acc[j] += g[j * a.E + p];
    }
    fold(acc, false);
    if (t == 0) {
#pragma unroll
      for (int j = 0; j < HG; ++j) a.grad_s_src[(long long)r * H + h0 + j] = acc[j];
    }
  });
}

// heads per group: the largest of 4, 3, 2, 1 that divides heads (heads 1-4: one group, each column id loaded once)
inline int gat_group(int heads) { return heads % 4 == 0 ? 4 : heads % 3 == 0 ? 3 : heads % 2 == 0 ? 2 : 1; }

#define HCSPMM_GAT_LAUNCH(KERNEL, ARGS, ROWS, STREAM)                                                       \
  do {                                                                                                      \
    const unsigned blocks_ = (unsigned)(((ROWS) + kSoftmaxThreads - 1) / kSoftmaxThreads);                  \
    switch (gat_group((ARGS).heads)) {                                                                      \
      case 4: hipLaunchKernelGGL(KERNEL<4>, dim3(blocks_), dim3(kSoftmaxThreads), 0, STREAM, ARGS); break;  \
      case 3: hipLaunchKernelGGL(KERNEL<3>, dim3(blocks_), dim3(kSoftmaxThreads), 0, STREAM, ARGS); break;  \
      case 2: hipLaunchKernelGGL(KERNEL<2>, dim3(blocks_), dim3(kSoftmaxThreads), 0, STREAM, ARGS); break;  \
      default: hipLaunchKernelGGL(KERNEL<1>, dim3(blocks_), dim3(kSoftmaxThreads), 0, STREAM, ARGS); break; \
    }                                                                                                       \
  } while (0)

}  // namespace

hipError_t launch_gat_attention(const GatArgs& a, hipStream_t stream) {
  if (a.heads <= 0) return hipErrorInvalidValue;
  if (a.N == 0 || a.E == 0) return hipSuccess;
  HCSPMM_GAT_LAUNCH(gat_attention_kernel, a, a.N, stream);
  return hipGetLastError();
}

hipError_t launch_gat_attention_backward(const GatArgs& a, hipStream_t stream) {
  if (a.heads <= 0) return hipErrorInvalidValue;
  if (a.N == 0 && a.n_t == 0) return hipSuccess;
  if (a.N > 0) {
    HCSPMM_GAT_LAUNCH(gat_attention_rows_kernel, a, a.N, stream);  // every row writes its grad_s_dst, empty rows zeros
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.n_t > 0) HCSPMM_GAT_LAUNCH(gat_attention_cols_kernel, a, a.n_t, stream);
  return hipGetLastError();
}

}  // namespace hcspmm
