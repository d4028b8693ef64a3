// gatv2_attention.hip -- GATv2 attention logits on the stored entries and their backward (include/hcspmm.h
// hcspmm_gatv2_scores*), fp32: per head h, for entry e of row r with column c,
//   l[h][e] = sum_k att[h][k] * LeakyReLU(H_dst[r][h*Dh + k] + H_src[c][h*Dh + k])
// head-major [heads][E], the layout hcspmm_edge_softmax takes.  The non-linearity sits inside the dot product, so nothing
// factors into per-node scalars: every entry gathers one D-wide row, as in the SDDMM (sddmm_impl.h).
//
//  * gatv2_scores_kernel: the SDDMM's walk (contiguous CSR chunks per wave, the row from one search and a cursor, H_dst's
//    row kept in registers while a lane group's entries stay in one row, kSddmmUnroll gathers in flight).  L lanes own one
//    entry and cover all heads: LH = sddmm_L(Dh, 4) consecutive lanes per head, 16 bytes each, so one column id serves
//    every head.  Per element z = a + b and l = z > 0 ? z : z * slope are rounded on their own (never contracted), then
//    fmaf(att, l, acc) in column order and an xor butterfly over the head's LH lanes: a head's bits are those of a
//    single-head call on its column slice.  More than 64 lanes' worth of columns (heads * LH > 64, or Dh > 256) takes the
//    MULTI build, which walks head groups and column chunks per entry and re-reads its operands.
//  * gatv2_grad_kernel<SIDE>: row-parallel, L = sddmm_L(D, 4) lanes per row, the row's own operand and att in registers,
//    one gathered row and one g per head and entry, the next step's column ids loaded while this step's rows arrive.  A
//    workgroup takes tiles of R consecutive rows (tile b, b + grid, ...: at most kGradMaxBlocks workgroups): rows of up to
//    kGradWaveRow entries by one lane group each, entries in order; up to kGradBlockRow by one wave, entry i by its lane
//    group i mod G, the groups' partial rows folded by an xor butterfly; longer rows by the whole workgroup, entry i by
//    lane group i mod NG, folded by the butterfly and then through LDS in wave order.  The order of every row's sum depends
//    on the row's length (and D) alone.  SIDE = dst also sums g * l per lane over the rows it walks (in a fixed
//    order: the long rows are found by ballot, not by arrival), folds them the same way and writes one [D] partial per
//    workgroup; gatv2_att_fold_kernel adds the partials in index order.  No atomics anywhere: two calls give the same bits.
#include "sddmm_impl.h"

namespace hcspmm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 load4(const float* p) { return *reinterpret_cast<const MemF32<4>::type*>(p); }

// z and l rounded on their own: a host reference reproduces the branch of every element from the fp32 sum's sign
__device__ __forceinline__ float v2_z(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float v2_leaky(float z, float slope) {
#pragma clang fp contract(off)
  return z > 0.f ? z : z * slope;
}

// acc += sum over the lane's four columns of att * LeakyReLU(a + b), in column order
__device__ __forceinline__ float score4(const f32x4& a, const f32x4& b, const f32x4& att, float slope, float acc) {
#pragma unroll
  for (int q = 0; q < 4; ++q) acc = fmaf(att[q], v2_leaky(v2_z(a[q], b[q]), slope), acc);
  return acc;
}

// ---------------------------------------------------------------- forward
// lane `sub` of an entry's L: head sub / LH (of the pass's L / LH heads), columns [4 (sub % LH), +4) of that head's chunk
template <int L, int LH, bool MULTI>
__global__ __launch_bounds__(kSddmmThreads) void gatv2_scores_kernel(Gatv2Args a) {
  constexpr int G = 64 / L, HP = L / LH;
  constexpr long long kChunk = (long long)kSddmmSteps * kSddmmUnroll * G;
  const int lane = threadIdx.x & 63, g = lane / L, sub = lane % L, hh = sub / LH, hs = sub % LH;
  const long long wave = ((long long)blockIdx.x * kSddmmThreads + threadIdx.x) >> 6;
  const long long e0 = wave * kChunk;
  if (e0 >= a.E) return;
  const long long e1 = min(e0 + kChunk, a.E);
  const float* __restrict__ Hd = a.H_dst;
  const float* __restrict__ Hs = a.H_src;
  const int heads = a.heads, Dh = a.D / a.heads;
  const float slope = a.slope;
  // single pass: this lane's columns of the whole run
  const bool live = hh < heads && hs * 4 < Dh;
  const int c0 = live ? hh * Dh + hs * 4 : 0;
  f32x4 att = {0.f, 0.f, 0.f, 0.f};
  if (!MULTI && live) att = load4(a.att + c0);
  long long e = e0 + g;
  int r = row_of(a.rowptr, a.N, e < e1 ? e : e0);
  int next = a.rowptr[r + 1];
  int ra = -1;  // row whose columns sit in `ar`
  f32x4 ar = {0.f, 0.f, 0.f, 0.f};
  for (; e < e1; e += G * kSddmmUnroll) {
    int rows[kSddmmUnroll], cols[kSddmmUnroll];
#pragma unroll
    for (int u = 0; u < kSddmmUnroll; ++u) {  // rows (a cursor: a group's entries ascend) and column ids, once for all heads
      const long long eu = e + (long long)u * G;
      rows[u] = -1;
      if (eu < e1) {
        while (next <= eu) next = a.rowptr[++r + 1];
        rows[u] = r;
        cols[u] = a.col[eu];
      }
    }
    if constexpr (!MULTI) {
      f32x4 bv[kSddmmUnroll], av[kSddmmUnroll];
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u) {  // the gathers, all in flight before any arithmetic
        bv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        av[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (rows[u] >= 0 && live) {
          bv[u] = load4(Hs + (size_t)cols[u] * a.ld_src + c0);
          const int prev = u == 0 ? ra : rows[u - 1];
          if (rows[u] != prev) av[u] = load4(Hd + (size_t)rows[u] * a.ld_dst + c0);
        }
      }
      float acc[kSddmmUnroll];
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u) {
        acc[u] = 0.f;
        if (rows[u] < 0) continue;
        if (rows[u] != ra) {
          ar = av[u];
          ra = rows[u];
        }
        if (live) acc[u] = score4(ar, bv[u], att, slope, 0.f);
      }
#pragma unroll
      for (int off = LH / 2; off > 0; off >>= 1)  // fixed butterfly over the head's lanes
#pragma unroll
        for (int u = 0; u < kSddmmUnroll; ++u) acc[u] += __shfl_xor(acc[u], off, 64);
      if (hs == 0 && hh < heads) {
        float* __restrict__ oh = a.out + (long long)hh * a.E;
#pragma unroll
        for (int u = 0; u < kSddmmUnroll; ++u)
          if (rows[u] >= 0) __builtin_nontemporal_store(acc[u], oh + e + (long long)u * G);
      }
    } else {
      const int n_chunks = (Dh + LH * 4 - 1) / (LH * 4);
      for (int h0 = 0; h0 < heads; h0 += HP) {  // head groups of L / LH heads; operands re-read (L1 / L2 hits)
        const int h = h0 + hh;
        float acc[kSddmmUnroll];
#pragma unroll
        for (int u = 0; u < kSddmmUnroll; ++u) acc[u] = 0.f;
        for (int k = 0; k < n_chunks; ++k) {
          const int ck = (k * LH + hs) * 4;
          if (h < heads && ck < Dh) {
            const int c = h * Dh + ck;
            const f32x4 at = load4(a.att + c);
            f32x4 bv[kSddmmUnroll], av[kSddmmUnroll];
#pragma unroll
            for (int u = 0; u < kSddmmUnroll; ++u) {
              bv[u] = av[u] = f32x4{0.f, 0.f, 0.f, 0.f};
              if (rows[u] >= 0) {
                bv[u] = load4(Hs + (size_t)cols[u] * a.ld_src + c);
                av[u] = load4(Hd + (size_t)rows[u] * a.ld_dst + c);
              }
            }
#pragma unroll
            for (int u = 0; u < kSddmmUnroll; ++u)
              if (rows[u] >= 0) acc[u] = score4(av[u], bv[u], at, slope, acc[u]);
          }
        }
#pragma unroll
        for (int off = LH / 2; off > 0; off >>= 1)
#pragma unroll
          for (int u = 0; u < kSddmmUnroll; ++u) acc[u] += __shfl_xor(acc[u], off, 64);
        if (hs == 0 && h < heads) {
          float* __restrict__ oh = a.out + (long long)h * a.E;
#pragma unroll
          for (int u = 0; u < kSddmmUnroll; ++u)
            if (rows[u] >= 0) __builtin_nontemporal_store(acc[u], oh + e + (long long)u * G);
        }
      }
    }
  }
}

template <int L, int LH, bool MULTI>
hipError_t launch_scores_LL(const Gatv2Args& a, hipStream_t stream) {
  constexpr long long kChunk = (long long)kSddmmSteps * kSddmmUnroll * (64 / L);
  const long long waves = (a.E + kChunk - 1) / kChunk;
  const long long blocks = (waves + kSddmmThreads / 64 - 1) / (kSddmmThreads / 64);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((gatv2_scores_kernel<L, LH, MULTI>), dim3((unsigned)blocks), dim3(kSddmmThreads), 0, stream, a);
  return hipGetLastError();
}

template <int L>
hipError_t launch_scores_L(const Gatv2Args& a, int lh, hipStream_t stream) {
  switch (lh) {
    case 1: return launch_scores_LL<L, 1, false>(a, stream);
    case 2: if constexpr (L >= 2) return launch_scores_LL<L, 2, false>(a, stream); break;
    case 4: if constexpr (L >= 4) return launch_scores_LL<L, 4, false>(a, stream); break;
    case 8: if constexpr (L >= 8) return launch_scores_LL<L, 8, false>(a, stream); break;
    case 16: if constexpr (L >= 16) return launch_scores_LL<L, 16, false>(a, stream); break;
    case 32: if constexpr (L >= 32) return launch_scores_LL<L, 32, false>(a, stream); break;
    case 64: if constexpr (L >= 64) return launch_scores_LL<L, 64, false>(a, stream); break;
  }
  return hipErrorInvalidValue;
}

hipError_t launch_scores_multi(const Gatv2Args& a, int lh, hipStream_t stream) {
  switch (lh) {
    case 1: return launch_scores_LL<64, 1, true>(a, stream);
    case 2: return launch_scores_LL<64, 2, true>(a, stream);
    case 4: return launch_scores_LL<64, 4, true>(a, stream);
    case 8: return launch_scores_LL<64, 8, true>(a, stream);
    case 16: return launch_scores_LL<64, 16, true>(a, stream);
    case 32: return launch_scores_LL<64, 32, true>(a, stream);
    default: return launch_scores_LL<64, 64, true>(a, stream);
  }
}

// ---------------------------------------------------------------- backward
constexpr int kGradThreads = 256;
constexpr int kGradWaves = kGradThreads / 64;
constexpr int kGradRowsPerGroup = 4;  // rows a lane group takes in turn: a workgroup covers 4 * (256 / L) rows
constexpr int kGradWaveRow = 32;     // rows longer than this: one wave (its 64 / L lane groups); up to it: one lane group
constexpr int kGradBlockRow = 256;    // rows longer than this: the whole workgroup
constexpr int kGradUnroll = 4;        // entries per lane group per step
constexpr int kGradMaxBlocks = 4096;  // workgroups of a row launch: beyond, a workgroup takes tiles b, b + 4096, ...

// sum of v over the lane groups of a workgroup, valid in wave 0 / group 0: an xor butterfly over the wave's 64 / L groups,
// then the wave partials in wave order through LDS
template <int L>
__device__ __forceinline__ f32x4 wave_fold4(f32x4 v) {  // sum over the wave's 64 / L lane groups, the same bits in all of them
#pragma unroll
  for (int off = L; off < 64; off <<= 1)
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] += __shfl_xor(v[q], off, 64);
  return v;
}

template <int L>
__device__ __forceinline__ f32x4 block_fold4(f32x4 v, float (*red)[L * 4], int wid, int g, int sub) {
  v = wave_fold4<L>(v);
  __syncthreads();  // (red[] of the previous fold has been read)
  if (g == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) red[wid][sub * 4 + q] = v[q];
  }
  __syncthreads();
  if (wid == 0 && g == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float w = red[0][sub * 4 + q];
#pragma unroll
      for (int k = 1; k < kGradWaves; ++k) w += red[k][sub * 4 + q];
      v[q] = w;
    }
  }
  return v;
}

// SIDE 0: grad_H_dst (own = H_dst[r], gathered = H_src[col], g[e]) and the att partials; SIDE 1: grad_H_src (own =
// H_src[c], gathered = H_dst[col_t], g[perm[e]], over the rows of A^T)
template <int SIDE, int L>
__global__ __launch_bounds__(kGradThreads) void gatv2_grad_kernel(Gatv2Args a) {
  constexpr int G = 64 / L, NG = kGradWaves * G, R = NG * kGradRowsPerGroup;
  constexpr int kMaskIters = (R + kGradThreads - 1) / kGradThreads;
  __shared__ unsigned long long longmask[kMaskIters * kGradWaves], midmask[kMaskIters * kGradWaves];
  __shared__ float red[kGradWaves][L * 4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane / L, sub = lane % L, gid = wid * G + g;
  const int N = SIDE == 0 ? a.N : a.n_t, D = a.D, Dh = a.D / a.heads;
  const float slope = a.slope;
  const float* __restrict__ own = SIDE == 0 ? a.H_dst : a.H_src;
  const float* __restrict__ oth = SIDE == 0 ? a.H_src : a.H_dst;
  const size_t ld_own = SIDE == 0 ? a.ld_dst : a.ld_src, ld_oth = SIDE == 0 ? a.ld_src : a.ld_dst;
  float* __restrict__ out = SIDE == 0 ? a.grad_dst : a.grad_src;
  const size_t ld_out = SIDE == 0 ? a.ld_gdst : a.ld_gsrc;
  const int* __restrict__ rowptr = SIDE == 0 ? a.rowptr : a.rowptr_t;
  const int* __restrict__ colp = SIDE == 0 ? a.col : a.col_t;
  const int n_tiles = (N + R - 1) / R;
  for (int cb = 0; cb < D; cb += L * 4) {  // one pass unless D > 256
    const int c = cb + sub * 4;
    const bool live = c < D;
    const int cs = live ? c : 0;
    const f32x4 att = live ? load4(a.att + cs) : f32x4{0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ gh = a.g + (long long)(cs / Dh) * a.E;
    f32x4 gl = {0.f, 0.f, 0.f, 0.f};  // SIDE 0: this lane's sum of g * l
    // acc += entries first, first + stride, ... < n of the row that starts at b
    auto walk = [&](const f32x4& mine, long long b, int n, int first, int stride, f32x4& acc) {
      int cc[kGradUnroll];
      long long ge[kGradUnroll];
      auto indices = [&](int i) {  // column ids and g positions of the step that starts at entry i
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {
          const int iu = i + u * stride;
          cc[u] = -1;
          if (iu < n) {
            cc[u] = colp[b + iu];
            ge[u] = SIDE == 0 ? b + iu : (long long)a.perm[b + iu];
          }
        }
      };
      indices(first);
      for (int i = first; i < n; i += stride * kGradUnroll) {
        f32x4 ov[kGradUnroll];
        float gv[kGradUnroll];
        bool on[kGradUnroll];
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {  // the gathers, all in flight before any arithmetic
          ov[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          gv[u] = 0.f;
          on[u] = cc[u] >= 0;
          if (on[u]) {
            ov[u] = load4(oth + (size_t)cc[u] * ld_oth + c);
            gv[u] = gh[ge[u]];
          }
        }
        indices(i + stride * kGradUnroll);  // the next step's indices travel while this step's rows arrive
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {
          if (!on[u]) continue;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float z = v2_z(mine[q], ov[u][q]);
            acc[q] = fmaf(gv[u], z > 0.f ? 1.f : slope, acc[q]);
            if constexpr (SIDE == 0) gl[q] = fmaf(gv[u], v2_leaky(z, slope), gl[q]);
          }
        }
      }
    };
    auto store_row = [&](int r, const f32x4& acc) {
      f32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = att[q] * acc[q];
      __builtin_nontemporal_store(o, reinterpret_cast<MemF32<4>::type*>(out + (size_t)r * ld_out + c));
    };
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // tiles of R rows in turn: a fixed assignment
      const int r0 = tile * R;
      // the tile's wave rows and workgroup rows as bit masks in row order (lists filled by arrival would let timing into the
      // att sums)
#pragma unroll
      for (int k = 0; k < kMaskIters; ++k) {
        const int i = k * kGradThreads + tid;
        int n = 0;
        if (i < R && r0 + i < N) n = rowptr[r0 + i + 1] - rowptr[r0 + i];
        const unsigned long long ml = __ballot(n > kGradBlockRow), mm = __ballot(n > kGradWaveRow && n <= kGradBlockRow);
        if (lane == 0) {
          longmask[k * kGradWaves + wid] = ml;
          midmask[k * kGradWaves + wid] = G > 1 ? mm : 0ull;  // (L = 64: a wave is one lane group)
        }
      }
      __syncthreads();
      // rows of up to kGradWaveRow entries: one lane group each
      for (int k = 0; k < kGradRowsPerGroup; ++k) {
        const int r = r0 + k * NG + gid;
        if (r >= N) break;
        const long long b = rowptr[r];
        const int n = rowptr[r + 1] - (int)b;
        if (n > (G > 1 ? kGradWaveRow : kGradBlockRow)) continue;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (n > 0 && live) {
          const f32x4 mine = load4(own + (size_t)r * ld_own + c);
          walk(mine, b, n, 0, 1, acc);
        }
        if (live) store_row(r, acc);
      }
      // rows of up to kGradBlockRow entries: the k-th of them in row order by wave k mod 4, entry i by its lane group i mod G
      if constexpr (G > 1) {
        int turn = 0;
        for (int w = 0; w < kMaskIters * kGradWaves; ++w) {
          unsigned long long m = midmask[w];
          while (m) {
            const int r = r0 + w * 64 + (__ffsll((long long)m) - 1);
            m &= m - 1;
            if (turn++ % kGradWaves != wid) continue;
            const long long b = rowptr[r];
            const int n = rowptr[r + 1] - (int)b;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if (live) {
              const f32x4 mine = load4(own + (size_t)r * ld_own + c);
              walk(mine, b, n, g, G, acc);
            }
            acc = wave_fold4<L>(acc);
            if (g == 0 && live) store_row(r, acc);
          }
        }
      }
      // longer rows: the whole workgroup, in row order
      for (int w = 0; w < kMaskIters * kGradWaves; ++w) {
        unsigned long long m = longmask[w];
        while (m) {
          const int r = r0 + w * 64 + (__ffsll((long long)m) - 1);
          m &= m - 1;
          const long long b = rowptr[r];
          const int n = rowptr[r + 1] - (int)b;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          if (live) {
            const f32x4 mine = load4(own + (size_t)r * ld_own + c);
            walk(mine, b, n, gid, NG, acc);
          }
          acc = block_fold4<L>(acc, red, wid, g, sub);
          if (wid == 0 && g == 0 && live) store_row(r, acc);
        }
      }
      __syncthreads();  // (longmask has been read by every thread)
    }
    if constexpr (SIDE == 0) {  // this workgroup's partial of grad_att, columns [cb, cb + 4 L)
      gl = block_fold4<L>(gl, red, wid, g, sub);
      if (wid == 0 && g == 0 && live)
        *reinterpret_cast<MemF32<4>::type*>(a.partial + (size_t)blockIdx.x * D + c) = gl;
    }
  }
}

// grad_att[j] = sum of the workgroups' partials in index order: 16 interleaved series per column, then those in order
constexpr int kFoldCols = 16, kFoldParts = 16;
__global__ __launch_bounds__(kFoldCols* kFoldParts) void gatv2_att_fold_kernel(const float* __restrict__ partial, int n_blocks,
                                                                                int D, float* __restrict__ grad_att) {
  __shared__ float red[kFoldParts][kFoldCols];
  const int cj = threadIdx.x % kFoldCols, part = threadIdx.x / kFoldCols, j = blockIdx.x * kFoldCols + cj;
  float s = 0.f;
  if (j < D)
    for (int b = part; b < n_blocks; b += kFoldParts) s += partial[(size_t)b * D + j];
  red[part][cj] = s;
  __syncthreads();
  if (part == 0 && j < D) {
    float w = red[0][cj];
#pragma unroll
    for (int k = 1; k < kFoldParts; ++k) w += red[k][cj];
    grad_att[j] = w;
  }
}

template <int L>
hipError_t launch_grad_L(const Gatv2Args& a, hipStream_t stream) {
  if (a.N > 0) {
    const unsigned blocks = (unsigned)gatv2_grad_blocks(a.N, a.D);
    hipLaunchKernelGGL((gatv2_grad_kernel<0, L>), dim3(blocks), dim3(kGradThreads), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.n_t > 0) {
    const unsigned blocks_t = (unsigned)gatv2_grad_blocks(a.n_t, a.D);
    hipLaunchKernelGGL((gatv2_grad_kernel<1, L>), dim3(blocks_t), dim3(kGradThreads), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace

// workgroups of the backward's row launches (= [D] partials of grad_att): a function of (N, D) alone
long long gatv2_grad_blocks(long long N, int D) {
  const int rows = kGradWaves * (64 / sddmm_L(D, 4)) * kGradRowsPerGroup;
  const long long tiles = (N + rows - 1) / rows;
  return tiles < kGradMaxBlocks ? tiles : kGradMaxBlocks;
}

hipError_t launch_gatv2_scores(const Gatv2Args& a, hipStream_t stream) {
  if (a.heads <= 0 || a.D <= 0 || a.D % a.heads != 0 || (a.D / a.heads) % 4 != 0) return hipErrorInvalidValue;
  if (a.N == 0 || a.E == 0) return hipSuccess;
  const int dh = a.D / a.heads, lh = sddmm_L(dh, 4);
  if ((long long)a.heads * lh > 64 || dh > 64 * 4) return launch_scores_multi(a, lh, stream);
  int L = lh;
  while (L < a.heads * lh) L <<= 1;
  switch (L) {
    case 1: return launch_scores_L<1>(a, lh, stream);
    case 2: return launch_scores_L<2>(a, lh, stream);
    case 4: return launch_scores_L<4>(a, lh, stream);
    case 8: return launch_scores_L<8>(a, lh, stream);
    case 16: return launch_scores_L<16>(a, lh, stream);
    case 32: return launch_scores_L<32>(a, lh, stream);
    default: return launch_scores_L<64>(a, lh, stream);
  }
}

hipError_t launch_gatv2_backward(const Gatv2Args& a, hipStream_t stream) {
  if (a.heads <= 0 || a.D <= 0 || a.D % a.heads != 0 || (a.D / a.heads) % 4 != 0) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if (a.N > 0 || a.n_t > 0) {
    switch (sddmm_L(a.D, 4)) {
      case 1: e = launch_grad_L<1>(a, stream); break;
      case 2: e = launch_grad_L<2>(a, stream); break;
      case 4: e = launch_grad_L<4>(a, stream); break;
      case 8: e = launch_grad_L<8>(a, stream); break;
      case 16: e = launch_grad_L<16>(a, stream); break;
      case 32: e = launch_grad_L<32>(a, stream); break;
      default: e = launch_grad_L<64>(a, stream); break;
    }
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(gatv2_att_fold_kernel, dim3((unsigned)((a.D + kFoldCols - 1) / kFoldCols)), dim3(kFoldCols * kFoldParts), 0,
                     stream, a.partial, (int)gatv2_grad_blocks(a.N, a.D), a.D, a.grad_att);
  return hipGetLastError();
}

}  // namespace hcspmm
