// gatv2_attention16.hip -- GATv2 attention logits and their backward on fp16 / bf16 node rows (the 16-bit dtypes of
// hcspmm_gatv2_scores_typed / hcspmm_gatv2_scores_backward_typed): per head h, for entry e of row r with
// column c,
//   l[h][e] = sum_k att[h][k] * LeakyReLU(H_dst[r][h*Dh + k] + H_src[c][h*Dh + k])
// with H_dst / H_src in 16 bits, att, the logits (head-major [heads][E]) and every sum in fp32.  The step's traffic is row gathers
// -- one D-wide row per entry in the forward, two in the backward -- and they halve here: rows travel as raw dwords (Lane<E, VEC>:
// 8 columns in one 16-byte load, 4 when Dh % 8 != 0), stay raw while they wait in registers and are widened pair by pair where they
// are used.  Widening is exact, so z = a + b and l = z > 0 ? z : z * slope are the fp32 unit's roundings on the same values.
//
//  * gatv2_scores16_kernel: sddmm_impl.h's edge-parallel walk (contiguous CSR chunks per wave, row_of once and a cursor,
//    kSddmmUnroll gathers in flight before any arithmetic).  One lane group spans the entry's whole row of heads * Dh columns, as in
//    sddmm_heads16.hip: a lane owns VEC columns inside one head, so one column id and one row search serve every head and each
//    H_src row is gathered once.  H_dst's row stays in registers (raw) while the group's entries stay in one row, att in VEC fp32
//    registers.  Per lane fmaf(att, l, acc) in column order; then a segmented reduction over the Dh / VEC lanes of each head: an xor
//    butterfly where that count is a power of two, else the head's first lane adds its neighbours in lane order -- fixed by
//    (Dh, VEC) alone.  The head's first lane writes the logit with a non-temporal store: every (h, e) exactly once, no atomics.
//  * gatv2_grad16_kernel<SIDE>: the fp32 unit's row-parallel scheme and determinism contract (fixed tile assignment, ballot-built
//    masks, no atomics) on L = D / VEC lanes per row (rounded up to a power of two), so a wave holds twice the rows of the fp32
//    launch at the same D and the grid never exceeds gatv2_grad_blocks(N, D).  Rows of up to kG16WaveRow entries by one lane group,
//    up to kG16BlockRow by one wave (entry i by lane group i mod G), longer ones by the workgroup (i mod NG); folded by an xor
//    butterfly, then through LDS in wave order.  The row's own operand stays raw, gathered rows are 16-byte loads, the next step's
//    column ids are loaded while this step's rows arrive.  fp32 sums, att * acc in fp32, stored as fp32 or rounded once to the
//    operands' type (16-byte non-temporal stores).  SIDE = dst also sums g * l per lane in a fixed order and writes one [D] partial
//    per workgroup; gatv2_att16_fold_kernel adds them in index order.
#include "sddmm_impl.h"

#include "hcspmm.h"

namespace hcspmm {
namespace {

// z and l rounded on their own, as in gatv2_attention.hip: a host reference reproduces every branch from the fp32 sum's sign
__device__ __forceinline__ float v216_z(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float v216_leaky(float z, float slope) {
#pragma clang fp contract(off)
  return z > 0.f ? z : z * slope;
}

// ---------------------------------------------------------------- forward
constexpr int kV216MinWaves = 4;

// a.D = heads * dh (the whole row), L * VEC >= a.D
template <typename E, int L, int VEC>
__global__ __launch_bounds__(kSddmmThreads, kV216MinWaves) void gatv2_scores16_kernel(Gatv2Args16 a, int dh) {
  typedef typename E::T T;
  typedef Lane<E, VEC> LN;
  typedef typename LN::raw_t raw_t;
  typedef typename LN::acc_t acc_t;
  constexpr int G = 64 / L;
  constexpr long long kChunk = (long long)kSddmmSteps * kSddmmUnroll * G;
  const int lane = threadIdx.x & 63, g = lane / L, sub = lane % L;
  const long long wave = ((long long)blockIdx.x * kSddmmThreads + threadIdx.x) >> 6;
  const long long e0 = wave * kChunk;
  if (e0 >= a.E) return;
  const long long e1 = min(e0 + kChunk, a.E);
  const T* __restrict__ Hd = reinterpret_cast<const T*>(a.H_dst);
  const T* __restrict__ Hs = reinterpret_cast<const T*>(a.H_src);
  const float slope = a.slope;
  const int c = sub * VEC;  // (D % VEC == 0: no lane is moved back)
  const bool live = c < a.D;
  const int lh = dh / VEC;  // lanes per head
  const int head = live ? c / dh : 0;
  const bool first = live && c - head * dh == 0;  // the head's first lane
  const bool pow2 = (lh & (lh - 1)) == 0;
  const acc_t att = live ? LN::load_partial(a.att + c) : azero<VEC>();
  float* __restrict__ oh = a.out + (long long)head * a.E;
  long long e = e0 + g;
  int r = row_of(a.rowptr, a.N, e < e1 ? e : e0);
  int next = a.rowptr[r + 1];
  int ra = -1;  // row whose H_dst columns sit in `ar`
  raw_t ar = LN::zero();
  for (; e < e1; e += G * kSddmmUnroll) {
    int rows[kSddmmUnroll], cols[kSddmmUnroll];
    raw_t bv[kSddmmUnroll], av[kSddmmUnroll];
#pragma unroll
    for (int u = 0; u < kSddmmUnroll; ++u) {  // rows (a cursor: a group's entries ascend) and column ids, once for all heads
      const long long eu = e + (long long)u * G;
      rows[u] = -1;
      cols[u] = 0;
      if (eu < e1) {
        while (next <= eu) next = a.rowptr[++r + 1];
        rows[u] = r;
        cols[u] = a.col[eu];
      }
    }
#pragma unroll
    for (int u = 0; u < kSddmmUnroll; ++u) {  // the gathers, all in flight before any arithmetic
      bv[u] = LN::zero();
      av[u] = LN::zero();
      if (rows[u] >= 0 && live) {
        bv[u] = LN::load(Hs + (size_t)cols[u] * a.ld_src + c);
        const int prev = u == 0 ? ra : rows[u - 1];
        if (rows[u] != prev) av[u] = LN::load(Hd + (size_t)rows[u] * a.ld_dst + c);
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
      if (live) {
#pragma unroll
        for (int q = 0; q < VEC; ++q)  // the dwords widened pair by pair, column order
          acc[u] = fmaf(aget(att, q), v216_leaky(v216_z(LN::elem(ar, q), LN::elem(bv[u], q)), slope), acc[u]);
      }
    }
    if (pow2) {  // heads start at multiples of lh lanes: the butterfly stays inside the head
      for (int off = lh >> 1; off > 0; off >>= 1)
#pragma unroll
        for (int u = 0; u < kSddmmUnroll; ++u) acc[u] += __shfl_xor(acc[u], off, 64);
    } else {  // lane order: ((s0 + s1) + s2) + ...
      float sum[kSddmmUnroll];
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u) sum[u] = acc[u];
      for (int t = 1; t < lh; ++t)
#pragma unroll
        for (int u = 0; u < kSddmmUnroll; ++u) sum[u] += __shfl(acc[u], (lane + t) & 63, 64);
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u) acc[u] = sum[u];
    }
    if (first) {
#pragma unroll
      for (int u = 0; u < kSddmmUnroll; ++u)
        if (rows[u] >= 0) __builtin_nontemporal_store(acc[u], oh + e + (long long)u * G);
    }
  }
}

template <typename E, int L, int VEC>
hipError_t launch_scores16_LV(const Gatv2Args16& a, int dh, hipStream_t stream) {
  constexpr long long kChunk = (long long)kSddmmSteps * kSddmmUnroll * (64 / L);
  const long long waves = (a.E + kChunk - 1) / kChunk;
  const long long blocks = (waves + kSddmmThreads / 64 - 1) / (kSddmmThreads / 64);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((gatv2_scores16_kernel<E, L, VEC>), dim3((unsigned)blocks), dim3(kSddmmThreads), 0, stream, a, dh);
  return hipGetLastError();
}

// ---------------------------------------------------------------- backward
constexpr int kG16Threads = 256;
constexpr int kG16Waves = kG16Threads / 64;
constexpr int kG16RowsPerGroup = 4;  // rows a lane group takes in turn: a workgroup covers 4 * (256 / L) rows
constexpr int kG16WaveRow = 32;      // rows longer than this: one wave (its 64 / L lane groups); up to it: one lane group
constexpr int kG16BlockRow = 256;    // rows longer than this: the whole workgroup
constexpr int kG16Unroll = 4;        // entries per lane group per step
constexpr int kG16MinWavesDst = 4, kG16MinWavesSrc = 5;  // waves per SIMD: the fp32 unit's occupancy (dst also carries the g * l sums)
constexpr int kG16MaxBlocks = 4096;  // workgroups of a row launch (gatv2_attention.hip's cap): beyond, tiles b, b + 4096, ...

// sum over the wave's 64 / L lane groups, the same bits in all of them
template <int L, int VEC>
__device__ __forceinline__ typename AccT<VEC>::type wave_fold16(typename AccT<VEC>::type v) {
#pragma unroll
  for (int off = L; off < 64; off <<= 1)
#pragma unroll
    for (int q = 0; q < VEC; ++q) aset(v, q, aget(v, q) + __shfl_xor(aget(v, q), off, 64));
  return v;
}

// sum over the lane groups of a workgroup, valid in wave 0 / group 0: the wave fold, then the wave partials in wave order through LDS
template <int L, int VEC>
__device__ __forceinline__ typename AccT<VEC>::type block_fold16(typename AccT<VEC>::type v, float (*red)[L * VEC], int wid, int g,
                                                                 int sub) {
  v = wave_fold16<L, VEC>(v);
  __syncthreads();  // (red[] of the previous fold has been read)
  if (g == 0) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) red[wid][sub * VEC + q] = aget(v, q);
  }
  __syncthreads();
  if (wid == 0 && g == 0) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      float w = red[0][sub * VEC + q];
#pragma unroll
      for (int k = 1; k < kG16Waves; ++k) w += red[k][sub * VEC + q];
      aset(v, q, w);
    }
  }
  return v;
}

// rows of a workgroup's tile at L lanes per row
constexpr int grad16_tile_rows(int L) { return kG16Waves * (64 / L) * kG16RowsPerGroup; }

// SIDE 0: grad_H_dst (own = H_dst[r], gathered = H_src[col], g[e]) and the att partials; SIDE 1: grad_H_src (own = H_src[c],
// gathered = H_dst[col_t], g[perm[e]], over the rows of A^T).  L * VEC >= a.D: one column pass.
template <typename E, int SIDE, int L, int VEC>
__global__ __launch_bounds__(kG16Threads, SIDE == 0 ? kG16MinWavesDst : kG16MinWavesSrc) void gatv2_grad16_kernel(Gatv2Args16 a) {
  typedef typename E::T T;
  typedef Lane<E, VEC> LN;
  typedef typename LN::raw_t raw_t;
  typedef typename LN::acc_t acc_t;
  constexpr int G = 64 / L, NG = kG16Waves * G, R = grad16_tile_rows(L);
  constexpr int kMaskIters = (R + kG16Threads - 1) / kG16Threads;
  __shared__ unsigned long long longmask[kMaskIters * kG16Waves], midmask[kMaskIters * kG16Waves];
  __shared__ float red[kG16Waves][L * VEC];
  __shared__ __attribute__((aligned(32))) float att_s[L * VEC];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane / L, sub = lane % L, gid = wid * G + g;
  const int N = SIDE == 0 ? a.N : a.n_t, D = a.D, Dh = a.D / a.heads;
  const float slope = a.slope;
  const T* __restrict__ own = reinterpret_cast<const T*>(SIDE == 0 ? a.H_dst : a.H_src);
  const T* __restrict__ oth = reinterpret_cast<const T*>(SIDE == 0 ? a.H_src : a.H_dst);
  const size_t ld_own = SIDE == 0 ? a.ld_dst : a.ld_src, ld_oth = SIDE == 0 ? a.ld_src : a.ld_dst;
  void* __restrict__ out = SIDE == 0 ? a.grad_dst : a.grad_src;
  const size_t ld_out = SIDE == 0 ? a.ld_gdst : a.ld_gsrc;
  const bool out16 = a.grad16 != 0;
  const int* __restrict__ rowptr = SIDE == 0 ? a.rowptr : a.rowptr_t;
  const int* __restrict__ colp = SIDE == 0 ? a.col : a.col_t;
  const int n_tiles = (N + R - 1) / R;
  const int c = sub * VEC;  // (D % VEC == 0: no lane is moved back)
  const bool live = c < D;
  const int cs = live ? c : 0;
  // att is read once per row, at the store: it waits in LDS, not in VEC registers that would be live across every walk
  if (gid == 0 && live) *reinterpret_cast<acc_t*>(att_s + c) = LN::load_partial(a.att + c);
  __syncthreads();
  const float* __restrict__ gh = a.g + (long long)(cs / Dh) * a.E;  // (VEC divides Dh: a lane's columns lie in one head)
  acc_t gl = azero<VEC>();  // SIDE 0: this lane's sum of g * l
  // acc += entries first, first + stride, ... < n of the row that starts at b
  auto walk = [&](const raw_t& mine, long long b, int n, int first, int stride, acc_t& acc) {
    int cc[kG16Unroll];
    int ge[kG16Unroll];  // (E < 2^31: capi.hip)
    auto indices = [&](int i) {  // column ids and g positions of the step that starts at entry i
#pragma unroll
      for (int u = 0; u < kG16Unroll; ++u) {
        const int iu = i + u * stride;
        cc[u] = -1;
        ge[u] = 0;
        if (iu < n) {
          cc[u] = colp[b + iu];
          ge[u] = SIDE == 0 ? (int)(b + iu) : a.perm[b + iu];
        }
      }
    };
    indices(first);
    for (int i = first; i < n; i += stride * kG16Unroll) {
      raw_t ov[kG16Unroll];
      float gv[kG16Unroll];
      bool on[kG16Unroll];
#pragma unroll
      for (int u = 0; u < kG16Unroll; ++u) {  // the gathers, all in flight before any arithmetic
        ov[u] = LN::zero();
        gv[u] = 0.f;
        on[u] = cc[u] >= 0;
        if (on[u]) {
          ov[u] = LN::load(oth + (size_t)cc[u] * ld_oth + c);
          gv[u] = gh[ge[u]];
        }
      }
      indices(i + stride * kG16Unroll);  // the next step's indices travel while this step's rows arrive
#pragma unroll
      for (int u = 0; u < kG16Unroll; ++u) {
        if (!on[u]) continue;
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float z = v216_z(LN::elem(mine, q), LN::elem(ov[u], q));
          aset(acc, q, fmaf(gv[u], z > 0.f ? 1.f : slope, aget(acc, q)));
          if constexpr (SIDE == 0) aset(gl, q, fmaf(gv[u], v216_leaky(z, slope), aget(gl, q)));
        }
      }
    }
  };
  auto store_row = [&](int r, const acc_t& acc) {  // att * acc in fp32; fp32, or one rounding to the operands' type
    const acc_t att = *reinterpret_cast<const acc_t*>(att_s + c);
    acc_t o;
#pragma unroll
    for (int q = 0; q < VEC; ++q) aset(o, q, aget(att, q) * aget(acc, q));
    if (out16) LN::store(reinterpret_cast<T*>(out) + (size_t)r * ld_out + c, o);
    else LN::store_partial(reinterpret_cast<float*>(out) + (size_t)r * ld_out + c, o);
  };
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // tiles of R rows in turn: a fixed assignment
    const int r0 = tile * R;
    // the tile's wave rows and workgroup rows as bit masks in row order (lists filled by arrival would let timing into the att sums)
#pragma unroll
    for (int k = 0; k < kMaskIters; ++k) {
      const int i = k * kG16Threads + tid;
      int n = 0;
      if (i < R && r0 + i < N) n = rowptr[r0 + i + 1] - rowptr[r0 + i];
      const unsigned long long ml = __ballot(n > kG16BlockRow), mm = __ballot(n > kG16WaveRow && n <= kG16BlockRow);
      if (lane == 0) {
        longmask[k * kG16Waves + wid] = ml;
        midmask[k * kG16Waves + wid] = G > 1 ? mm : 0ull;  // (L = 64: a wave is one lane group)
      }
    }
    __syncthreads();
    // rows of up to kG16WaveRow entries: one lane group each
    for (int k = 0; k < kG16RowsPerGroup; ++k) {
      const int r = r0 + k * NG + gid;
      if (r >= N) break;
      const long long b = rowptr[r];
      const int n = rowptr[r + 1] - (int)b;
      if (n > (G > 1 ? kG16WaveRow : kG16BlockRow)) continue;
      acc_t acc = azero<VEC>();
      if (n > 0 && live) {
        const raw_t mine = LN::load(own + (size_t)r * ld_own + c);
        walk(mine, b, n, 0, 1, acc);
      }
      if (live) store_row(r, acc);
    }
    // rows of up to kG16BlockRow entries: the k-th of them in row order by wave k mod 4, entry i by its lane group i mod G
    if constexpr (G > 1) {
      int turn = 0;
      for (int w = 0; w < kMaskIters * kG16Waves; ++w) {
        unsigned long long m = midmask[w];
        while (m) {
          const int r = r0 + w * 64 + (__ffsll((long long)m) - 1);
          m &= m - 1;
          if (turn++ % kG16Waves != wid) continue;
          const long long b = rowptr[r];
          const int n = rowptr[r + 1] - (int)b;
          acc_t acc = azero<VEC>();
          if (live) {
            const raw_t mine = LN::load(own + (size_t)r * ld_own + c);
            walk(mine, b, n, g, G, acc);
          }
          acc = wave_fold16<L, VEC>(acc);
          if (g == 0 && live) store_row(r, acc);
        }
      }
    }
    // longer rows: the whole workgroup, in row order
    for (int w = 0; w < kMaskIters * kG16Waves; ++w) {
      unsigned long long m = longmask[w];
      while (m) {
        const int r = r0 + w * 64 + (__ffsll((long long)m) - 1);
        m &= m - 1;
        const long long b = rowptr[r];
        const int n = rowptr[r + 1] - (int)b;
        acc_t acc = azero<VEC>();
        if (live) {
          const raw_t mine = LN::load(own + (size_t)r * ld_own + c);
          walk(mine, b, n, gid, NG, acc);
        }
        acc = block_fold16<L, VEC>(acc, red, wid, g, sub);
        if (wid == 0 && g == 0 && live) store_row(r, acc);
      }
    }
    __syncthreads();  // (longmask has been read by every thread)
  }
  if constexpr (SIDE == 0) {  // this workgroup's [D] partial of grad_att
    gl = block_fold16<L, VEC>(gl, red, wid, g, sub);
    if (wid == 0 && g == 0 && live)
      *reinterpret_cast<typename MemF32<VEC>::type*>(a.partial + (size_t)blockIdx.x * D + c) = gl;
  }
}

// grad_att[j] = sum of the workgroups' partials in index order: 16 interleaved series per column, then those in order
constexpr int kFold16Cols = 16, kFold16Parts = 16;
__global__ __launch_bounds__(kFold16Cols* kFold16Parts) void gatv2_att16_fold_kernel(const float* __restrict__ partial, int n_blocks,
                                                                                    int D, float* __restrict__ grad_att) {
  __shared__ float red[kFold16Parts][kFold16Cols];
  const int cj = threadIdx.x % kFold16Cols, part = threadIdx.x / kFold16Cols, j = blockIdx.x * kFold16Cols + cj;
  float s = 0.f;
  if (j < D)
    for (int b = part; b < n_blocks; b += kFold16Parts) s += partial[(size_t)b * D + j];
  red[part][cj] = s;
  __syncthreads();
  if (part == 0 && j < D) {
    float w = red[0][cj];
#pragma unroll
    for (int k = 1; k < kFold16Parts; ++k) w += red[k][cj];
    grad_att[j] = w;
  }
}

// workgroups of a row launch over n rows at L lanes per row: never more than gatv2_grad_blocks(n, D), whose tiles hold fewer rows
inline long long grad16_blocks(long long n, int L) {
  const long long tiles = (n + grad16_tile_rows(L) - 1) / grad16_tile_rows(L);
  return tiles < kG16MaxBlocks ? tiles : kG16MaxBlocks;
}

template <typename E, int L, int VEC>
hipError_t launch_grad16_LV(const Gatv2Args16& a, hipStream_t stream) {
  if (a.N > 0) {
    hipLaunchKernelGGL((gatv2_grad16_kernel<E, 0, L, VEC>), dim3((unsigned)grad16_blocks(a.N, L)), dim3(kG16Threads), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.n_t > 0) {
    hipLaunchKernelGGL((gatv2_grad16_kernel<E, 1, L, VEC>), dim3((unsigned)grad16_blocks(a.n_t, L)), dim3(kG16Threads), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(gatv2_att16_fold_kernel, dim3((unsigned)((a.D + kFold16Cols - 1) / kFold16Cols)),
                     dim3(kFold16Cols * kFold16Parts), 0, stream, a.partial, (int)grad16_blocks(a.N, L), a.D, a.grad_att);
  return hipGetLastError();
}

template <typename E, int VEC, bool BWD> hipError_t gatv2_16_L(const Gatv2Args16& a, int dh, hipStream_t stream) {
#define HCSPMM_V216_CASE(LANES)                                                    \
  case LANES:                                                                     \
    if constexpr (BWD) return launch_grad16_LV<E, LANES, VEC>(a, stream);         \
    else return launch_scores16_LV<E, LANES, VEC>(a, dh, stream);
  switch (sddmm_L(a.D, VEC)) {
    HCSPMM_V216_CASE(1)
    HCSPMM_V216_CASE(2)
    HCSPMM_V216_CASE(4)
    HCSPMM_V216_CASE(8)
    HCSPMM_V216_CASE(16)
    HCSPMM_V216_CASE(32)
    default:
      if constexpr (BWD) return launch_grad16_LV<E, 64, VEC>(a, stream);
      else return launch_scores16_LV<E, 64, VEC>(a, dh, stream);
  }
#undef HCSPMM_V216_CASE
}

template <bool BWD> hipError_t gatv2_16_dispatch(const Gatv2Args16& a, int dtype, hipStream_t stream) {
  if (!gatv2_16_supported(a.D, a.heads)) return hipErrorInvalidValue;
  const int dh = a.D / a.heads;
  const bool v8 = dh % 8 == 0;
  if (dtype == HCSPMM_DTYPE_F16) return v8 ? gatv2_16_L<F16, 8, BWD>(a, dh, stream) : gatv2_16_L<F16, 4, BWD>(a, dh, stream);
  if (dtype == HCSPMM_DTYPE_BF16) return v8 ? gatv2_16_L<BF16, 8, BWD>(a, dh, stream) : gatv2_16_L<BF16, 4, BWD>(a, dh, stream);
  return hipErrorInvalidValue;
}

}  // namespace

// one lane group per row: Dh % 4 == 0 and D within 64 lanes of 8 (Dh % 8 == 0) or 4 columns, sddmm_heads16's range
bool gatv2_16_supported(int D, int heads) { return sddmm_heads16_supported(D, heads); }

hipError_t launch_gatv2_scores16(const Gatv2Args16& a, int dtype, hipStream_t stream) {
  if (a.N == 0 || a.E == 0) return gatv2_16_supported(a.D, a.heads) ? hipSuccess : hipErrorInvalidValue;
  return gatv2_16_dispatch<false>(a, dtype, stream);
}

// E = 0 takes the same launches: every row is empty, so all three gradients come out as zeros
hipError_t launch_gatv2_backward16(const Gatv2Args16& a, int dtype, hipStream_t stream) {
  return gatv2_16_dispatch<true>(a, dtype, stream);
}

}  // namespace hcspmm
