// capi.hip -- C-ABI entry points that enqueue device work (see include/hcspmm.h).
//
// hcspmm_forward replaces the reference launchers spmm_forward_plus / _more / _fixed32 / _fixed64
// (hybrid_kernel/hybrid_all_kernel.cu:410-594) and hcspmm_forward_fused the five fused launchers
// (:596-863).  Differences by design: work goes to the caller's stream (the reference uses the
// legacy default stream), every launch is checked (the reference checks none, :283-287), Z is the
// caller's buffer, and nothing synchronises or allocates.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "fingerprint.h"
#include "graph_build.h"
#include "hcspmm.h"
#include "spmm_kernels.h"

namespace {
thread_local int g_last_hip_error = 0;

int fail_hip(hipError_t e) {
  g_last_hip_error = (int)e;
  return HCSPMM_EHIP;
}

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// 8-bit e4m3fn codes (hcspmm_forward_fp8): an element type of the launch decisions below only -- the typed entry points
// refuse it (their dtype range ends at BF16)
constexpr int kDtypeF8 = HCSPMM_DTYPE_BF16 + 1;

inline int elem_bytes(int dtype) { return dtype == HCSPMM_DTYPE_F32 ? 4 : dtype == kDtypeF8 ? 1 : 2; }

// Per-lane access width (in elements).  fp32: 16 bytes per lane for every embedding width of at least 4 columns, whatever
// the row strides and base addresses are -- the kernels address fp32 vectors with element alignment and move a lane whose
// columns would run past the row back onto the row's last four (spmm_impl.h MemF32 / lane_col) -- 8 bytes for D = 2, 3
// and single elements for D = 1.  16-bit features: below.
int pick_vec(int dtype, int D, int64_t ldx, int64_t ldz, const void* X, const void* Z, const void* ws) {
  // (8-byte lanes for fp32 widths up to 16 -- more lanes per row, eight loads in flight per lane -- were measured too: D = 16 is 10 %
  // SLOWER that way, D = 12 3 % faster, D = 4 ... 8 the same: not adopted)
  if (dtype == HCSPMM_DTYPE_F32) return D >= 4 ? 4 : D >= 2 ? 2 : 1;
  // 16-bit features: 8 (or, below 8 columns, 4) elements per lane whenever every row starts on a dword -- an even width, even row
  // strides, 4-byte aligned bases; the fp32 workspace is always that -- the last lane moved back onto the row's last elements;
  // single elements otherwise (odd widths or strides)
  const bool dword_rows = ((D | ldx | ldz) & 1) == 0 && aligned(X, 4) && aligned(Z, 4) && (!ws || aligned(ws, 4));
  // below 32 columns 8-byte lanes win: 5-8 lanes per row keep eight loads in flight per lane (L = 8), where three 16-byte lanes
  // (L = 4) keep four -- D = 20 / 22 / 24 are 7-10 % faster that way, D = 32 is not (profiles/r04/ab_ragged_lanes_bf16.log)
  if (dword_rows && D >= 32) return 8;
  if (dword_rows && D >= 4) return 4;
  return 1;
}

// the access width wide_choice assumes (from the embedding width alone, so that callers can ask ahead of a launch)
inline int nominal_vec(int dtype, int D) {
  if (dtype == HCSPMM_DTYPE_F32) return D >= 4 ? 4 : D >= 2 ? 2 : 1;
  // 8-bit codes: widths are multiples of 4 (hcspmm_forward_fp8 refuses the rest), 8 codes per lane from 32 columns up, as for the
  // 16-bit types (whose accumulator shape those builds share)
  if (dtype == kDtypeF8) return D >= 32 ? 8 : 4;
  return (D % 2 == 0 && D >= 32) ? 8 : (D % 2 == 0 && D >= 4) ? 4 : 1;
}
}  // namespace

extern "C" const char* hcspmm_strerror(int code) {
  switch (code) {
    case HCSPMM_OK: return "ok";
    case HCSPMM_EINVAL: return "invalid argument (null / negative size / column id out of range / X too short for the plan)";
    case HCSPMM_ENOMEM: return "host allocation failed";
    case HCSPMM_EPLAN: return "plan does not match this graph (magic/version/N/E/layout/fingerprint)";
    case HCSPMM_EHIP: return "HIP runtime error (see hcspmm_last_hip_error)";
    case HCSPMM_EWORKSPACE: return "workspace too small";
    case HCSPMM_ERANGE: return "size exceeds the int32 index contract";
    default: return "unknown hcspmm error";
  }
}

// Column-panel choice for the sparse region.  Wide embeddings are processed panel-major in slices of
// 32 fp32 columns (one 128-byte line per gathered row): with a quarter of every row in play at a
// time, four times as many distinct rows fit the per-XCD L2 -- measured at D = 32 the L2 hit rate is
// 51 % against 34 % at D = 128 on the same graph, and the launch is bound by what misses L2.  Each
// pass re-reads the column indices and pays the per-task overhead again, so short-row graphs
// (mean task length < 8) keep one pass over the full width.  HCSPMM_PANEL_COLS overrides
// (-1: one pass; n > 0: n columns, rounded up to a multiple of 16).
static int panel_choice(const hcspmm_plan_header* h, int D, int dtype) {
  static const int env = [] {
    const char* e = getenv("HCSPMM_PANEL_COLS");
    return e ? atoi(e) : 0;
  }();
  if (env < 0) return D;
  if (env > 0) return env >= D ? D : ((env + 15) / 16) * 16;
  if (h->panel_cols != 0) {  // the plan's own choice (hcspmm_plan_params.panel_cols; hcspmm.tune_plan measures it)
    const long long cols = h->panel_cols < 0 ? D : (long long)h->panel_cols * (4 / elem_bytes(dtype));
    return cols >= D ? D : (int)cols;
  }
  const int line_cols = 128 / elem_bytes(dtype);  // 32 fp32, 64 16-bit or 128 8-bit columns: one cache line per gathered row
  if (D < 2 * line_cols || h->n_tasks <= 0) return D;
  const double mean_len = (double)h->nnz_sparse / ((double)h->n_tasks + (double)h->n_slice_tasks);
  if (mean_len < 8.0) return D;
  // an X beyond the 256 MiB Infinity Cache is gathered from HBM whatever the order: two lines per row and pass (256
  // contiguous bytes per gather) measure 2-3 % faster there than one (config 4 / 5 shares, 16 M-node power law:
  // profiles/r03/ab_panel_width.log), while a cache-resident X wants exactly one (Reddit-scale: 64 columns +8 %, all 128 +20 %)
  const double x_bytes = (double)h->num_columns * (double)D * (double)elem_bytes(dtype);
  const int cols = x_bytes > 256.0 * 1048576.0 ? 2 * line_cols : line_cols;
  return D >= 2 * cols ? cols : D;
}

// Wide-task threshold.  A lane group sums a task with U loads in flight, so a task of T entries is a
// chain of T/U dependent memory round trips; the whole launch is about
// passes * nnz_sparse / (8 * R * resident waves) such rounds deep.  The threshold is the largest
// power of two in [16, 256] not exceeding a quarter of that depth times 8: small (latency-bound)
// launches hand every row longer than 16 entries to a whole wave, large (throughput-bound) ones
// keep rows up to 256 entries on one lane group, in CSR order.
static int wide_choice(const hcspmm_plan_header* h, int D, int dtype, int* n_wide, int* panel_cols = nullptr) {
  const int vec = nominal_vec(dtype, D);
  const int pw = panel_choice(h, D, dtype);
  if (panel_cols) *panel_cols = pw;
  const double passes = (double)((D + pw - 1) / pw);
  int L = 4;
  while (L < (pw + vec - 1) / vec && L < 64) L <<= 1;
  const int R = 64 / L;
  *n_wide = 0;
  const double work = passes * (double)h->nnz_sparse;
  if (R == 1) return INT32_MAX;
  const double kResidentWaves = 256.0 * 16.0;
  const double t = 0.25 * work / ((double)R * kResidentWaves);
  int b = 0;
  while (b < 4 && (double)(16 << (b + 1)) <= t) ++b;
  *n_wide = h->n_len_gt[b];
  return *n_wide > 0 ? (16 << b) : INT32_MAX;
}

extern "C" int32_t hcspmm_wide_threshold_typed(const hcspmm_plan_header* h, int D, int dtype) {
  if (D <= 0 || dtype < HCSPMM_DTYPE_F32 || dtype > HCSPMM_DTYPE_BF16) return INT32_MAX;
  if (!h) {  // plan-free kernel: fixed threshold (kPlanFreeWide in spmm_impl.h) unless a wave holds one lane group
    const int vec = nominal_vec(dtype, D);
    return (D + vec - 1) / vec > 32 ? INT32_MAX : 64;
  }
  int n_wide = 0;
  return wide_choice(h, D, dtype, &n_wide);
}

extern "C" int32_t hcspmm_wide_threshold_fp8(const hcspmm_plan_header* h, int D) {
  if (D <= 0 || D % 4 != 0) return INT32_MAX;
  if (!h) return (D + nominal_vec(kDtypeF8, D) - 1) / nominal_vec(kDtypeF8, D) > 32 ? INT32_MAX : 64;  // (as hcspmm_wide_threshold_typed)
  int n_wide = 0;
  return wide_choice(h, D, kDtypeF8, &n_wide);
}

extern "C" int32_t hcspmm_wide_threshold(const hcspmm_plan_header* h, int D) {
  return hcspmm_wide_threshold_typed(h, D, HCSPMM_DTYPE_F32);
}

extern "C" int32_t hcspmm_own_tiny_launch(const hcspmm_plan_header* h, int fused) {
  return h && hcspmm::plan_own_tiny_launch(h->n_tiny, fused) ? 1 : 0;
}

extern "C" int hcspmm_abi_version(void) { return HCSPMM_ABI_VERSION; }

// Device variant of hcspmm_graph_fingerprint_host: every thread adds the terms of its grid-stride share, a wave
// folds them with shuffles and issues one 64-bit atomic add (the sum is order-independent, so the result is exact).
namespace {
__global__ __launch_bounds__(256) void fingerprint_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          long long N, long long E, unsigned long long* out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long acc = (i0 == 0) ? hcspmm::fp_seed(N, E) : 0ull;
  for (long long r = i0; r <= N; r += stride) acc += hcspmm::fp_term_rowptr((uint64_t)r, rowptr[r]);
  for (long long e = i0; e < E; e += stride) acc += hcspmm::fp_term_col((uint64_t)e, col[e]);
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}
}  // namespace

namespace {
// edgeToRow[e] = largest r with rowptr[r] <= e (rows without entries never win: the search looks for the LAST such row)
__global__ __launch_bounds__(256) void edge_to_row_kernel(const int32_t* __restrict__ rowptr, int N, long long E,
                                                          int32_t* __restrict__ e2r) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
    int lo = 0, hi = N;  // invariant: rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if ((long long)rowptr[mid] <= e) lo = mid;
      else hi = mid;
    }
    e2r[e] = lo;
  }
}
}  // namespace

extern "C" int hcspmm_edge_to_row_device(const int32_t* rowptr, int64_t N, int64_t E, int32_t* e2r, void* stream_v) {
  if (N < 0 || E < 0 || !rowptr || (E > 0 && !e2r)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  if (E == 0) return HCSPMM_OK;
  long long blocks = (E + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(edge_to_row_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_v), rowptr,
                     (int)N, (long long)E, e2r);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

// Graphs built on the device (graph_build.h): the sampler's scan and selection, and the transpose
static_assert(HCSPMM_SAMPLE_WAVE_ROW_MAX == hcspmm::kSampleWaveRowMax, "hcspmm.h documents the sampler's wave-row limit");

extern "C" size_t hcspmm_sample_workspace_bytes(int64_t N) {
  return (N < 0 || N > INT32_MAX - 16) ? 0 : hcspmm::sample_workspace_bytes((long long)N);
}

extern "C" int hcspmm_sample_row_pointers_device(const int32_t* rowptr, int64_t N, int fanout, int32_t* rowptr_s, void* workspace,
                                                 size_t workspace_bytes, void* stream_v) {
  if (N < 0 || fanout < 1 || !rowptr || !rowptr_s) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16) return HCSPMM_ERANGE;
  if (!workspace || workspace_bytes < hcspmm::sample_workspace_bytes((long long)N)) return HCSPMM_EWORKSPACE;
  const hipError_t e = hcspmm::launch_sample_row_pointers(rowptr, (long long)N, fanout, rowptr_s, workspace,
                                                          reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

extern "C" int hcspmm_sample_neighbors_device(const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_s, int64_t N, int64_t E,
                                              int fanout, uint64_t seed, int32_t* col_s, int32_t* entry_s, void* stream_v) {
  if (N < 0 || E < 0 || fanout < 1 || !rowptr || !rowptr_s || (E > 0 && (!col || !col_s || !entry_s))) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  if (N == 0 || E == 0) return HCSPMM_OK;
  const hipError_t e = hcspmm::launch_sample_neighbors(rowptr, col, rowptr_s, (long long)N, fanout, seed, col_s, entry_s,
                                                       reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

extern "C" size_t hcspmm_transpose_graph_device_workspace_bytes(int64_t N, int64_t M, int64_t E) {
  if (N < 0 || M < 0 || E < 0 || M > INT32_MAX - 16 || E > INT32_MAX) return 0;
  return hcspmm::transpose_workspace_bytes((long long)M, (long long)E);
}

extern "C" int hcspmm_transpose_graph_device(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t M, int64_t E,
                                             int32_t* rowptr_t, int32_t* col_t, int32_t* entry_t, void* workspace,
                                             size_t workspace_bytes, void* stream_v) {
  if (N < 0 || M < 0 || E < 0 || !rowptr || !rowptr_t || (E > 0 && (!col || !col_t || !entry_t))) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || M > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  const size_t need = hcspmm::transpose_workspace_bytes((long long)M, (long long)E);
  if (need > 0 && (!workspace || workspace_bytes < need)) return HCSPMM_EWORKSPACE;
  const hipError_t e = hcspmm::launch_transpose_graph(rowptr, col, (long long)N, (long long)M, (long long)E, rowptr_t, col_t, entry_t,
                                                      workspace, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

extern "C" int hcspmm_graph_fingerprint_device(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t E,
                                               uint64_t* out_d, void* stream_v) {
  if (!rowptr || !out_d || N < 0 || E < 0 || (E > 0 && !col)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
  hipError_t e = hipMemsetAsync(out_d, 0, sizeof(uint64_t), stream);
  if (e != hipSuccess) return fail_hip(e);
  long long blocks = (N + 1 + E + 256 * 16 - 1) / (256 * 16);
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(fingerprint_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, rowptr, col, (long long)N, (long long)E,
                     reinterpret_cast<unsigned long long*>(out_d));
  e = hipGetLastError();
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}
extern "C" int hcspmm_last_hip_error(void) { return g_last_hip_error; }

namespace {
// weights / output of a fused launch (dense-tile windows multiply their tile by W inside the hybrid kernel)
struct FusedOperands {
  const float* W;
  long long ldr, ldc;
  float* out;
  int H;
  int mode;  // bit 0: dense-tile windows update inside the hybrid launch; bit 1: ordinary / tiny sparse rows in the row-tile launch
};

// the graph arguments every planned-or-plan-free entry point receives
struct GraphIn {
  const int32_t *rowptr, *col, *blockPartition, *edgeToColumn, *edgeToRow, *hybrid_type, *plan_d;
  const hcspmm_plan_header* ph;
  int64_t N, E;
};

// an entry point's graph parameters (every one names them alike)
#define GRAPH_IN GraphIn{rowptr, col, blockPartition, edgeToColumn, edgeToRow, hybrid_type, plan_d, ph, N, E}

constexpr int64_t kNoSource = INT64_MAX;  // bind_graph's src_rows of a launch that gathers no rows (the copy op)

// The one "plan or plan-free" binding, after the entry point's own size / null / range checks.
// Planned (plan_d and ph): hcspmm_plan_check, then src_rows against the rows the plan gathers (EINVAL), then the workspace against
// ws_mult partial-sum areas (EWORKSPACE); p gets the plan fields from the host copy of the header, the n_wide / panel_cols that
// wide_choice decides for element type `dtype`, partial (null when the plan has no split rows), col and N / D.  The launcher-owned
// fields stay zero: plan_layout.h fills them.
// Plan-free: one of plan_d / ph alone, or a missing window array, is EINVAL; p gets col and N / D, and p.plan stays null.
int bind_graph(hcspmm::PlanArgs& p, const GraphIn& g, int D, int64_t src_rows, void* workspace, size_t workspace_bytes, int ws_mult,
               int dtype) {
  p = hcspmm::PlanArgs{};
  p.col = g.col;
  p.N = (int)g.N;
  p.D = D;
  p.E = (int)g.E;
  const hcspmm_plan_header* ph = g.ph;
  if (!(g.plan_d && ph)) {
    if (g.plan_d || ph) return HCSPMM_EINVAL;  // both or neither
    if (!g.blockPartition || !g.hybrid_type || (g.E > 0 && (!g.edgeToColumn || !g.edgeToRow))) return HCSPMM_EINVAL;
    return HCSPMM_OK;
  }
  const int rc = hcspmm_plan_check(ph, g.N, g.E, 0);
  if (rc != HCSPMM_OK) return rc;
  if (src_rows < ph->num_columns) return HCSPMM_EINVAL;  // the plan gathers rows the source does not have
  const size_t need = (size_t)ws_mult * hcspmm_workspace_bytes(ph, D);
  if (need > 0 && (!workspace || workspace_bytes < need)) return HCSPMM_EWORKSPACE;
  p.partial = need ? reinterpret_cast<float*>(workspace) : nullptr;
  p.plan = g.plan_d;
  p.off_tasks = ph->off_tasks;
  p.off_sched = ph->off_tasks;  // (use_schedule moves the binary product onto the exact-length copies)
  p.n_tasks = ph->n_tasks;
  p.n_tiny = ph->n_tiny;
  p.off_slice_table = ph->off_slice_table;
  p.off_slice_tasks = ph->off_slice_tasks;
  p.n_slices = ph->n_slices;
  p.slice_xcd_tasks = ph->slice_xcd_tasks;
  p.off_dense_index = ph->off_dense_index;
  p.off_dense_pack = ph->off_dense_pack;
  p.n_dense = ph->n_dense;
  p.off_dense_compact = ph->off_dense_compact;
  p.n_dense_compact = ph->n_dense_compact;
  p.off_dense_compact2 = ph->off_dense_compact2;
  p.n_dense_compact2 = ph->n_dense_compact2;
  p.off_fixups = ph->off_fixups;
  p.n_split_rows = ph->n_split_rows;
  wide_choice(ph, D, dtype, &p.n_wide, &p.panel_cols);
  return HCSPMM_OK;
}

// The binary product (launches of spmm_impl.h) reads its wide, ordinary and sliced descriptors from the plan's schedule copies
// where the plan has them (hcspmm.h off_task_sched): the same tasks, each summed by the same lanes in the same order, with the
// lane groups of a wave ending together.  The tiny tasks, the fix-up pass and every other launch keep the lists as they are.
inline void use_schedule(hcspmm::PlanArgs& p, const hcspmm_plan_header* ph) {
  if (ph->off_task_sched != 0) p.off_sched = ph->off_task_sched;
  if (ph->off_slice_sched != 0) p.off_slice_tasks = ph->off_slice_sched;
  // ... and the first indices of those descriptors from the records that belong to the copies (hcspmm.h off_task_sched_idx),
  // the sliced region's list bounds from the header's copy of the slice table.  A plan without the records leaves all of it
  // zero: the kernel then reads col behind the descriptor and the table from the plan, as before.
  if (ph->off_task_sched != 0 && ph->off_task_sched_idx != 0) p.off_sched_idx = ph->off_task_sched_idx;
  if (ph->off_slice_sched != 0 && ph->off_slice_sched_idx != 0) {
    p.off_slice_idx = ph->off_slice_sched_idx;
    if (ph->n_slices == 8) {
      p.slice_tbl_n = 9;
      for (int s = 0; s < 9; ++s) p.slice_tbl[s] = ph->slice_table_copy[s];
    }
  }
}

inline void set_operands(hcspmm::PlanArgs& p, const void* X, void* Z, int64_t ldx, int64_t ldz) {
  p.X = X;
  p.Z = Z;
  p.ldx = (size_t)ldx;
  p.ldz = (size_t)ldz;
}

// the plan-free launch's arguments, from a PlanArgs that bind_graph left plan-free and set_operands filled
inline hcspmm::WindowArgs window_args(const GraphIn& g, const hcspmm::PlanArgs& p) {
  return hcspmm::WindowArgs{p.X, p.Z, g.rowptr, g.col, g.blockPartition, g.edgeToColumn, g.edgeToRow, g.hybrid_type, p.ldx, p.ldz,
                            p.N, p.D};
}

// one launcher family's builds for the three typed element types
template <class A>
using Launcher = hipError_t (*)(const A&, int, hipStream_t);
template <class A>
hipError_t launch_typed(int dtype, Launcher<A> f32, Launcher<A> f16, Launcher<A> bf16, const A& a, int vec, hipStream_t stream) {
  return (dtype == HCSPMM_DTYPE_F32 ? f32 : dtype == HCSPMM_DTYPE_F16 ? f16 : bf16)(a, vec, stream);
}

int forward_impl(const void* X, int64_t x_rows, int64_t ldx, void* Z, int64_t ldz, int dtype, const GraphIn& g, int D,
                 void* workspace, size_t workspace_bytes, void* stream_v, const FusedOperands* fused, const float* values = nullptr,
                 int heads = 0, const int32_t* vindex = nullptr, int64_t num_values = 0) {
  using namespace hcspmm;
  if (dtype < HCSPMM_DTYPE_F32 || dtype > HCSPMM_DTYPE_BF16) return HCSPMM_EINVAL;
  if (g.N < 0 || g.E < 0 || D <= 0 || ldx < D || ldz < D) return HCSPMM_EINVAL;
  // heads > 0: the multi-head weighted product (fp32, Dh = D / heads columns per head, Dh % 4 == 0)
  // vindex: the indexed form (entry e weighs values[h * num_values + vindex[e]]); one head then takes any D
  if (heads > 0 && (dtype != HCSPMM_DTYPE_F32 || !values || fused || D % heads != 0 ||
                    ((D / heads) % 4 != 0 && !(vindex && heads == 1))))
    return HCSPMM_EINVAL;
  if (g.N == 0) return HCSPMM_OK;
  if (!X || !Z || !g.rowptr || (g.E > 0 && !g.col)) return HCSPMM_EINVAL;
  if (g.N > INT32_MAX - 16 || g.E > INT32_MAX) return HCSPMM_ERANGE;
  if (fused && !(g.plan_d && g.ph)) return HCSPMM_EINVAL;  // the fused forms are planned launches
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
  PlanArgs a;
  const int rc = bind_graph(a, g, D, x_rows, workspace, workspace_bytes, 1, dtype);
  if (rc != HCSPMM_OK) return rc;
  set_operands(a, X, Z, ldx, ldz);
  const int vec = pick_vec(dtype, D, ldx, ldz, X, Z, a.partial);
  hipError_t e;
  if (a.plan) {
    if (fused) {
      a.fused = fused->mode;
      a.H = fused->H;
      a.W = fused->W;
      a.w_ldr = fused->ldr;
      a.w_ldc = fused->ldc;
      a.out = fused->out;
    }
    if (fused && (vec != 4 || dtype != HCSPMM_DTYPE_F32)) return HCSPMM_EINVAL;  // (fused_form said otherwise)
    if (fused && (fused->mode & 2)) {
      // row-tile form: the ordinary / tiny tasks and the dense windows are summed AND multiplied by the tile launches
      // (fused_rows.hip); the hybrid launch below then runs the sliced and wide tasks only and ends with the fix-up pass,
      // which also adds the segments of split rows that sit among the ordinary tasks
      e = launch_fused_tiles(a, stream);
      if (e != hipSuccess) return fail_hip(e);
    }
    if (values) {
      if (fused) return HCSPMM_EINVAL;
      const WPlanArgs wa{a, values, g.rowptr, g.ph->segment_len};
      if (vindex) e = launch_plan_wi_f32(WHPlanArgs{wa, (long long)num_values, D / heads, vindex}, vec, stream);
      else if (heads > 0) e = launch_plan_wh_f32(WHPlanArgs{wa, (long long)g.E, D / heads, nullptr}, vec, stream);
      else e = launch_typed(dtype, launch_plan_w_f32, launch_plan_w_f16, launch_plan_w_bf16, wa, vec, stream);
    } else {
      if (!fused) use_schedule(a, g.ph);
      e = launch_typed(dtype, launch_plan_f32, launch_plan_f16, launch_plan_bf16, a, vec, stream);
    }
  } else {
    const WindowArgs w = window_args(g, a);
    if (values) {
      const WWindowArgs wa{w, values};
      if (vindex) e = launch_window_wi_f32(WHWindowArgs{wa, (long long)num_values, D / heads, vindex}, vec, stream);
      else if (heads > 0) e = launch_window_wh_f32(WHWindowArgs{wa, (long long)g.E, D / heads, nullptr}, vec, stream);
      else e = launch_typed(dtype, launch_window_w_f32, launch_window_w_f16, launch_window_w_bf16, wa, vec, stream);
    } else {
      e = launch_typed(dtype, launch_window_f32, launch_window_f16, launch_window_bf16, w, vec, stream);
    }
  }
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}
}  // namespace

extern "C" int hcspmm_forward_typed(const void* X, int64_t x_rows, int64_t ldx, void* Z, int64_t ldz, int dtype, const int32_t* rowptr,
                                    const int32_t* col, const int32_t* blockPartition, const int32_t* edgeToColumn,
                                    const int32_t* edgeToRow, const int32_t* hybrid_type, const int32_t* plan_d,
                                    const hcspmm_plan_header* ph, int64_t N, int64_t E, int D, void* workspace,
                                    size_t workspace_bytes, void* stream_v) {
  return forward_impl(X, x_rows, ldx, Z, ldz, dtype, GRAPH_IN, D, workspace, workspace_bytes, stream_v, nullptr);
}

// Edge-weighted product (spmm_weighted*.hip): the plan and launch decisions of hcspmm_forward_typed, values read on every call.
extern "C" int hcspmm_forward_weighted(const void* X, int64_t x_rows, int64_t ldx, void* Z, int64_t ldz, int dtype,
                                       const int32_t* rowptr, const int32_t* col, const int32_t* blockPartition,
                                       const int32_t* edgeToColumn, const int32_t* edgeToRow, const int32_t* hybrid_type,
                                       const int32_t* plan_d, const hcspmm_plan_header* ph, int64_t N, int64_t E, int D,
                                       void* workspace, size_t workspace_bytes, void* stream_v, const float* values) {
  if (!values) return HCSPMM_EINVAL;  // never a silent binary product
  return forward_impl(X, x_rows, ldx, Z, ldz, dtype, GRAPH_IN, D, workspace, workspace_bytes, stream_v, nullptr, values);
}

// Multi-head edge-weighted product (spmm_weighted_heads.hip): hcspmm_forward_weighted's checks and launch decisions, values
// [heads][E], fp32 only.
extern "C" int hcspmm_forward_weighted_heads(const void* X, int64_t x_rows, int64_t ldx, void* Z, int64_t ldz, int dtype,
                                             const int32_t* rowptr, const int32_t* col, const int32_t* blockPartition,
                                             const int32_t* edgeToColumn, const int32_t* edgeToRow, const int32_t* hybrid_type,
                                             const int32_t* plan_d, const hcspmm_plan_header* ph, int64_t N, int64_t E, int D,
                                             void* workspace, size_t workspace_bytes, void* stream_v, const float* values,
                                             int heads) {
  if (!values || heads <= 0) return HCSPMM_EINVAL;
  if ((long long)E * heads > INT64_MAX / 4) return HCSPMM_ERANGE;
  return forward_impl(X, x_rows, ldx, Z, ldz, dtype, GRAPH_IN, D, workspace, workspace_bytes, stream_v, nullptr, values, heads);
}

// Multi-head edge-weighted product with indexed values (spmm_weighted_indexed.hip): hcspmm_forward_weighted_heads's checks and
// launch decisions, entry e of head h weighing values[h * num_values + value_index[e]].
extern "C" int hcspmm_forward_weighted_indexed(const void* X, int64_t x_rows, int64_t ldx, void* Z, int64_t ldz, int dtype,
                                               const int32_t* rowptr, const int32_t* col, const int32_t* blockPartition,
                                               const int32_t* edgeToColumn, const int32_t* edgeToRow, const int32_t* hybrid_type,
                                               const int32_t* plan_d, const hcspmm_plan_header* ph, int64_t N, int64_t E, int D,
                                               void* workspace, size_t workspace_bytes, void* stream_v, const float* values,
                                               int heads, const int32_t* value_index, int64_t num_values) {
  if (!values || heads <= 0 || num_values < 0 || (E > 0 && (!value_index || num_values == 0))) return HCSPMM_EINVAL;
  if (num_values > INT32_MAX || num_values > INT64_MAX / 4 / heads) return HCSPMM_ERANGE;
  static const int32_t no_entries = 0;  // E = 0: nothing is read through the index, which may be NULL
  return forward_impl(X, x_rows, ldx, Z, ldz, dtype, GRAPH_IN, D, workspace, workspace_bytes, stream_v, nullptr, values, heads,
                      value_index ? value_index : &no_entries, num_values);
}

// 8-bit feature storage (quantize_fp8.hip, spmm_kernels_f8.hip, spmm_weighted_f8.hip): forward_impl's checks and launch
// decisions for one-byte elements, fp32 Z, nullable values and per-row scales.
extern "C" int hcspmm_quantize_fp8(const float* X, int64_t rows, int64_t ldx, int D, int format, const float* scale_in, void* Xq,
                                   int64_t ldq, float* scale_out, void* stream_v) {
  if (format != HCSPMM_FP8_E4M3) return HCSPMM_EINVAL;
  if (rows < 0 || D <= 0 || D % 4 != 0 || ldx < D || ldq < D || ldq % 4 != 0) return HCSPMM_EINVAL;
  if (rows == 0) return HCSPMM_OK;
  if (!X || !Xq || (!scale_out && !scale_in) || !aligned(Xq, 4)) return HCSPMM_EINVAL;
  const hipError_t e = hcspmm::launch_quantize_fp8(X, (long long)rows, (long long)ldx, D, scale_in, reinterpret_cast<unsigned char*>(Xq),
                                                   (long long)ldq, scale_out, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

extern "C" int hcspmm_forward_fp8(const void* Xq, int64_t x_rows, int64_t ldx, int format, const float* row_scale,
                                  const float* values, float* Z, int64_t ldz, const int32_t* rowptr, const int32_t* col,
                                  const int32_t* blockPartition, const int32_t* edgeToColumn, const int32_t* edgeToRow,
                                  const int32_t* hybrid_type, const int32_t* plan_d, const hcspmm_plan_header* ph, int64_t N,
                                  int64_t E, int D, void* workspace, size_t workspace_bytes, void* stream_v) {
  if (format != HCSPMM_FP8_E4M3) return HCSPMM_EINVAL;
  if (N < 0 || E < 0 || x_rows < 0 || D <= 0 || ldx < D || ldz < D) return HCSPMM_EINVAL;
  if (D % 4 != 0 || ldx % 4 != 0) return HCSPMM_EINVAL;  // rows of codes start on dwords
  if (N == 0) return HCSPMM_OK;
  if (!Xq || !Z || !rowptr || (E > 0 && !col) || !aligned(Xq, 4) || !aligned(Z, 4)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
  const int vec = nominal_vec(kDtypeF8, D);
  const bool binary = !values && !row_scale;
  const GraphIn g = GRAPH_IN;
  hcspmm::PlanArgs a;
  const int rc = bind_graph(a, g, D, x_rows, workspace, workspace_bytes, 1, kDtypeF8);
  if (rc != HCSPMM_OK) return rc;
  if (a.partial && !aligned(a.partial, 4)) return HCSPMM_EINVAL;
  set_operands(a, Xq, Z, ldx, ldz);
  hipError_t e;
  if (a.plan) {
    if (binary) {
      use_schedule(a, ph);
      e = hcspmm::launch_plan_f8(a, vec, stream);
    } else {
      a.row_scale = row_scale;
      e = hcspmm::launch_plan_w_f8(hcspmm::WPlanArgs{a, values, rowptr, ph->segment_len}, vec, stream);
    }
  } else {
    const hcspmm::WindowArgs w = window_args(g, a);
    e = binary ? hcspmm::launch_window_f8(w, vec, stream) : hcspmm::launch_window_w_f8(hcspmm::WWindowArgs{w, values, row_scale}, vec, stream);
  }
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

namespace {
// backward = false: hcspmm_forward_extremum (src = X, dst = Z); true: its backward (src = grad_Z, dst = grad_X, square)
int extremum_impl(bool backward, const float* src, int64_t src_rows, int64_t lds, float* dst, int64_t ldd, int dtype, const GraphIn& g,
                  int D, void* workspace, size_t workspace_bytes, void* stream_v, int reduce, int32_t* arg_out, const int32_t* arg_in,
                  int64_t ldarg, const int32_t* perm) {
  if (dtype != HCSPMM_DTYPE_F32 || (reduce != HCSPMM_REDUCE_MAX && reduce != HCSPMM_REDUCE_MIN)) return HCSPMM_EINVAL;
  if (g.N < 0 || g.E < 0 || D <= 0 || lds < D || ldd < D) return HCSPMM_EINVAL;
  if ((backward || arg_out) && ldarg < D) return HCSPMM_EINVAL;
  if (g.N == 0) return HCSPMM_OK;
  if (!src || !dst || !g.rowptr || (g.E > 0 && !g.col)) return HCSPMM_EINVAL;
  if (backward && (!arg_in || (g.E > 0 && !perm))) return HCSPMM_EINVAL;
  if (g.N > INT32_MAX - 16 || g.E > INT32_MAX) return HCSPMM_ERANGE;
  hcspmm::XArgs x{};
  // workspace: the fp32 values of the split rows' partial slots; forward: their positions in a second area behind them
  const int rc = bind_graph(x.p, g, D, src_rows, workspace, workspace_bytes, backward ? 1 : 2, HCSPMM_DTYPE_F32);
  if (rc != HCSPMM_OK) return rc;
  if (x.p.plan) {
    x.ppos = (x.p.partial && !backward) ? reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + hcspmm_workspace_bytes(g.ph, D))
                                        : nullptr;
    x.segment_len = g.ph->segment_len;
  }
  set_operands(x.p, src, dst, lds, ldd);
  x.rowptr = g.rowptr;
  x.flip = reduce == HCSPMM_REDUCE_MIN ? 0x80000000u : 0u;
  x.arg = arg_out;
  x.garg = arg_in;
  x.perm = perm;
  x.ldarg = (size_t)ldarg;
  const int vec = pick_vec(HCSPMM_DTYPE_F32, D, lds, ldd, src, dst, nullptr);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
  const hipError_t e = backward ? hcspmm::launch_extremum_backward_f32(x, vec, stream) : hcspmm::launch_extremum_f32(x, vec, stream);
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}
}  // namespace

extern "C" size_t hcspmm_extremum_workspace_bytes(const hcspmm_plan_header* ph, int D) {
  return 2 * hcspmm_workspace_bytes(ph, D);
}

// Max / min aggregation (spmm_extremum.hip): the plan and checks of hcspmm_forward_weighted, fp32 only.
extern "C" int hcspmm_forward_extremum(const void* X, int64_t x_rows, int64_t ldx, void* Z, int64_t ldz, int dtype,
                                       const int32_t* rowptr, const int32_t* col, const int32_t* blockPartition,
                                       const int32_t* edgeToColumn, const int32_t* edgeToRow, const int32_t* hybrid_type,
                                       const int32_t* plan_d, const hcspmm_plan_header* ph, int64_t N, int64_t E, int D,
                                       void* workspace, size_t workspace_bytes, void* stream_v, int reduce, int32_t* arg_out,
                                       int64_t ldarg) {
  return extremum_impl(false, reinterpret_cast<const float*>(X), x_rows, ldx, reinterpret_cast<float*>(Z), ldz, dtype, GRAPH_IN, D,
                       workspace, workspace_bytes, stream_v, reduce, arg_out, nullptr, ldarg, nullptr);
}

extern "C" int hcspmm_forward_extremum_backward(const float* grad_Z, int64_t ldg, const int32_t* arg, int64_t ldarg, float* grad_X,
                                                int64_t ldgx, const int32_t* rowptr, const int32_t* col,
                                                const int32_t* blockPartition, const int32_t* edgeToColumn,
                                                const int32_t* edgeToRow, const int32_t* hybrid_type, const int32_t* plan_d,
                                                const hcspmm_plan_header* ph, int64_t N, int64_t E, int D,
                                                const int32_t* transpose_perm, void* workspace, size_t workspace_bytes,
                                                void* stream_v) {
  return extremum_impl(true, grad_Z, N, ldg, grad_X, ldgx, HCSPMM_DTYPE_F32, GRAPH_IN, D, workspace, workspace_bytes, stream_v,
                       HCSPMM_REDUCE_MAX, nullptr, arg, ldarg, transpose_perm);
}

extern "C" size_t hcspmm_multi_workspace_bytes(const hcspmm_plan_header* ph, int D) { return 6 * hcspmm_workspace_bytes(ph, D); }

// Sum, sum of squares, max and min in one gather pass (spmm_multi.hip): the plan and checks of hcspmm_forward_extremum, six
// nullable outputs.
extern "C" int hcspmm_forward_multi(const void* X, int64_t x_rows, int64_t ldx, int dtype, float* Z_sum, float* Z_sumsq, float* Z_max,
                                    float* Z_min, int64_t ldz, int32_t* arg_max, int32_t* arg_min, int64_t ldarg,
                                    const int32_t* rowptr, const int32_t* col, const int32_t* blockPartition,
                                    const int32_t* edgeToColumn, const int32_t* edgeToRow, const int32_t* hybrid_type,
                                    const int32_t* plan_d, const hcspmm_plan_header* ph, int64_t N, int64_t E, int D, void* workspace,
                                    size_t workspace_bytes, void* stream_v) {
  if (dtype != HCSPMM_DTYPE_F32) return HCSPMM_EINVAL;
  if (N < 0 || E < 0 || D <= 0 || ldx < D || ldz < D) return HCSPMM_EINVAL;
  if (!Z_sum && !Z_sumsq && !Z_max && !Z_min) return HCSPMM_EINVAL;
  if ((arg_max || arg_min) && ldarg < D) return HCSPMM_EINVAL;
  if (N == 0) return HCSPMM_OK;
  if (!X || !rowptr || (E > 0 && !col)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  hcspmm::MArgs m{};
  // workspace: six areas of hcspmm_workspace_bytes each -- sum, sum of squares, max, its position, min, its position
  const int rc = bind_graph(m.p, GRAPH_IN, D, x_rows, workspace, workspace_bytes, 6, HCSPMM_DTYPE_F32);
  if (rc != HCSPMM_OK) return rc;
  if (m.p.plan) {
    m.area = hcspmm_workspace_bytes(ph, D) / sizeof(float);
    m.segment_len = ph->segment_len;
  }
  set_operands(m.p, X, nullptr, ldx, ldz);
  m.rowptr = rowptr;
  m.zsum = Z_sum;
  m.zsumsq = Z_sumsq;
  m.zmax = Z_max;
  m.zmin = Z_min;
  m.amax = arg_max;
  m.amin = arg_min;
  m.ldarg = (size_t)ldarg;
  const int vec = pick_vec(HCSPMM_DTYPE_F32, D, ldx, ldz, X, nullptr, nullptr);
  const hipError_t e = hcspmm::launch_multi_f32(m, vec, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

extern "C" size_t hcspmm_softmax_workspace_bytes(const hcspmm_plan_header* ph, int D) { return 4 * hcspmm_workspace_bytes(ph, D); }

// Per-channel softmax aggregation (spmm_softmax.hip): the plan and checks of hcspmm_forward_multi, Z required, three nullable
// statistics.
extern "C" int hcspmm_forward_softmax(const void* X, int64_t x_rows, int64_t ldx, int dtype, const float* beta, float* Z, float* M,
                                      float* L, float* Q, int64_t ldz, const int32_t* rowptr, const int32_t* col,
                                      const int32_t* blockPartition, const int32_t* edgeToColumn, const int32_t* edgeToRow,
                                      const int32_t* hybrid_type, const int32_t* plan_d, const hcspmm_plan_header* ph, int64_t N,
                                      int64_t E, int D, void* workspace, size_t workspace_bytes, void* stream_v) {
  if (dtype != HCSPMM_DTYPE_F32) return HCSPMM_EINVAL;
  if (N < 0 || E < 0 || D <= 0 || ldx < D || ldz < D) return HCSPMM_EINVAL;
  if (!Z || !beta) return HCSPMM_EINVAL;
  if (N == 0) return HCSPMM_OK;
  if (!X || !rowptr || (E > 0 && !col)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  hcspmm::SArgs s{};
  // workspace: four areas of hcspmm_workspace_bytes each -- m, l, a, q of the split rows' partial slots
  const int rc = bind_graph(s.p, GRAPH_IN, D, x_rows, workspace, workspace_bytes, 4, HCSPMM_DTYPE_F32);
  if (rc != HCSPMM_OK) return rc;
  if (s.p.plan) {
    s.area = hcspmm_workspace_bytes(ph, D) / sizeof(float);
    s.segment_len = ph->segment_len;
  }
  set_operands(s.p, X, nullptr, ldx, ldz);
  s.rowptr = rowptr;
  s.beta = beta;
  s.z = Z;
  s.m = M;
  s.l = L;
  s.q = Q;
  const int vec = pick_vec(HCSPMM_DTYPE_F32, D, ldx, ldz, X, nullptr, nullptr);
  const hipError_t e = hcspmm::launch_softmax_f32(s, vec, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

// Its gradient with respect to X (softmax_aggr_grad.hip) on the graph the backward walks: a plain-sum launch, one partial area.
extern "C" int hcspmm_softmax_backward(const float* grad_Z, const float* Z, const float* M, const float* L, int64_t ld_in,
                                       int64_t src_rows, const float* X, int64_t ldx, const float* beta, float* grad_X, int64_t ldgx,
                                       const int32_t* rowptr, const int32_t* col, const int32_t* blockPartition,
                                       const int32_t* edgeToColumn, const int32_t* edgeToRow, const int32_t* hybrid_type,
                                       const int32_t* plan_d, const hcspmm_plan_header* ph, int64_t N, int64_t E, int D,
                                       void* workspace, size_t workspace_bytes, void* stream_v) {
  if (N < 0 || E < 0 || src_rows < 0 || D <= 0 || ld_in < D || ldx < D || ldgx < D) return HCSPMM_EINVAL;
  if (!grad_X || !beta) return HCSPMM_EINVAL;
  if (N == 0) return HCSPMM_OK;
  if (!X || !rowptr || (E > 0 && (!col || !grad_Z || !Z || !M || !L || src_rows == 0))) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  hcspmm::SGradArgs a{};
  const int rc = bind_graph(a.p, GRAPH_IN, D, src_rows, workspace, workspace_bytes, 1, HCSPMM_DTYPE_F32);
  if (rc != HCSPMM_OK) return rc;
  if (a.p.plan) a.segment_len = ph->segment_len;
  set_operands(a.p, X, grad_X, ldx, ldgx);
  a.rowptr = rowptr;
  a.beta = beta;
  a.G = grad_Z;
  a.Zf = Z;
  a.M = M;
  a.L = L;
  a.ld_in = (size_t)ld_in;
  const int vec = pick_vec(HCSPMM_DTYPE_F32, D, ldx, ldgx, X, grad_X, nullptr);
  const hipError_t e = hcspmm::launch_softmax_backward_f32(a, vec, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

extern "C" size_t hcspmm_gated_workspace_bytes(const hcspmm_plan_header* ph, int D) { return 2 * hcspmm_workspace_bytes(ph, D); }

// Gated neighbour aggregation (spmm_gated.hip): a plain-sum launch per output on the binary product's plan, P read by row, Q and V
// gathered; one workspace area per output.
extern "C" int hcspmm_forward_gated(const float* P, int64_t ldp, const float* Q, int64_t ldq, const float* V, int64_t ldv,
                                    int64_t src_rows, float* Z_gate, float* Z_dgate, int64_t ldz, const int32_t* rowptr,
                                    const int32_t* col, const int32_t* blockPartition, const int32_t* edgeToColumn,
                                    const int32_t* edgeToRow, const int32_t* hybrid_type, const int32_t* plan_d,
                                    const hcspmm_plan_header* ph, int64_t N, int64_t E, int D, void* workspace,
                                    size_t workspace_bytes, void* stream_v) {
  if (N < 0 || E < 0 || src_rows < 0 || D <= 0 || ldp < D || ldq < D || ldv < D || ldz < D) return HCSPMM_EINVAL;
  if (!Z_gate && !Z_dgate) return HCSPMM_EINVAL;
  if (N == 0) return HCSPMM_OK;
  if (!P || !rowptr || (E > 0 && (!col || !Q || !V || src_rows == 0))) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  hcspmm::GatedArgs a{};
  // workspace: two areas of hcspmm_workspace_bytes each, one per output (a single-output call uses the first)
  const int rc = bind_graph(a.p, GRAPH_IN, D, src_rows, workspace, workspace_bytes, 2, HCSPMM_DTYPE_F32);
  if (rc != HCSPMM_OK) return rc;
  if (a.p.plan) {
    a.area = hcspmm_workspace_bytes(ph, D) / sizeof(float);
    a.segment_len = ph->segment_len;
  }
  a.outputs = (Z_gate ? 1 : 0) | (Z_dgate ? 2 : 0);
  set_operands(a.p, nullptr, Z_gate ? Z_gate : Z_dgate, ldp, ldz);
  a.z2 = Z_gate ? Z_dgate : nullptr;
  a.rowptr = rowptr;
  a.P = P;
  a.Q = Q;
  a.V = V;
  a.ldp = (size_t)ldp;
  a.ldq = (size_t)ldq;
  a.ldv = (size_t)ldv;
  const int vec = pick_vec(HCSPMM_DTYPE_F32, D, ldp, ldz, P, nullptr, nullptr);
  const hipError_t e = hcspmm::launch_gated_f32(a, vec, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

// Edge-feature messages (spmm_edge_messages.hip): the plan, checks and launch decisions of hcspmm_forward_weighted in fp32, F read on
// every call.
extern "C" int hcspmm_forward_edge_messages(const void* X, int64_t x_rows, int64_t ldx, const float* F, int64_t f_rows, int64_t ldf,
                                            const int32_t* f_index, int op, void* Z, int64_t ldz, const int32_t* rowptr,
                                            const int32_t* col, const int32_t* blockPartition, const int32_t* edgeToColumn,
                                            const int32_t* edgeToRow, const int32_t* hybrid_type, const int32_t* plan_d,
                                            const hcspmm_plan_header* ph, int64_t N, int64_t E, int D, void* workspace,
                                            size_t workspace_bytes, void* stream_v) {
  if (op != HCSPMM_EDGE_OP_MUL && op != HCSPMM_EDGE_OP_ADD_RELU && op != HCSPMM_EDGE_OP_COPY) return HCSPMM_EINVAL;
  const bool reads_x = op != HCSPMM_EDGE_OP_COPY;
  if (N < 0 || E < 0 || D <= 0 || f_rows < 0 || ldf < D || ldz < D || (reads_x && ldx < D)) return HCSPMM_EINVAL;
  if (E > 0 && (!F || f_rows == 0 || (!f_index && f_rows < E))) return HCSPMM_EINVAL;
  if (N == 0) return HCSPMM_OK;
  if ((reads_x && !X) || !Z || !rowptr || (E > 0 && !col)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX || f_rows > INT32_MAX) return HCSPMM_ERANGE;
  hcspmm::EdgeMsgArgs a{};
  const int rc = bind_graph(a.p, GRAPH_IN, D, reads_x ? x_rows : kNoSource, workspace, workspace_bytes, 1, HCSPMM_DTYPE_F32);
  if (rc != HCSPMM_OK) return rc;
  if (a.p.plan) a.segment_len = ph->segment_len;
  set_operands(a.p, reads_x ? X : nullptr, Z, ldx, ldz);
  a.rowptr = rowptr;
  a.op = op;
  a.F = F;
  a.ldf = (size_t)ldf;
  a.findex = f_index;
  const int vec = pick_vec(HCSPMM_DTYPE_F32, D, ldx, ldz, X, Z, nullptr);
  const hipError_t e = hcspmm::launch_edge_messages_f32(a, vec, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

// Gradient of the edge-feature messages with respect to F (edge_messages_grad.hip): column_index is trusted, as in the plan-free
// hcspmm_sddmm.
extern "C" int hcspmm_edge_messages_grad(const float* grad_Z, int64_t ldg, const float* X, int64_t x_rows, int64_t ldx, const float* F,
                                         int64_t ldf, float* grad_F, int64_t ldgf, int op, const int32_t* rowptr, const int32_t* col,
                                         int64_t N, int64_t E, int D, void* stream_v) {
  if (op != HCSPMM_EDGE_OP_MUL && op != HCSPMM_EDGE_OP_ADD_RELU && op != HCSPMM_EDGE_OP_COPY) return HCSPMM_EINVAL;
  const bool reads_x = op != HCSPMM_EDGE_OP_COPY, reads_f = op == HCSPMM_EDGE_OP_ADD_RELU;
  if (N < 0 || E < 0 || D <= 0 || ldg < D || ldgf < D || (reads_x && (ldx < D || x_rows < 0)) || (reads_f && ldf < D))
    return HCSPMM_EINVAL;
  if (!rowptr || (E > 0 && (!grad_Z || !grad_F || !col || N == 0 || (reads_x && (!X || x_rows == 0)) || (reads_f && !F))))
    return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  if (E == 0) return HCSPMM_OK;
  hcspmm::EdgeMsgGradArgs a{};
  a.gZ = grad_Z;
  a.X = X;
  a.F = F;
  a.gF = grad_F;
  a.ldg = (size_t)ldg;
  a.ldx = (size_t)ldx;
  a.ldf = (size_t)ldf;
  a.ldgf = (size_t)ldgf;
  a.rowptr = rowptr;
  a.col = col;
  a.N = (int)N;
  a.D = D;
  a.op = op;
  a.E = (long long)E;
  const int vec = pick_vec(HCSPMM_DTYPE_F32, D, ldg, ldgf, grad_Z, grad_F, nullptr);
  const hipError_t e = hcspmm::launch_edge_messages_grad_f32(a, vec, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

extern "C" int hcspmm_edge_norm_device(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t E, int kind,
                                       float* values_out, void* stream_v) {
  if (N < 0 || E < 0 || (kind != HCSPMM_NORM_SYM && kind != HCSPMM_NORM_MEAN)) return HCSPMM_EINVAL;
  if (E > 0 && (!rowptr || !col || !values_out || N == 0)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  const hipError_t e = hcspmm::launch_edge_norm(rowptr, col, (int)N, (long long)E, kind == HCSPMM_NORM_SYM ? 0 : 1, values_out,
                                                reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

namespace {
// heads > 0: the multi-head form (fp32, Dh = D / heads columns per head, Dh % 4 == 0); 0: hcspmm_sddmm
int sddmm_impl(const void* A, int64_t lda, const void* B, int64_t b_rows, int64_t ldb, int dtype, float* out,
               const int32_t* rowptr, const int32_t* col, const int32_t* plan_d, const hcspmm_plan_header* ph, int64_t N,
               int64_t E, int D, void* stream_v, int heads) {
  if (dtype < HCSPMM_DTYPE_F32 || dtype > HCSPMM_DTYPE_BF16) return HCSPMM_EINVAL;
  if (heads > 0 && (dtype != HCSPMM_DTYPE_F32 || D <= 0 || D % heads != 0 || (D / heads) % 4 != 0)) return HCSPMM_EINVAL;
  if (heads > 0 && (long long)E * heads > INT64_MAX / 4) return HCSPMM_ERANGE;
  if (N < 0 || E < 0 || b_rows < 0 || D <= 0 || lda < D || ldb < D) return HCSPMM_EINVAL;
  if (!rowptr || (E > 0 && (!A || !B || !out || !col || N == 0))) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX) return HCSPMM_ERANGE;
  if ((plan_d == nullptr) != (ph == nullptr)) return HCSPMM_EINVAL;  // both or neither
  if (ph) {
    const int rc = hcspmm_plan_check(ph, N, E, 0);
    if (rc != HCSPMM_OK) return rc;
    if (b_rows < ph->num_columns) return HCSPMM_EINVAL;  // the graph gathers rows B does not have
  }
  if (E == 0) return HCSPMM_OK;
  const int dh = heads > 0 ? D / heads : D;
  hcspmm::SddmmArgs a{A, B, (size_t)lda, (size_t)ldb, rowptr, col, out, (int)N, dh, (long long)E};
  const int vec = pick_vec(dtype, dh, lda, ldb, A, B, nullptr);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
  const hipError_t e = heads > 0 ? hcspmm::launch_sddmm_heads_f32(a, heads, vec, stream)
                                 : launch_typed(dtype, hcspmm::launch_sddmm_f32, hcspmm::launch_sddmm_f16, hcspmm::launch_sddmm_bf16, a,
                                                vec, stream);
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}
}  // namespace

// SDDMM (sddmm.hip): out[e] = <A[row(e)], B[col(e)]>.  With a plan its header vouches for the column range, as in
// hcspmm_forward_typed; plan-free, column_index is trusted.
extern "C" int hcspmm_sddmm(const void* A, int64_t lda, const void* B, int64_t b_rows, int64_t ldb, int dtype, float* out,
                            const int32_t* rowptr, const int32_t* col, const int32_t* plan_d, const hcspmm_plan_header* ph,
                            int64_t N, int64_t E, int D, void* stream_v) {
  return sddmm_impl(A, lda, B, b_rows, ldb, dtype, out, rowptr, col, plan_d, ph, N, E, D, stream_v, 0);
}

// Multi-head SDDMM (sddmm_heads.hip): hcspmm_sddmm's checks, then heads column slices of D / heads in one launch; fp32 only.
extern "C" int hcspmm_sddmm_heads(const void* A, int64_t lda, const void* B, int64_t b_rows, int64_t ldb, int dtype, float* out,
                                  const int32_t* rowptr, const int32_t* col, const int32_t* plan_d, const hcspmm_plan_header* ph,
                                  int64_t N, int64_t E, int D, void* stream_v, int heads) {
  if (heads <= 0) return HCSPMM_EINVAL;
  return sddmm_impl(A, lda, B, b_rows, ldb, dtype, out, rowptr, col, plan_d, ph, N, E, D, stream_v, heads);
}

namespace {
int edge_softmax_impl(const float* x, const float* y, float* out, const int32_t* rowptr, int64_t N, int64_t E, int heads,
                      void* stream_v, bool backward) {
  if (N < 0 || E < 0 || heads <= 0 || !rowptr) return HCSPMM_EINVAL;
  if (E > 0 && (!x || !out || (backward && !y) || N == 0)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX || (long long)E * heads > INT64_MAX / 4) return HCSPMM_ERANGE;
  const hcspmm::SoftmaxArgs a{x, y, out, rowptr, (int)N, heads, (long long)E};
  const hipError_t e = hcspmm::launch_edge_softmax(a, backward, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}
}  // namespace

extern "C" int hcspmm_edge_softmax(const float* logits, float* alpha, const int32_t* rowptr, int64_t N, int64_t E, int heads,
                                   void* stream_v) {
  return edge_softmax_impl(logits, nullptr, alpha, rowptr, N, E, heads, stream_v, false);
}

extern "C" int hcspmm_edge_softmax_backward(const float* alpha, const float* grad_alpha, float* grad_logits, const int32_t* rowptr,
                                            int64_t N, int64_t E, int heads, void* stream_v) {
  return edge_softmax_impl(alpha, grad_alpha, grad_logits, rowptr, N, E, heads, stream_v, true);
}

// GAT attention (gat_attention.hip).  Every array with at least one element needs a pointer; column ids (and perm) are
// trusted, as on the plan-free paths.
extern "C" int hcspmm_gat_attention(const float* s_dst, const float* s_src, int64_t src_rows, float slope, float* alpha,
                                    const int32_t* rowptr, const int32_t* col, int64_t N, int64_t E, int heads, void* stream_v) {
  if (N < 0 || E < 0 || src_rows < 0 || heads <= 0 || !rowptr || !__builtin_isfinite(slope)) return HCSPMM_EINVAL;
  if ((N > 0 && !s_dst) || (src_rows > 0 && !s_src)) return HCSPMM_EINVAL;
  if (E > 0 && (!alpha || !col || N == 0 || src_rows == 0)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX || E * heads > INT64_MAX / 4 || N * heads > INT64_MAX / 4 ||
      src_rows > INT64_MAX / 4 / heads)
    return HCSPMM_ERANGE;
  const hcspmm::GatArgs a{s_dst, s_src, nullptr, nullptr, rowptr, col, nullptr, alpha, nullptr, nullptr, slope, (int)N, heads,
                          (long long)E};
  const hipError_t e = hcspmm::launch_gat_attention(a, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

namespace {
// rowptr_t / perm / n_t: the rows of A^T (the pattern-symmetric entry point passes A's own and N)
int gat_backward_impl(const float* alpha, const float* grad_alpha, const float* s_dst, const float* s_src, float slope,
                      const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_t, const int32_t* perm, int64_t n_t, int64_t N,
                      int64_t E, int heads, float* grad_scores, float* grad_s_dst, float* grad_s_src, void* stream_v) {
  if (N < 0 || E < 0 || n_t < 0 || heads <= 0 || !rowptr || !rowptr_t || !__builtin_isfinite(slope)) return HCSPMM_EINVAL;
  if ((N > 0 && (!s_dst || !grad_s_dst)) || (n_t > 0 && (!s_src || !grad_s_src))) return HCSPMM_EINVAL;
  if (E > 0 && (!alpha || !grad_alpha || !col || !perm || !grad_scores || N == 0 || n_t == 0)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || n_t > INT32_MAX - 16 || E > INT32_MAX || E * heads > INT64_MAX / 4 || N * heads > INT64_MAX / 4 ||
      n_t * heads > INT64_MAX / 4)
    return HCSPMM_ERANGE;
  const hcspmm::GatArgs a{s_dst, s_src, alpha, grad_alpha, rowptr, col, perm, grad_scores, grad_s_dst, grad_s_src, slope, (int)N,
                          heads, (long long)E, rowptr_t, (int)n_t};
  const hipError_t e = hcspmm::launch_gat_attention_backward(a, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}
}  // namespace

extern "C" int hcspmm_gat_attention_backward(const float* alpha, const float* grad_alpha, const float* s_dst, const float* s_src,
                                             float slope, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t N,
                                             int64_t E, int heads, float* grad_scores, float* grad_s_dst, float* grad_s_src,
                                             void* stream_v) {
  return gat_backward_impl(alpha, grad_alpha, s_dst, s_src, slope, rowptr, col, rowptr, perm, N, N, E, heads, grad_scores,
                           grad_s_dst, grad_s_src, stream_v);
}

// The same launches walking A^T's rows for the column side (hcspmm_transpose_graph): no symmetry needed.
extern "C" int hcspmm_gat_attention_backward_directed(const float* alpha, const float* grad_alpha, const float* s_dst,
                                                      const float* s_src, float slope, const int32_t* rowptr, const int32_t* col,
                                                      const int32_t* rowptr_t, const int32_t* entry_t, int64_t src_rows, int64_t N,
                                                      int64_t E, int heads, float* grad_scores, float* grad_s_dst,
                                                      float* grad_s_src, void* stream_v) {
  return gat_backward_impl(alpha, grad_alpha, s_dst, s_src, slope, rowptr, col, rowptr_t, entry_t, src_rows, N, E, heads,
                           grad_scores, grad_s_dst, grad_s_src, stream_v);
}

// GATv2 attention logits (gatv2_attention.hip).  Every array with at least one element needs a pointer; column ids (and
// perm) are trusted, as on the plan-free paths.
namespace {
bool gatv2_shape_ok(int D, int heads) { return heads > 0 && D > 0 && D % heads == 0 && (D / heads) % 4 == 0; }
}  // namespace

extern "C" int hcspmm_gatv2_scores(const float* H_dst, int64_t ld_dst, const float* H_src, int64_t src_rows, int64_t ld_src,
                                   const float* att, float slope, float* logits, const int32_t* rowptr, const int32_t* col,
                                   int64_t N, int64_t E, int D, int heads, void* stream_v) {
  if (N < 0 || E < 0 || src_rows < 0 || !gatv2_shape_ok(D, heads) || ld_dst < D || ld_src < D || !rowptr || !att ||
      !__builtin_isfinite(slope))
    return HCSPMM_EINVAL;
  if ((N > 0 && !H_dst) || (src_rows > 0 && !H_src)) return HCSPMM_EINVAL;
  if (E > 0 && (!logits || !col || N == 0 || src_rows == 0)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 16 || E > INT32_MAX || E > INT64_MAX / 4 / heads) return HCSPMM_ERANGE;
  if (E == 0) return HCSPMM_OK;
  hcspmm::Gatv2Args a{};
  a.H_dst = H_dst, a.H_src = H_src, a.att = att, a.rowptr = rowptr, a.col = col, a.out = logits;
  a.ld_dst = (size_t)ld_dst, a.ld_src = (size_t)ld_src;
  a.slope = slope, a.N = (int)N, a.D = D, a.heads = heads, a.E = (long long)E;
  const hipError_t e = hcspmm::launch_gatv2_scores(a, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

extern "C" size_t hcspmm_gatv2_backward_workspace_bytes(int64_t N, int64_t E, int D, int heads) {
  if (N <= 0 || E < 0 || !gatv2_shape_ok(D, heads) || N > INT32_MAX - 2048) return 0;
  return (size_t)hcspmm::gatv2_grad_blocks((long long)N, D) * (size_t)D * sizeof(float);
}

namespace {
// rowptr_t / col_t / perm / n_t: A^T (the pattern-symmetric entry point passes A's own arrays and N)
int gatv2_backward_impl(const float* grad_logits, const float* H_dst, int64_t ld_dst, const float* H_src, int64_t ld_src,
                        const float* att, float slope, const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_t,
                        const int32_t* col_t, const int32_t* perm, int64_t n_t, int64_t N, int64_t E, int D, int heads,
                        float* grad_dst, int64_t ld_gdst, float* grad_src, int64_t ld_gsrc, float* grad_att, void* workspace,
                        size_t workspace_bytes, void* stream_v) {
  if (N < 0 || E < 0 || n_t < 0 || !gatv2_shape_ok(D, heads) || ld_dst < D || ld_src < D || ld_gdst < D || ld_gsrc < D || !rowptr ||
      !rowptr_t || !att || !grad_att || !__builtin_isfinite(slope))
    return HCSPMM_EINVAL;
  if ((N > 0 && (!H_dst || !grad_dst)) || (n_t > 0 && (!H_src || !grad_src))) return HCSPMM_EINVAL;
  if (E > 0 && (!grad_logits || !col || !col_t || !perm || N == 0 || n_t == 0)) return HCSPMM_EINVAL;
  if (N > INT32_MAX - 2048 || n_t > INT32_MAX - 2048 || E > INT32_MAX - 4096 || E > INT64_MAX / 4 / heads) return HCSPMM_ERANGE;
  const size_t need = hcspmm_gatv2_backward_workspace_bytes(N, E, D, heads);
  if (workspace_bytes < need) return HCSPMM_EWORKSPACE;
  if (need > 0 && !workspace) return HCSPMM_EINVAL;
  hcspmm::Gatv2Args a{};
  a.H_dst = H_dst, a.H_src = H_src, a.att = att, a.g = grad_logits, a.rowptr = rowptr, a.col = col, a.perm = perm;
  a.rowptr_t = rowptr_t, a.col_t = col_t, a.n_t = (int)n_t;
  a.grad_dst = grad_dst, a.grad_src = grad_src, a.grad_att = grad_att, a.partial = static_cast<float*>(workspace);
  a.ld_dst = (size_t)ld_dst, a.ld_src = (size_t)ld_src, a.ld_gdst = (size_t)ld_gdst, a.ld_gsrc = (size_t)ld_gsrc;
  a.slope = slope, a.N = (int)N, a.D = D, a.heads = heads, a.E = (long long)E;
  // E = 0 takes the same launches: every row is empty, so all three gradients come out as zeros
  const hipError_t e = hcspmm::launch_gatv2_backward(a, reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}
}  // namespace

extern "C" int hcspmm_gatv2_scores_backward(const float* grad_logits, const float* H_dst, int64_t ld_dst, const float* H_src,
                                            int64_t ld_src, const float* att, float slope, const int32_t* rowptr,
                                            const int32_t* col, const int32_t* perm, int64_t N, int64_t E, int D, int heads,
                                            float* grad_dst, int64_t ld_gdst, float* grad_src, int64_t ld_gsrc, float* grad_att,
                                            void* workspace, size_t workspace_bytes, void* stream_v) {
  return gatv2_backward_impl(grad_logits, H_dst, ld_dst, H_src, ld_src, att, slope, rowptr, col, rowptr, col, perm, N, N, E, D, heads,
                             grad_dst, ld_gdst, grad_src, ld_gsrc, grad_att, workspace, workspace_bytes, stream_v);
}

// The same launches walking A^T (hcspmm_transpose_graph) for grad_H_src: no symmetry needed.
extern "C" int hcspmm_gatv2_scores_backward_directed(const float* grad_logits, const float* H_dst, int64_t ld_dst,
                                                     const float* H_src, int64_t ld_src, const float* att, float slope,
                                                     const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_t,
                                                     const int32_t* col_t, const int32_t* entry_t, int64_t src_rows, int64_t N,
                                                     int64_t E, int D, int heads, float* grad_dst, int64_t ld_gdst, float* grad_src,
                                                     int64_t ld_gsrc, float* grad_att, void* workspace, size_t workspace_bytes,
                                                     void* stream_v) {
  return gatv2_backward_impl(grad_logits, H_dst, ld_dst, H_src, ld_src, att, slope, rowptr, col, rowptr_t, col_t, entry_t, src_rows, N,
                             E, D, heads, grad_dst, ld_gdst, grad_src, ld_gsrc, grad_att, workspace, workspace_bytes, stream_v);
}

extern "C" int hcspmm_forward_strided(const float* X, int64_t x_rows, int64_t ldx, float* Z, int64_t ldz, const int32_t* rowptr,
                                      const int32_t* col, const int32_t* blockPartition, const int32_t* edgeToColumn,
                                      const int32_t* edgeToRow, const int32_t* hybrid_type, const int32_t* plan_d,
                                      const hcspmm_plan_header* ph, int64_t N, int64_t E, int D, void* workspace,
                                      size_t workspace_bytes, void* stream_v) {
  return hcspmm_forward_typed(X, x_rows, ldx, Z, ldz, HCSPMM_DTYPE_F32, rowptr, col, blockPartition, edgeToColumn, edgeToRow,
                              hybrid_type, plan_d, ph, N, E, D, workspace, workspace_bytes, stream_v);
}

extern "C" int hcspmm_forward(const float* X, float* Z, const int32_t* rowptr, const int32_t* col,
                              const int32_t* blockPartition, const int32_t* edgeToColumn, const int32_t* edgeToRow,
                              const int32_t* hybrid_type, const int32_t* plan_d, const hcspmm_plan_header* ph,
                              int64_t N, int64_t E, int D, void* workspace, size_t workspace_bytes, void* stream_v) {
  return hcspmm_forward_strided(X, N, D, Z, D, rowptr, col, blockPartition, edgeToColumn, edgeToRow, hybrid_type, plan_d, ph,
                                N, E, D, workspace, workspace_bytes, stream_v);
}

// Forms of the fused operators (fp32).  0: two launches -- hybrid SpMM (out2 = A*X), then the streaming update over all rows.
// 1 ("in-launch", plans built with hcspmm_plan_params.fuse_in_launch = 1): the dense-tile windows multiply their tile by the
// weights while it is in the MFMA accumulators (spmm_impl.h fused_dense_region); the windows on the sparse-row path -- listed
// in the plan (off_sparse_windows) -- go through the update kernel afterwards.  Slower than 0 on MI355X (profiles/r02/ab_fused.log).
// 2 ("row-tile", fused_rows.hip): tiles of 16 consecutive tasks of the length-sorted list, and dense windows, are summed,
// written to out2, parked in LDS and multiplied before they leave the CU; the hybrid launch keeps the sliced and wide tasks,
// whose rows (a few thousand) a small launch multiplies behind the fix-up pass.  `out` has form 0's bits.  Needs the sparse
// region in ONE column pass (D < 64, or a short-row graph), 17 <= D <= 128, H <= 32 or 49 ... 64 (widths off the 16-column grid padded).
// Which one: HCSPMM_FUSED_SINGLE_LAUNCH=0 / 1 / 2 in the environment, else the plan's flags (fuse_in_launch = -1 / 1 / 2),
// else automatic: form 2 when out2 (N x D fp32) is 80 MB or more at D <= 64 -- it is then beyond what the update launch
// finds in the caches next to X and out, and not re-reading it is worth +2 ... +34 % (profiles/r03/ab_fused_rows.log: TT / RD /
// YeastH-sized low-degree graphs and dense-heavy graphs from 1/5 of their size up; every point above 80 MB gains, every
// sparse-row point below it loses 4-20 % -- the cache-resident Reddit-scale graph 1-2 %).  Beyond 64 columns (whole-row tiles
// up to 112 columns, two column chunks of 64 with eight-wave workgroups at 128) the tiles' LDS area costs occupancy: with
// H <= 32 graphs with a quarter of their rows in dense-tile windows gain 5-22 % (automatic from 256 MB of out2), sparse-row
// graphs -2 ... +4 %, and H = 64 is mixed (-6 ... +4 %), so those stay
// opt-in.  A shape outside a form falls back to the next one down.
static int fused_form(const hcspmm_plan_header* ph, const void* X, const void* out2, const void* out, int D, int H,
                      const void* workspace = nullptr) {
  static const int forced = [] {
    const char* e = getenv("HCSPMM_FUSED_SINGLE_LAUNCH");
    return !e ? -1 : (e[0] == '0' ? 0 : (e[0] == '2' ? 2 : 1));
  }();
  if (!ph) return 0;
  int asked = forced;
  if (asked < 0) {
    if (ph->flags & HCSPMM_PLAN_FUSE_NEVER) asked = 0;
    else if (ph->flags & HCSPMM_PLAN_FUSE_ROWS) asked = 2;
    else if (ph->flags & HCSPMM_PLAN_FUSE_IN_LAUNCH) asked = 1;
    else {
      const double out2_bytes = (double)ph->num_nodes * (double)D * 4.0;
      const bool dense_heavy = 64.0 * (double)ph->n_dense >= (double)ph->num_nodes;  // a quarter of the rows in dense-tile windows
      asked = (D <= 64 ? out2_bytes >= 80e6 : (D <= 128 && H <= 32 && dense_heavy && out2_bytes >= 256e6)) ? 2 : 0;
      // (both widths off the 16-column grid -- 22 x 22 -- is the one padded shape that measured slower than two launches on the
      // sparse-row graphs, -9 ... -12 %: profiles/r04/ab_dense_panels.log; it stays opt-in)
      if (D % 16 != 0 && H % 16 != 0) asked = 0;
    }
  }
  if (asked == 0) return 0;
  // both forms are 16-byte-per-lane builds: a caller's workspace that is only 4- or 8-byte aligned takes the two-launch form
  // (which serves every alignment) instead of failing
  if (!aligned(X, 16) || !aligned(out2, 16) || (workspace && !aligned(workspace, 16))) return 0;
  if (asked >= 2 && hcspmm::fused_tiles_supported(D, H) && aligned(out, 16) && panel_choice(ph, D, HCSPMM_DTYPE_F32) >= D) return 2;
  if (!(ph->flags & HCSPMM_PLAN_FUSE_IN_LAUNCH) && forced != 1) return 0;  // form 1 only where it was asked for by name
  bool dense_ok = ph->n_dense > 0 && D % 16 == 0 && D >= 32 && H % 16 == 0 && H <= 32 && H > 0;
  if (dense_ok) {
    const int dv = D <= 32 ? 2 : 4;  // (plan_layout.h: the narrowest lane width that covers the row in one panel)
    const int rows = (D + 16 * dv - 1) / (16 * dv) * 16 * dv;
    dense_ok = (size_t)rows * (size_t)(H + 4) * sizeof(float) <= 64 * 1024;
  }
  return dense_ok ? 1 : 0;
}

extern "C" int hcspmm_fused_in_launch(const hcspmm_plan_header* ph, int D, int H) {
  return fused_form(ph, nullptr, nullptr, nullptr, D, H);  // (null pointers count as aligned)
}

extern "C" int hcspmm_forward_fused(const float* X, float* out, float* out2, const float* weights, int64_t ldr,
                                    int64_t ldc, int H, const int32_t* rowptr, const int32_t* col,
                                    const int32_t* blockPartition, const int32_t* edgeToColumn,
                                    const int32_t* edgeToRow, const int32_t* hybrid_type, const int32_t* plan_d,
                                    const hcspmm_plan_header* ph, int64_t N, int64_t E, int D, void* workspace,
                                    size_t workspace_bytes, void* stream_v) {
  if (!out || !out2 || !weights || H <= 0) return HCSPMM_EINVAL;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
  const GraphIn g = GRAPH_IN;
  const int form = (plan_d && ph) ? fused_form(ph, X, out2, out, D, H, hcspmm_workspace_bytes(ph, D) ? workspace : nullptr) : 0;
  if (form == 2) {
    const FusedOperands f{weights, (long long)ldr, (long long)ldc, out, H, 2};
    const int rc = forward_impl(X, N, D, out2, D, HCSPMM_DTYPE_F32, g, D, workspace, workspace_bytes, stream_v, &f);
    if (rc != HCSPMM_OK) return rc;
    int n_wide = 0;
    wide_choice(ph, D, HCSPMM_DTYPE_F32, &n_wide);
    const hipError_t e = hcspmm::launch_dense_update_leftover(out2, weights, (long long)ldr, (long long)ldc, out, (int)N, D, H,
                                                              plan_d, ph->off_tasks, n_wide, ph->off_fixups, ph->n_split_rows,
                                                              ph->off_slice_tasks, ph->n_slice_tasks, stream);
    return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
  }
  if (form == 1) {
    const FusedOperands f{weights, (long long)ldr, (long long)ldc, out, H, 1};
    const int rc = forward_impl(X, N, D, out2, D, HCSPMM_DTYPE_F32, g, D, workspace, workspace_bytes, stream_v, &f);
    if (rc != HCSPMM_OK) return rc;
    if (ph->n_sparse_windows == 0) return HCSPMM_OK;
    const hipError_t e = hcspmm::launch_dense_update(out2, weights, (long long)ldr, (long long)ldc, out, (int)N, D, H,
                                                     plan_d + ph->off_sparse_windows, ph->n_sparse_windows, stream);
    return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
  }
  const int rc = hcspmm_forward(X, out2, rowptr, col, blockPartition, edgeToColumn, edgeToRow, hybrid_type, plan_d, ph,
                                N, E, D, workspace, workspace_bytes, stream_v);
  if (rc != HCSPMM_OK) return rc;
  const hipError_t e = hcspmm::launch_dense_update(out2, weights, (long long)ldr, (long long)ldc, out, (int)N, D, H, nullptr, 0,
                                                   stream);
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

extern "C" int hcspmm_dense_update(const float* in, const float* weights, int64_t ldr, int64_t ldc, float* out, int64_t N, int D,
                                   int H, void* stream_v) {
  if (N < 0 || D <= 0 || H <= 0 || (N > 0 && (!in || !weights || !out))) return HCSPMM_EINVAL;
  if (N > INT32_MAX) return HCSPMM_ERANGE;
  const hipError_t e = hcspmm::launch_dense_update(in, weights, (long long)ldr, (long long)ldc, out, (int)N, D, H, nullptr, 0,
                                                   reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

extern "C" size_t hcspmm_weight_grad_workspace(int64_t N, int D, int H) {
  if (N <= 0 || !hcspmm::weight_grad_supported(D, H)) return 0;
  return (size_t)hcspmm::weight_grad_groups(N) * (size_t)D * (size_t)H * sizeof(float);
}

extern "C" int hcspmm_weight_grad(const float* A, int64_t lda, const float* B, int64_t ldb, float* out, int64_t N, int D,
                                  int H, void* workspace, size_t workspace_bytes, void* stream_v) {
  if (N <= 0 || D <= 0 || H <= 0 || lda < D || ldb < H || !A || !B || !out) return HCSPMM_EINVAL;
  if (!hcspmm::weight_grad_supported(D, H)) return HCSPMM_EINVAL;
  if (N > INT32_MAX) return HCSPMM_ERANGE;
  if (!workspace || workspace_bytes < hcspmm_weight_grad_workspace(N, D, H)) return HCSPMM_EWORKSPACE;
  const hipError_t e = hcspmm::launch_weight_grad(A, lda, B, ldb, out, reinterpret_cast<float*>(workspace), N, D, H,
                                                  reinterpret_cast<hipStream_t>(stream_v));
  return e == hipSuccess ? HCSPMM_OK : fail_hip(e);
}

#undef GRAPH_IN
