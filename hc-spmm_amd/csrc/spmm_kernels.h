// spmm_kernels.h -- internal launch interface between capi.hip and the kernel translation units
// (spmm_kernels.hip: fp32, spmm_kernels_h16.hip: fp16 / bf16; device code in spmm_impl.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hcspmm {

// Arguments of the planned hybrid launch (device pointers; `plan` is the uploaded blob of
// hcspmm_plan_build, the off_* / n_* fields are copied from the host copy of its header).
struct PlanArgs {
  const void* X;  // features, element type of the launch (fp32, or fp16 / bf16 bits)
  void* Z;
  float* partial;  // workspace: n_partials x D partial sums of split rows
  const int* col;
  const int* plan;
  size_t ldx, ldz;  // row strides of X and Z in elements (>= D)
  int off_tasks, n_tasks;
  int off_dense_index, off_dense_pack, n_dense;
  int off_dense_compact, n_dense_compact;    // the last n_dense_compact dense windows use fixed 64-word records
  int off_dense_compact2, n_dense_compact2;  // the n_dense_compact2 before them use 128-word records
  int off_fixups, n_split_rows;
  int N, D;
  int n_wide;                          // the n_wide longest tasks are summed by whole waves
  int n_tiny;                          // the last n_tiny tasks carry their (<= 2) indices inline
  int panel_cols;                      // feature columns per sparse pass (D = one pass; 32 = panel-major)
  int sparse_wgs_pp, dense_vec;        // filled by the launcher
  int wide_wgs, sparse_wgs, n_panels;  // filled by the launcher
  int tiny_wgs;                        // filled by the launcher: workgroups of the tiny-task region (per panel)
  int tiny_kernel_wgs;                 // filled by the launcher: > 0 = the tiny tasks run as their own launch (per panel)
  // XCD-affine column slices (hcspmm.h n_slices): slice s owns descriptors [table[s], table[s+1]) of the slice task
  // list and is served by the workgroups b = s (mod 8) of the sliced region, the first slice_wgs of every panel
  int off_slice_table, off_slice_tasks, n_slices, slice_xcd_tasks;
  int slice_wgs;                       // filled by the launcher (a multiple of 8)
  int free_wgs_pp;                     // filled by the launcher: wide + ordinary + tiny workgroups per panel
  // fused aggregate+update (hcspmm_forward_fused, fp32 only): when fused != 0 every dense-tile window also
  // multiplies its 16 x D tile by the weights while it is still in the MFMA accumulators and writes 16 rows of
  // out (N x H, row-major); Z is then the operator's out2.  W: D x H with element strides (w_ldr, w_ldc).
  int fused, H;
  int fused_dense_wgs;  // filled by the launcher: workgroups of the fused dense region (each strides over windows)
  union {
    const float* W;
    // 8-bit weighted launches (spmm_weighted_f8.hip; they have no fused form): [x_rows] fp32 scales of the gathered rows, or null.
    // Entry e of column c weighs values[e] * row_scale[c], one fp32 multiplication; a null values / row_scale is 1 (both null is
    // the binary launch, launch_plan_f8)
    const float* row_scale;
  };
  long long w_ldr, w_ldc;
  float* out;
  // entries of col: the 16-byte index loads of sparse_task stay inside col[0, E).  (Last, so that no other member moves: one
  // more dword in the middle cost the 16-bit weighted L = 32 build four more bytes of scratch.)
  int E;
  // where the wide and the ordinary regions of the binary product's launch read their descriptors: off_tasks, or the plan's
  // exact-length schedule copy of the non-tiny tasks (hcspmm.h off_task_sched).  (Last as well, for the same reason.)
  int off_sched;
  // first-index records of the schedule copies (hcspmm.h off_task_sched_idx / off_slice_sched_idx), as word offsets into plan:
  // record i of a section holds the first (at most 32) column indices of descriptor i, padded with -1, so the ordinary and the
  // sliced waves of the binary product's launch ask for their first indices together with their descriptors.  0: the plan has
  // none, or the launch does not use them; the waves then read col behind the descriptor.  (Last, like off_sched.)
  int off_sched_idx, off_slice_idx;
  // the slice table itself (hcspmm.h slice_table_copy) when slice_tbl_n != 0: the sliced waves then find their list's bounds
  // in the kernel arguments instead of the plan
  int slice_tbl_n;
  int slice_tbl[9];
};

// Arguments of the row-tile fused launch (fused_rows.hip): the planned launch's arguments (Z = out2; W / out / H set) plus the
// tile counts.  fp32, 16 bytes per lane.
struct TilesArgs {
  PlanArgs p;
  int n_ord_tiles, n_tiny_tiles;  // filled by the launcher: tiles of 16 ordinary / tiny tasks
  int chunk, tile_stride;         // filled by the launcher: feature columns per pass of a sparse tile (D: one pass), words per tile row
};

// Arguments of the plan-free launch: the reference's seven graph tensors as they are.
struct WindowArgs {
  const void* X;
  void* Z;
  const int* rowptr;
  const int* col;
  const int* blockPartition;
  const int* edgeToColumn;
  const int* edgeToRow;
  const int* hybrid_type;
  size_t ldx, ldz;  // row strides of X and Z in elements (>= D)
  int N, D;
};

// Arguments of the weighted launches (spmm_weighted*.hip, hcspmm_forward_weighted): Z = A_w * X with A_w's values aligned with
// column_index.  The plan is the binary one, unchanged; the kernels find each entry's position from the task descriptors (ordinary,
// wide and sliced tasks carry their first entry), from rowptr (tiny tasks, dense-tile windows: a lane's entry is its row's first
// entry plus a running popcount of the row's mask bits) and from the fix-up list (tiny row segments).
struct WPlanArgs {
  PlanArgs p;
  const float* values;  // [E]
  const int* rowptr;    // [N + 1]
  int segment_len;      // plan header: entries per segment of a split row
};
struct WWindowArgs {
  WindowArgs w;
  const float* values;  // [E]
  const float* row_scale;  // 8-bit launches only: PlanArgs::row_scale of the plan-free form
};

// vec = elements per lane access.  fp32: 4 for every D >= 4 (element-aligned vectors: any stride, any base address), 2 / 1 for
// D = 2, 3 / 1.  16-bit: 8 (D >= 32) or 4 when D and the strides are even and the bases 4-byte aligned (dword-aligned vectors), else 1.
hipError_t launch_plan_f32(const PlanArgs& a, int vec, hipStream_t stream);
// what the planned launchers decide for a plan's n_tiny tiny tasks (spmm_impl.h own_tiny_launch): true = a launch of their own
bool plan_own_tiny_launch(int n_tiny, int fused);
hipError_t launch_window_f32(const WindowArgs& a, int vec, hipStream_t stream);
hipError_t launch_plan_f16(const PlanArgs& a, int vec, hipStream_t stream);
hipError_t launch_window_f16(const WindowArgs& a, int vec, hipStream_t stream);
hipError_t launch_plan_bf16(const PlanArgs& a, int vec, hipStream_t stream);
hipError_t launch_window_bf16(const WindowArgs& a, int vec, hipStream_t stream);
// the weighted forms (same vec contract)
hipError_t launch_plan_w_f32(const WPlanArgs& a, int vec, hipStream_t stream);
hipError_t launch_window_w_f32(const WWindowArgs& a, int vec, hipStream_t stream);
hipError_t launch_plan_w_f16(const WPlanArgs& a, int vec, hipStream_t stream);
hipError_t launch_window_w_f16(const WWindowArgs& a, int vec, hipStream_t stream);
hipError_t launch_plan_w_bf16(const WPlanArgs& a, int vec, hipStream_t stream);
hipError_t launch_window_w_bf16(const WWindowArgs& a, int vec, hipStream_t stream);
// 8-bit e4m3fn codes in, fp32 out (vec: 8 for D >= 32, else 4; D, strides and bases on the dword grid)
hipError_t launch_plan_f8(const PlanArgs& a, int vec, hipStream_t stream);
hipError_t launch_window_f8(const WindowArgs& a, int vec, hipStream_t stream);
hipError_t launch_plan_w_f8(const WPlanArgs& a, int vec, hipStream_t stream);
hipError_t launch_window_w_f8(const WWindowArgs& a, int vec, hipStream_t stream);
// per-row quantiser (quantize_fp8.hip): s[r] = amax_r / 448 (or scale_in[r]), q = rne_e4m3(clamp(x / s[r], -448, 448))
hipError_t launch_quantize_fp8(const float* X, long long rows, long long ldx, int D, const float* scale_in, unsigned char* Xq,
                               long long ldq, float* scale_out, hipStream_t stream);
// the multi-head weighted forms (spmm_weighted_heads_impl.h): values [heads][E], column c takes head c / dh's.  Entry e of
// head h weighs values[h * E + e] (direct: vindex == nullptr; spmm_weighted_heads.hip, hcspmm_forward_weighted_heads) or
// values[h * E + vindex[e]] (indexed; spmm_weighted_indexed.hip, hcspmm_forward_weighted_indexed).  fp32 only
struct WHPlanArgs {
  WPlanArgs w;
  long long E;        // values per head slice of w.values
  int dh;             // columns per head
  const int* vindex;  // [entries], or nullptr for the direct form
};
struct WHWindowArgs {
  WWindowArgs w;
  long long E;
  int dh;
  const int* vindex;
};
// direct form (a.vindex == nullptr): vec 4 only, dh % 4 == 0, D % dh == 0
hipError_t launch_plan_wh_f32(const WHPlanArgs& a, int vec, hipStream_t stream);
hipError_t launch_window_wh_f32(const WHWindowArgs& a, int vec, hipStream_t stream);
// indexed form (a.vindex set): vec 4 with the direct form's rules, or one head (dh = D) with any vec launch_plan_w_f32 takes
hipError_t launch_plan_wi_f32(const WHPlanArgs& a, int vec, hipStream_t stream);
hipError_t launch_window_wi_f32(const WHWindowArgs& a, int vec, hipStream_t stream);
// values[e] = 1/sqrt(deg(row e) * deg(col e)) (kind 0) or 1/deg(row e) (kind 1), deg = row length
hipError_t launch_edge_norm(const int* rowptr, const int* col, int N, long long E, int kind, float* values, hipStream_t stream);

// dW[D x H] = A^T * B (A: N x D rows lda apart, B: N x H rows ldb apart); `partial` holds
// weight_grad_groups(N) * D * H floats.  Shapes: weight_grad_supported(D, H).
bool weight_grad_supported(int D, int H);
int weight_grad_groups(long long N);
hipError_t launch_weight_grad(const float* A, long long lda, const float* B, long long ldb, float* out, float* partial,
                              long long N, int D, int H, hipStream_t stream);

// out[N x H] = in[N x D] * W (D x H, element strides ldr / ldc), fp32 MFMA.  tile_list (device, n_tiles ids of
// 16-row tiles) restricts the product to those tiles (the windows a fused launch has not already multiplied);
// nullptr = every tile.
hipError_t launch_dense_update(const float* in, const float* W, long long ldr, long long ldc, float* out, int N,
                               int D, int H, const int* tile_list, int n_tiles, hipStream_t stream);
// Row-tile form of the fused operators (fused_rows.hip): persistent launches that sum 16 tasks (or one dense window) at a
// time, write out2 and multiply the tile by the weights before it leaves the CU.  a: as for launch_plan_f32 with vec = 4
// (n_wide / panel_cols from wide_choice; needs panel_cols >= D); the hybrid launch with a.fused = 2 (sliced and wide tasks
// only + fix-up pass) follows.  fused_tiles_supported: the (D, H) shapes.
bool fused_tiles_supported(int D, int H);
hipError_t launch_fused_tiles(const PlanArgs& a, hipStream_t stream);
// out rows of the sparse-path rows that launch does not cover -- whole rows among the n_wide longest tasks, split rows
// (fix-up list), column-sliced rows that fell into one piece -- read from `in` (= out2, after the fix-up pass).
// Shapes: dense_update_streams(in, out, D, H).
hipError_t launch_dense_update_leftover(const float* in, const float* W, long long ldr, long long ldc, float* out, int N,
                                        int D, int H, const int* plan, int off_tasks, int n_wide, int off_fixups,
                                        int n_split_rows, int off_slice_tasks, int n_slice_tasks, hipStream_t stream);
// true when launch_dense_update takes the LDS-staged streaming kernel for this shape (the shapes the single-launch
// fused dense-tile epilogue is built for as well)
bool dense_update_streams(const float* in, const float* out, int D, int H);

// SDDMM and edge softmax (sddmm.hip; include/hcspmm.h hcspmm_sddmm, hcspmm_edge_softmax*): the kernels that produce and
// differentiate edge values.  out[e] = <A[row(e)], B[col(e)]> in fp32 for e in [0, E), A and B of one element type.
struct SddmmArgs {
  const void* A;  // [N][lda]: row r of A pairs with the entries of CSR row r
  const void* B;  // [b_rows][ldb]: indexed by column ids
  size_t lda, ldb;
  const int* rowptr;  // [N + 1]
  const int* col;     // [E]
  float* out;         // [E]
  int N, D;
  long long E;
};
// vec: as for launch_plan_* (pick_vec with A and B in the places of X and Z)
hipError_t launch_sddmm_f32(const SddmmArgs& a, int vec, hipStream_t stream);
hipError_t launch_sddmm_f16(const SddmmArgs& a, int vec, hipStream_t stream);
hipError_t launch_sddmm_bf16(const SddmmArgs& a, int vec, hipStream_t stream);
// multi-head SDDMM (sddmm_heads.hip, hcspmm_sddmm_heads): out[h*E + e] = <A[row(e)][h*D : (h+1)*D], B[col(e)][h*D : (h+1)*D]>
// for h < heads, a.D = columns per head; fp32, vec as pick_vec gives for one head's column slice
hipError_t launch_sddmm_heads_f32(const SddmmArgs& a, int heads, int vec, hipStream_t stream);
// per row r and head h, over the head-major [heads][E] arrays:
//   forward  out = softmax(x) over the row's entries;  backward  out = x * (y - sum_row x * y)  (x = alpha, y = grad_alpha)
struct SoftmaxArgs {
  const float* x;  // forward: logits; backward: alpha
  const float* y;  // backward: grad_alpha (forward: unused)
  float* out;      // forward: alpha; backward: grad_logits
  const int* rowptr;
  int N, heads;
  long long E;
};
hipError_t launch_edge_softmax(const SoftmaxArgs& a, bool backward, hipStream_t stream);

// GAT attention (gat_attention.hip; include/hcspmm.h hcspmm_gat_attention*): scores node-major [rows][heads], per-entry
// arrays head-major [heads][E].
//   forward   out = softmax over the row of LeakyReLU(s_dst[r] + s_src[col[e]])  (alpha)
//   backward  out = g (the gradient of the scores' sum z), grad_s_dst = row sums of g, grad_s_src = row sums of g[perm]
struct GatArgs {
  const float* s_dst;       // [N][heads]
  const float* s_src;       // [src_rows][heads] (backward: src_rows = N)
  const float* alpha;       // backward: [heads][E]
  const float* grad_alpha;  // backward: [heads][E]
  const int* rowptr;        // [N + 1]
  const int* col;           // [E]
  const int* perm;          // backward: [E], hcspmm_transpose_permutation's or hcspmm_transpose_graph's entry_index_t
  float* out;               // forward: alpha; backward: g
  float* grad_s_dst;        // backward: [N][heads]
  float* grad_s_src;        // backward: [n_t][heads]
  float slope;
  int N, heads;
  long long E;
  // backward, column side: the rows of A^T and, per entry of A^T, its position in A (perm).  The pattern-symmetric entry point
  // passes A's own row pointers and N
  const int* rowptr_t;      // [n_t + 1]
  int n_t;
};
hipError_t launch_gat_attention(const GatArgs& a, hipStream_t stream);
hipError_t launch_gat_attention_backward(const GatArgs& a, hipStream_t stream);

// GATv2 attention logits and their backward (gatv2_attention.hip; include/hcspmm.h hcspmm_gatv2_scores*), fp32:
//   forward   out[h*E + e] = sum_k att[h][k] * LeakyReLU(H_dst[row(e)][h*Dh + k] + H_src[col(e)][h*Dh + k]),  Dh = D / heads
//   backward  grad_dst / grad_src / grad_att from g = the gradient of out; partial holds gatv2_grad_blocks(N, D) * D floats
struct Gatv2Args {
  const float* H_dst;  // [N][ld_dst]
  const float* H_src;  // [src_rows][ld_src] (backward: src_rows = N)
  const float* att;    // [heads][Dh]
  const float* g;      // backward: [heads][E]
  const int* rowptr;   // [N + 1]
  const int* col;      // [E]
  const int* perm;     // backward: [E], hcspmm_transpose_permutation's or hcspmm_transpose_graph's entry_index_t
  float* out;          // forward: [heads][E]
  float* grad_dst;     // backward: [N][ld_gdst]
  float* grad_src;     // backward: [N][ld_gsrc]
  float* grad_att;     // backward: [heads][Dh]
  float* partial;      // backward: the workgroups' [D] partials of grad_att
  size_t ld_dst, ld_src, ld_gdst, ld_gsrc;
  float slope;
  int N, D, heads;
  long long E;
  // backward, grad_src side: A^T's rows and column ids (the rows of A) and, per entry of A^T, its position in A (perm).  The
  // pattern-symmetric entry point passes A's own arrays and N
  const int* rowptr_t;  // [n_t + 1]
  const int* col_t;     // [E]
  int n_t;
};
long long gatv2_grad_blocks(long long N, int D);
hipError_t launch_gatv2_scores(const Gatv2Args& a, hipStream_t stream);
hipError_t launch_gatv2_backward(const Gatv2Args& a, hipStream_t stream);

// Max / min aggregation and its backward (spmm_extremum.hip; include/hcspmm.h hcspmm_forward_extremum*), fp32.  p as for
// launch_plan_f32 (forward: X, Z; backward: X = grad_Z, Z = grad_X, ldx = its row stride), or p.plan == nullptr for the
// plan-free launch (then only X, Z, col, ldx, ldz, N, D are read).  Forward: partial = the fp32 values of the split rows'
// partial slots, ppos = their positions (n_partials x D each); backward: partial = fp32 sums of the split rows.
struct XArgs {
  PlanArgs p;
  const int* rowptr;  // [N + 1]
  int segment_len;    // plan header: entries per segment of a split row
  unsigned flip;      // forward: 0 = max, 0x80000000 = min (max of the negated values)
  int* arg;           // forward: [N][ldarg] winning entries, or nullptr
  int* ppos;          // forward: positions of the partial slots
  const int* garg;    // backward: the forward's arg, [N][ldarg]
  const int* perm;    // backward: [E] hcspmm_transpose_permutation
  size_t ldarg;
};
// vec: 4 (D >= 4), 2 or 1, as pick_vec gives for fp32
hipError_t launch_extremum_f32(const XArgs& a, int vec, hipStream_t stream);
hipError_t launch_extremum_backward_f32(const XArgs& a, int vec, hipStream_t stream);

// Sum, sum of squares, max and min of each row's neighbours in one gather pass (spmm_multi.hip; include/hcspmm.h
// hcspmm_forward_multi), fp32.  p as for launch_extremum_f32 with p.Z unused: the six outputs below share the row stride p.ldz
// (values) / ldarg (positions), and a null one is not written.  p.partial = six areas of `area` floats each -- sum, sum of
// squares, max, its position, min, its position of every partial slot (n_partials x D per area).
struct MArgs {
  PlanArgs p;
  const int* rowptr;  // [N + 1]
  int segment_len;    // plan header: entries per segment of a split row
  float *zsum, *zsumsq, *zmax, *zmin;
  int *amax, *amin;
  size_t ldarg;
  size_t area;        // floats per workspace area
};
// vec: 4 (D >= 4), 2 or 1, as pick_vec gives for fp32
hipError_t launch_multi_f32(const MArgs& a, int vec, hipStream_t stream);

// Per-channel softmax aggregation (spmm_softmax.hip; include/hcspmm.h hcspmm_forward_softmax), fp32.  p as for launch_multi_f32
// with p.Z unused: the outputs below share the row stride p.ldz, z is required and a null m / l / q is not written.
// p.partial = four areas of `area` floats each -- m, l, a, q of every partial slot (n_partials x D per area).
struct SArgs {
  PlanArgs p;
  const int* rowptr;  // [N + 1]
  int segment_len;    // plan header: entries per segment of a split row
  const float* beta;  // [D]
  float *z, *m, *l, *q;
  size_t area;        // floats per workspace area
};
// vec: 4 (D >= 4), 2 or 1, as pick_vec gives for fp32
hipError_t launch_softmax_f32(const SArgs& a, int vec, hipStream_t stream);
// its gradient with respect to X (softmax_aggr_grad.hip, hcspmm_softmax_backward), a plain-sum launch on the graph the backward
// walks: row j sums exp(beta x_j - M_i) / L_i * G_i * (1 + beta (x_j - Z_i)) over its entries (j, i).  p as for
// launch_edge_messages_f32 with p.X = X (the tasks' OWN rows, N of them, stride p.ldx) and p.Z = grad_X; G, Z, M, L are gathered
// through the column ids and share the row stride ld_in; partial = fp32 sums of the split rows.
struct SGradArgs {
  PlanArgs p;
  const int* rowptr;  // [N + 1]
  int segment_len;    // plan header: entries per segment of a split row
  const float* beta;  // [D]
  const float *G, *Zf, *M, *L;
  size_t ld_in;
};
hipError_t launch_softmax_backward_f32(const SGradArgs& a, int vec, hipStream_t stream);

// Edge-feature messages (spmm_edge_messages.hip; include/hcspmm.h hcspmm_forward_edge_messages), fp32: Z[r] = sum over the entries
// e of row r of m(X[col(e)], F[fi(e)]), fi(e) = findex ? findex[e] : e.  p as for launch_extremum_f32 (p.plan == nullptr: plan-free;
// p.X may be null for the copy op); partial = fp32 sums of the split rows.
struct EdgeMsgArgs {
  PlanArgs p;
  const int* rowptr;  // [N + 1]
  int segment_len;    // plan header: entries per segment of a split row
  int op;             // HCSPMM_EDGE_OP_*
  const float* F;     // [f_rows][ldf]
  size_t ldf;
  const int* findex;  // [E], or nullptr for the direct form
};
hipError_t launch_edge_messages_f32(const EdgeMsgArgs& a, int vec, hipStream_t stream);
// its gradient with respect to F (edge_messages_grad.hip, hcspmm_edge_messages_grad): gF[e] from gZ[row(e)], X[col(e)] and F[e]
struct EdgeMsgGradArgs {
  const float* gZ;  // [N][ldg]
  const float* X;   // [x_rows][ldx] (copy: unused)
  const float* F;   // [E][ldf] (add_relu only)
  float* gF;        // [E][ldgf]
  size_t ldg, ldx, ldf, ldgf;
  const int* rowptr;  // [N + 1]
  const int* col;     // [E]
  int N, D, op;
  long long E;
};
hipError_t launch_edge_messages_grad_f32(const EdgeMsgGradArgs& a, int vec, hipStream_t stream);

// Gated neighbour aggregation (spmm_gated.hip; include/hcspmm.h hcspmm_forward_gated), fp32: with z = fl(P[r] + Q[col(e)]),
// Z_gate[r] = sum over the entries e of row r of sigma(z) * V[col(e)] and Z_dgate[r] the same sum with sigma'(z).  p as for
// launch_softmax_backward_f32 with p.X unused: P holds the tasks' OWN rows (N of them), Q and V are gathered through the column
// ids.  outputs: bit 0 = Z_gate, bit 1 = Z_dgate.  p.Z / p.partial take the first output that is asked for; with both, z2 and
// the workspace area `area` floats behind p.partial take Z_dgate (same row stride p.ldz).
struct GatedArgs {
  PlanArgs p;
  const int* rowptr;  // [N + 1]
  int segment_len;    // plan header: entries per segment of a split row
  int outputs;
  const float *P, *Q, *V;
  size_t ldp, ldq, ldv;
  float* z2;
  size_t area;        // floats per workspace area
};
// vec: 4 (D >= 4), 2 or 1, as pick_vec gives for fp32
hipError_t launch_gated_f32(const GatedArgs& a, int vec, hipStream_t stream);


}  // namespace hcspmm
