/*
 * hcspmm.h -- C ABI of libhcspmm.so: MI355X-native (gfx950) hybrid SpMM for GNN
 * aggregation, the drop-in for the hot path of ZJU-DAILY/HC-SpMM.
 *
 * Every entry point names the reference interface it replaces (file:line under
 * the reference tree; "K.cu" = hybrid_kernel/hybrid_all_kernel.cu, "B.cpp" =
 * hybrid_kernel/hybrid_all.cpp).  The ABI is plain C: raw pointers, sizes and a
 * HIP stream; no torch types, no exceptions, no global mutable state (this describes the C ABI: the two Python-visible
 * front-ends above it each keep a process-wide, weakly-referencing registry of the plans they made).  All
 * functions return HCSPMM_OK (0) or a negative code; hcspmm_strerror() names it.
 *
 * Pointer naming: *_h = host memory, *_d = device (HBM) memory.
 * Index arrays are int32 (reference: dataset.py:102-103, K.cu:439-443); features
 * are fp32 row-major (hcspmm_forward_typed also takes fp16 / bf16).  A is binary in every entry point
 * the reference has: their edge values are never read.  hcspmm_forward_weighted is
 * the edge-weighted product Z = A_w * X on the same graph tensors and plans, with an fp32 value per
 * stored entry (normalised GCN / GraphSAGE-mean aggregation, edge-weighted graphs).
 */
#ifndef HCSPMM_H
#define HCSPMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 = the signatures below.  Entry points ADDED since 3 was introduced leave it unchanged (a consumer built against an older header keeps
 * working): hcspmm_loi_reorder_fast, hcspmm_dense_update (round 4); hcspmm_forward_weighted, hcspmm_edge_norm_device,
 * hcspmm_transpose_permutation (round 5); hcspmm_sddmm, hcspmm_edge_softmax, hcspmm_edge_softmax_backward (round 6); hcspmm_gat_attention,
 * hcspmm_gat_attention_backward (round 7); hcspmm_forward_weighted_heads, hcspmm_sddmm_heads (round 8); hcspmm_extremum_workspace_bytes,
 * hcspmm_forward_extremum, hcspmm_forward_extremum_backward (round 9); hcspmm_gatv2_scores, hcspmm_gatv2_backward_workspace_bytes,
 * hcspmm_gatv2_scores_backward (round 10); hcspmm_quantize_fp8, hcspmm_forward_fp8,
 * hcspmm_wide_threshold_fp8 (round 13); hcspmm_forward_edge_messages, hcspmm_edge_messages_grad (round 14);
 * hcspmm_multi_workspace_bytes, hcspmm_forward_multi (round 15); hcspmm_softmax_workspace_bytes, hcspmm_forward_softmax,
 * hcspmm_softmax_backward (round 17); hcspmm_sample_workspace_bytes, hcspmm_sample_row_pointers_device,
 * hcspmm_sample_neighbors_device, hcspmm_transpose_graph_device_workspace_bytes, hcspmm_transpose_graph_device (round 19);
 * hcspmm_gated_workspace_bytes, hcspmm_forward_gated (round 22).
 * HCSPMM_RULE_MI355X as the front-ends' default classifier is a front-end
 * matter: every C entry point that classifies takes its rule as an argument. */
#define HCSPMM_ABI_VERSION 3

/* Row-window geometry: hybrid_kernel/config.h:4-5 (BLK_H 16, BLK_W 8). */
#define HCSPMM_BLK_H 16
#define HCSPMM_BLK_W 8

/* return codes */
#define HCSPMM_OK 0
#define HCSPMM_EINVAL (-1)     /* bad argument (null pointer, negative size, D <= 0, a column id outside [0, num_columns), ...) */
#define HCSPMM_ENOMEM (-2)     /* host allocation failed */
#define HCSPMM_EPLAN (-3)      /* plan blob does not match this graph (magic, version, N, E, section bounds, fingerprint) */
#define HCSPMM_EHIP (-4)       /* a HIP runtime call or kernel launch failed (hcspmm_last_hip_error) */
#define HCSPMM_EWORKSPACE (-5) /* workspace smaller than hcspmm_workspace_bytes() */
#define HCSPMM_ERANGE (-6)     /* a size exceeds what the int32 index contract can address */

/* Window classifier rule. */
#define HCSPMM_RULE_INTENDED 0       /* logit > 0 -> sparse-row(0) else dense-tile(1); paper p.7, K.cu:261 w/o guard */
#define HCSPMM_RULE_INTENDED_GUARD 1 /* K.cu:261 literally: size > 32 || logit > 0 -> 0 */
#define HCSPMM_RULE_AS_SHIPPED 2     /* K.cu:262 literally: float used as bool */
#define HCSPMM_RULE_MI355X 3         /* same two features, coefficients refit on MI355X with the paper's procedure
                                        against THIS library's two sub-paths (tools/refit_classifier.py,
                                        profiles/r01/classifier_refit_v3.json) at embedding width 32: for
                                        narrow embeddings (D < 64); not a reference output */
#define HCSPMM_RULE_MI355X_WIDE 4    /* the same refit at embedding width 128: for D >= 64 (preprocess does not
                                        know D -- the reference's signature has none -- so the caller picks) */

const char* hcspmm_strerror(int code);
int hcspmm_abi_version(void);
/* hipError_t (as int) of the most recent failing HIP call on this thread, 0 if none. */
int hcspmm_last_hip_error(void);

/* ------------------------------------------------------------------------------------------
 * preprocess (host).  Replaces `preprocess` K.cu:339-408 (binding B.cpp:13-17, :501) and its
 * kernels fill_edgeToRow K.cu:314-326, fill_segment K.cu:289-301, thrust::sort K.cu:386-399,
 * generate_edgetocolumn K.cu:242-269.  Integer outputs are bit-exact with the reference
 * algorithm (Appendix A of SURVEY.md); empty windows get blockPartition = hybrid_type = 0.
 *   row_pointers_h[N+1], column_index_h[E] : CSR, columns ascending & unique within a row
 *   num_columns : rows of the matrix the column ids index (the reference's graphs are square: pass num_nodes, or
 *                 <= 0 for the same); a multi-GPU row block passes the height of the gathered embedding matrix.
 *                 Every column id is checked against [0, num_columns) -- HCSPMM_EINVAL otherwise -- so that a
 *                 malformed CSR is an error here instead of an out-of-bounds gather on the GPU (the reference
 *                 checks nothing).
 *   blockPartition_h[W], hybrid_type_h[W], edgeToColumn_h[E], edgeToRow_h[E] : outputs, W = ceil(N/16)
 *   num_threads <= 0 : HCSPMM_THREADS if set, else min(64, host hardware threads); the outputs do not depend on it.
 *   edgeToRow_h may be NULL (not produced): it is the plain CSR row expansion, which a caller whose
 *   graph lives in HBM can generate there without a host round trip.
 * ---------------------------------------------------------------------------------------- */
int hcspmm_preprocess_host(const int32_t* row_pointers_h, const int32_t* column_index_h, int64_t num_nodes,
                           int64_t num_edges, int64_t num_columns, int rule, int num_threads,
                           int32_t* blockPartition_h, int32_t* edgeToColumn_h, int32_t* edgeToRow_h,
                           int32_t* hybrid_type_h);

/* edgeToRow on the device: edgeToRow_d[e] = the row that owns stored entry e (the plain CSR row expansion).  Replaces
 * fill_edgeToRow K.cu:314-337 for callers whose graph already lives in HBM (hcspmm_preprocess_host then gets
 * edgeToRow_h = NULL): one thread per entry, a binary search in row_pointers (which sits in L2).  Rows without
 * entries are skipped correctly.  Asynchronous on `stream`. */
int hcspmm_edge_to_row_device(const int32_t* row_pointers_d, int64_t num_nodes, int64_t num_edges, int32_t* edgeToRow_d,
                              void* stream);

/* ------------------------------------------------------------------------------------------
 * Launch plan (host build, device resident).  New on MI355X: the reference branches per thread
 * block on hybrid_type (K.cu:960,1039) with one block per window; here the host turns the
 * classified windows into (a) sparse-row tasks ordered by power-of-two length class (row order inside a
 * class), long rows split into segments, and
 * (b) packed dense-tile windows (sorted unique columns + 0/1 tile masks in MFMA lane order).
 * The blob travels in the reference's reserved `row_nzr` tensor slot (K.cu:405: row_nzr/col_nzr
 * are [0] placeholders that every forward receives and never reads).
 *
 * The first HCSPMM_PLAN_HEADER_WORDS int32 words of the blob are a hcspmm_plan_header; callers
 * keep a host copy of it (hcspmm_forward needs the counts to size its grid without a device
 * read-back).
 * ---------------------------------------------------------------------------------------- */
#define HCSPMM_PLAN_MAGIC 0x48435350 /* "HCSP" */
#define HCSPMM_PLAN_VERSION 8
#define HCSPMM_TINY_LEN 2 /* tasks of at most this many entries carry their indices in the descriptor */
#define HCSPMM_COMPACT_K 40     /* dense windows of at most this many (padded) columns use compact records ... */
#define HCSPMM_COMPACT_WORDS 64 /* ... of this many words: [window, K/4, U[40], 10 x (mask lo, mask hi), pad] */
#define HCSPMM_COMPACT2_K 80    /* wider windows up to this many (padded) columns use double records ... */
#define HCSPMM_COMPACT2_WORDS 128 /* ... of this many words: [window, K/4, U[80], 20 x (mask lo, mask hi), pad] */
#define HCSPMM_PLAN_HEADER_WORDS 64
#define HCSPMM_SCHED_INDEX_WORDS 32 /* a first-index record of the schedule copies: one 128-byte line (off_task_sched_idx) */

typedef struct hcspmm_plan_header {
  int32_t magic;            /* HCSPMM_PLAN_MAGIC */
  int32_t version;          /* HCSPMM_PLAN_VERSION */
  int32_t total_words;      /* size of the whole blob in int32 words */
  int32_t num_nodes;        /* N the plan was built for */
  int32_t num_edges;        /* E the plan was built for */
  int32_t num_windows;      /* W */
  int32_t split_threshold;  /* rows with more entries than this are split ... */
  int32_t segment_len;      /* ... into segments of this many entries */
  int32_t n_tasks;          /* sparse-row tasks (one per whole row or row segment), by descending power-of-two length class,
                               rows ascending inside a class (off_task_sched: the same in exact length order) */
  int32_t n_dense;          /* dense-tile windows */
  int32_t n_split_rows;     /* rows whose partial sums are combined by the fix-up pass */
  int32_t n_partials;       /* partial-sum slots (rows of the workspace) */
  int32_t off_tasks;        /* word offsets of the sections inside the blob */
  int32_t off_dense_index;
  int32_t off_dense_pack;
  int32_t off_fixups;
  int32_t nnz_sparse;       /* entries handled by the sparse-row path */
  int32_t nnz_dense;        /* entries handled by the dense-tile path */
  int32_t uniq_dense;       /* sum of unique columns over dense windows (gathered X rows) */
  int32_t max_dense_k;      /* largest padded K (8*blockPartition) among dense windows */
  int32_t n_len_gt[5];      /* tasks longer than 16, 32, 64, 128, 256 entries (class boundaries are powers
                               of two, so these are prefix sizes of the task list: the launch can hand the n longest tasks to
                               whole waves -- "wide" tasks -- at any of these thresholds) */
  int32_t n_tiny;           /* the last n_tiny tasks have at most HCSPMM_TINY_LEN entries and carry their column indices
                               inline: (row, or -(slot+1) for a row segment | index0 | length | index1), absent = -1 */
  int32_t n_dense_compact;  /* the last n_dense_compact dense windows have K <= HCSPMM_COMPACT_K and live in fixed
                               HCSPMM_COMPACT_WORDS-word records: [window, K/4, U[40], 10 x (mask lo, mask hi), pad] */
  int32_t off_dense_compact; /* word offset of those records (a multiple of 64) */
  int32_t n_dense_compact2; /* the n_dense_compact2 dense windows before them have HCSPMM_COMPACT_K < K <= HCSPMM_COMPACT2_K
                               and live in HCSPMM_COMPACT2_WORDS-word records of the same layout (U[80], 20 masks) */
  int32_t off_dense_compact2; /* word offset of those records (a multiple of 64) */
  int32_t num_columns;      /* rows of X this plan gathers from: every column id it holds or refers to is < this */
  int32_t n_sparse_windows; /* row windows NOT on the dense-tile path (sparse-row and empty ones), ... */
  int32_t off_sparse_windows; /* ... their ids, ascending: the 16-row tiles the update pass of
                               hcspmm_forward_fused still has to multiply by the weights */
  uint32_t fingerprint_lo;  /* hcspmm_graph_fingerprint_host(row_pointers, column_index) of the graph the plan was */
  uint32_t fingerprint_hi;  /* built from: a plan for another graph with the same N and E is told apart by it */
  int32_t dense_k_sum;      /* sum over dense windows of K = 8*blockPartition (padded condensed columns): the
                               dense-tile path executes exactly 2*16*K*D flop per window */
  int32_t flags;            /* HCSPMM_PLAN_FUSE_IN_LAUNCH: the fused operators update this plan's dense-tile windows inside the
                               hybrid launch (hcspmm_plan_params.fuse_in_launch) */
  /* XCD-affine column slices: sparse-path rows longer than slice_threshold are cut where their
   * (ascending) column ids cross n_slices - 1 boundaries and every segment_len entries; the pieces of slice s form
   * their own task list, served only by workgroups with blockIdx % 8 == s % 8 -- workgroups that share one of the
   * eight per-XCD L2s -- so that L2 holds 1/8 of the X rows those tasks gather.  Placement is a speed matter only. */
  int32_t n_slices;         /* 0: none; else a multiple of 8 */
  int32_t slice_threshold;  /* rows with more entries than this are sliced (when n_slices > 0) */
  int32_t off_slice_table;  /* n_slices + 1 task offsets relative to off_slice_tasks, each a multiple of 64: slice s
                               owns descriptors [table[s], table[s+1]), longest length class first, padded with
                               (-1, 0, 0, -1) */
  int32_t off_slice_tasks;  /* descriptors (row, first entry, length, partial slot or -1), as the ordinary tasks */
  int32_t n_slice_tasks;    /* = table[n_slices], padding included */
  int32_t slice_xcd_tasks;  /* max over x in [0, 8) of the descriptors of the slices s = x (mod 8): sizes the region */
  int32_t nnz_sliced;       /* entries covered by sliced tasks (part of nnz_sparse) */
  int32_t n_sliced_rows;
  int32_t panel_cols;       /* hcspmm_plan_params.panel_cols: 0 = the launch chooses, > 0: feature columns per
                               sparse pass for fp32 features (16-bit features: twice as many), < 0: one pass over all columns */
  /* Schedule copies: the same descriptors in exact descending length order, equal lengths in the order of
   * the list they were copied from, so that the lane groups of a wave end together.  The binary product's launch reads them
   * in place of the lists above.  Built when num_columns <= 2 097 152 (one 128-byte line per X row fits the Infinity Cache:
   * measured a gain at 233 K columns and a loss at 4.86 M and 16 M, where the lost row order costs L2 hits; the boundary between
   * them is not measured); HCSPMM_TASK_SCHEDULE=0 / 1 in the
   * environment at plan build forces them off / on.  Both offsets are 0 when absent. */
  int32_t off_task_sched;   /* n_tasks - n_tiny descriptors: the non-tiny prefix of the task list.  Its first n_len_gt[b]
                               are still exactly the tasks longer than 16 << b.  0: absent */
  int32_t off_slice_sched;  /* n_slice_tasks descriptors under the same slice table: every list's real descriptors in that
                               order, its padding behind them.  0: absent (always when n_slices == 0) */
  /* First-index records of the schedule copies: one record of HCSPMM_SCHED_INDEX_WORDS int32 (128 bytes, 128-byte
   * aligned inside the blob) per descriptor of a schedule copy, in the copy's order.  Record i holds
   * column_index[first, first + min(length, 32)) of descriptor i, the rest -1; a padding descriptor's record is all -1.  A wave of
   * the binary product's launch knows its records' address from its position in the grid alone, so it asks for them together
   * with its descriptors instead of one memory round trip later.  Built with the schedule copies unless HCSPMM_SCHED_INDEX=0 is in
   * the environment at plan build.  Both offsets are multiples of 32 words and 0 when absent; plans without them run as before. */
  int32_t off_task_sched_idx;  /* n_tasks - n_tiny records, behind the schedule copies.  0: absent (always when off_task_sched == 0) */
  int32_t off_slice_sched_idx; /* n_slice_tasks records behind them.  0: absent (always when off_slice_sched == 0) */
  int32_t slice_table_copy[9]; /* with the records and n_slices == 8: the nine words at off_slice_table once more, so that a
                                  launcher -- which holds the header, not the blob -- can pass the table as kernel arguments;
                                  else 0 */
  int32_t reserved[5];
} hcspmm_plan_header;

#define HCSPMM_PLAN_FUSE_IN_LAUNCH 1
#define HCSPMM_PLAN_FUSE_ROWS 2 /* ... and the sparse-row path as well: the row-tile form (hcspmm_plan_params.fuse_in_launch = 2) */
#define HCSPMM_PLAN_FUSE_NEVER 4 /* always two launches (fuse_in_launch < 0); no flag = the operator chooses per call */

/* Tunables for the plan; zero-initialise for defaults. */
typedef struct hcspmm_plan_params {
  int32_t split_threshold; /* default 512 */
  int32_t segment_len;     /* default 256 */
  int32_t fuse_in_launch;  /* form of hcspmm_forward_fused for this plan (see there): 0 = chosen per call (row tiles when out2 --
                              N x D fp32 -- is 80 MB or more at D <= 64, or 256 MB or more at D <= 128, H <= 32 on a graph
                              with a quarter of its rows in dense-tile windows; else two launches), < 0 = always two launches, 1 = dense-tile
                              windows multiply by the weights inside the hybrid launch (slower on MI355X:
                              profiles/r02/ab_fused.log), 2 = row tiles wherever the shape allows */
  int32_t slice_threshold; /* XCD-affine column slices: 0 = automatic (on for num_columns >= 65536 when at least 5 % of
                              the sparse-path entries sit in rows longer than 256 entries and -- below 250 000 columns --
                              the sparse path holds at least 3 M entries; HCSPMM_SLICE_THRESHOLD in the environment
                              overrides), > 0: rows longer than this are sliced, < 0: off */
  int32_t n_slices;        /* 0 = 8 (HCSPMM_SLICES overrides); rounded up to a multiple of 8, at most 64 */
  int32_t panel_cols;      /* feature columns per pass of the sparse-row path: 0 = chosen at launch from the plan's counts and
                              the embedding width (32 fp32 columns = one cache line per gathered row for wide embeddings, 64
                              when X exceeds the Infinity Cache, one pass for short-row graphs), > 0: this many (a multiple
                              of 16; fp32 -- 16-bit features take twice as many), < 0: one pass.  The best value depends on
                              the graph's size and degree mix in no monotone way (profiles/r03/ab_panel_midsize.log): a
                              caller that will run many steps can measure it (hcspmm.tune_plan in the Python front-end) */
} hcspmm_plan_params;

/* Number of int32 words a plan for this graph needs (so the caller can allocate the tensor). */
int hcspmm_plan_words(const int32_t* row_pointers_h, int64_t num_nodes, int64_t num_edges,
                      const int32_t* blockPartition_h, const int32_t* hybrid_type_h,
                      const hcspmm_plan_params* params, int64_t* words_out);

/* Fill plan_h[words] (host).  The caller uploads it to HBM unchanged.  num_columns as for
 * hcspmm_preprocess_host (<= 0: num_nodes); column ids are range-checked here too (HCSPMM_EINVAL), since a plan
 * may be built for a classification that did not come from hcspmm_preprocess_host. */
int hcspmm_plan_build(const int32_t* row_pointers_h, const int32_t* column_index_h, int64_t num_nodes,
                      int64_t num_edges, int64_t num_columns, const int32_t* blockPartition_h,
                      const int32_t* edgeToColumn_h, const int32_t* hybrid_type_h, const hcspmm_plan_params* params,
                      int32_t* plan_h, int64_t words);

/* Validate a header against (N, E) and its own section layout (every section inside total_words, counts
 * consistent); plan_words_available = length of the buffer that holds the blob (<= 0: not checked).
 * HCSPMM_OK or HCSPMM_EPLAN. */
int hcspmm_plan_check(const hcspmm_plan_header* header_h, int64_t num_nodes, int64_t num_edges,
                      int64_t plan_words_available);

/* 64-bit fingerprint of a CSR graph: an order-independent sum of mixed (index, value) pairs over row_pointers
 * and column_index, so host threads and GPU waves can each add their share.  hcspmm_plan_build stores it in the
 * header; a binding that is handed a plan together with graph tensors it has not seen with that plan computes
 * the device variant once (one small kernel + an 8-byte read-back, then cached by the caller) and refuses a
 * mismatch with HCSPMM_EPLAN: a plan built for a different graph with the same N and E (e.g. the same graph
 * after a LOI reorder) would otherwise silently produce a wrong Z.
 *   fingerprint_out_d : 8-byte device buffer, overwritten (zeroed on `stream` first). */
int hcspmm_graph_fingerprint_host(const int32_t* row_pointers_h, const int32_t* column_index_h, int64_t num_nodes,
                                  int64_t num_edges, uint64_t* fingerprint_out_h);
int hcspmm_graph_fingerprint_device(const int32_t* row_pointers_d, const int32_t* column_index_d, int64_t num_nodes,
                                    int64_t num_edges, uint64_t* fingerprint_out_d, void* stream);

/* Bytes of device workspace hcspmm_forward* needs for this plan and embedding_dim (may be 0). */
size_t hcspmm_workspace_bytes(const hcspmm_plan_header* header_h, int embedding_dim);

/* Wide-task threshold hcspmm_forward will use for this plan and embedding_dim: sparse-path rows
 * (or row segments) with more entries than this are summed by a whole wave -- its 64/L lane groups
 * take alternate chunks and are combined by a fixed shuffle tree (deterministic, but not the
 * sequential CSR order); rows at or below it are summed strictly in CSR order by one lane group,
 * bit-identical to the reference's sparse-row loop (K.cu:1377-1380).  Small graphs get a small
 * threshold (latency-bound: the longest row's dependent-load chain is the kernel time), large
 * graphs a large one (throughput-bound).  Returns INT32_MAX when no task is wide.  header_h == NULL
 * asks about the plan-free kernel (fixed threshold of 64 entries). */
int32_t hcspmm_wide_threshold(const hcspmm_plan_header* header_h, int embedding_dim);

/* ------------------------------------------------------------------------------------------
 * forward: Z = A * X.  Replaces the launchers spmm_forward_plus K.cu:410, spmm_forward_plus_more :457,
 * spmm_forward_plus_fixed32 :500, spmm_forward_plus_fixed64 :553 (bindings B.cpp:194-308; Python names
 * forward / forward_more / forward_fixed32 / forward_fixed64 and the backward* aliases B.cpp:516-523) and
 * the kernels
 * spmm_forward_cuda_kernel_arbi_warps_hybrid_{adaptive,adaptive_more,32,64} K.cu:919-1637.
 * One entry point serves every embedding_dim (the fixed32/fixed64 variants are the same math).
 *
 *   X_d[N*D], Z_d[N*D]            fp32 row-major, Z fully overwritten
 *   row_pointers_d .. hybrid_type_d   the 7 graph tensors of the reference API (device)
 *   plan_d / plan_header_h        plan blob in HBM + host copy of its header, or both NULL:
 *                                 then the plan-free kernel runs (one workgroup per row window,
 *                                 branch on hybrid_type, as the reference does)
 *   workspace_d / workspace_bytes >= hcspmm_workspace_bytes(); may be NULL when that is 0
 *   stream                        hipStream_t (as void*); NULL = the null stream
 * Asynchronous: returns after enqueueing; no host-device synchronisation inside.
 * ---------------------------------------------------------------------------------------- */
int hcspmm_forward(const float* X_d, float* Z_d, const int32_t* row_pointers_d, const int32_t* column_index_d,
                   const int32_t* blockPartition_d, const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d,
                   const int32_t* hybrid_type_d, const int32_t* plan_d, const hcspmm_plan_header* plan_header_h,
                   int64_t num_nodes, int64_t num_edges, int embedding_dim, void* workspace_d,
                   size_t workspace_bytes, void* stream);

/* The same product on strided views: X rows are ldx elements apart, Z rows ldz (both >= embedding_dim),
 * so a column panel of a wider matrix can be read / written in place (the multi-GPU shard gathers X
 * panel by panel and writes each panel's product straight into its slice of Z).
 * x_rows = rows of X (hcspmm_forward: num_nodes -- the reference's graphs are square); with a plan, a launch
 * whose plan gathers beyond it (header num_columns > x_rows) is refused with HCSPMM_EINVAL.  The plan-free
 * kernel reads column_index as it is handed over, like the reference: its caller vouches for the range
 * (hcspmm_preprocess_host checked it when it produced the window tensors). */
int hcspmm_forward_strided(const float* X_d, int64_t x_rows, int64_t ldx, float* Z_d, int64_t ldz, const int32_t* row_pointers_d,
                           const int32_t* column_index_d, const int32_t* blockPartition_d,
                           const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d, const int32_t* hybrid_type_d,
                           const int32_t* plan_d, const hcspmm_plan_header* plan_header_h, int64_t num_nodes,
                           int64_t num_edges, int embedding_dim, void* workspace_d, size_t workspace_bytes,
                           void* stream);

/* Feature element types of hcspmm_forward_typed. */
#define HCSPMM_DTYPE_F32 0
#define HCSPMM_DTYPE_F16 1  /* IEEE binary16 */
#define HCSPMM_DTYPE_BF16 2 /* bfloat16 */

/* The same product for fp32, fp16 or bf16 features (the half-precision variants of the paper's Table VII, p.16;
 * the reference repository ships fp32 only).  X and Z hold `dtype` elements, ldx / ldz count elements.  16-bit
 * rows are gathered as stored (half the bytes of the fp32 path -- the launch is bound by exactly those bytes),
 * widened exactly, summed in fp32 in the same order as the fp32 path, and rounded once (to nearest even) per
 * output element:  Z = round_dtype(fp32 sum).  The workspace is fp32 whatever the dtype
 * (hcspmm_workspace_bytes).  dtype = HCSPMM_DTYPE_F32 is hcspmm_forward_strided. */
int hcspmm_forward_typed(const void* X_d, int64_t x_rows, int64_t ldx, void* Z_d, int64_t ldz, int dtype,
                         const int32_t* row_pointers_d, const int32_t* column_index_d,
                         const int32_t* blockPartition_d, const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d,
                         const int32_t* hybrid_type_d, const int32_t* plan_d, const hcspmm_plan_header* plan_header_h,
                         int64_t num_nodes, int64_t num_edges, int embedding_dim, void* workspace_d,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Edge-weighted forward: Z = A_w * X.  Arguments of hcspmm_forward_typed (strided X / Z, x_rows, rectangular blocks, all
 * three dtypes, with a plan or plan-free) plus
 *   values_d[E]  fp32, aligned with column_index: values_d[e] belongs to CSR entry e.  NULL is HCSPMM_EINVAL.
 *   Z[r][:] = sum over e in [row_pointers[r], row_pointers[r+1])  values[e] * X[column_index[e]][:]
 * Every step is acc = fmaf(values[e], x, acc), in the order hcspmm_forward_typed adds that row: CSR order on ordinary and
 * tiny tasks, ascending window columns on the dense-tile path (v_mfma_f32_16x16x4_f32 is a k-ordered fma chain; non-edges
 * contribute fmaf(0, x, acc)), the same fixed shuffle tree on wide tasks, the same slice / segment order through the fix-up
 * pass.  Hence values == 1 gives hcspmm_forward_typed's bits on every path, and exactly representable products give the
 * bits of a sequential fp32 sum.  16-bit features are widened, accumulated in fp32 and rounded once (RNE); values stay fp32.
 * The values are read on every call and never enter the plan: a caller may change them between calls (learned or attention
 * weights) without preprocessing again.  Separate kernels (spmm_weighted*.hip); the binary ones are untouched.
 * ---------------------------------------------------------------------------------------- */
int hcspmm_forward_weighted(const void* X_d, int64_t x_rows, int64_t ldx, void* Z_d, int64_t ldz, int dtype,
                            const int32_t* row_pointers_d, const int32_t* column_index_d, const int32_t* blockPartition_d,
                            const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d, const int32_t* hybrid_type_d,
                            const int32_t* plan_d, const hcspmm_plan_header* plan_header_h, int64_t num_nodes,
                            int64_t num_edges, int embedding_dim, void* workspace_d, size_t workspace_bytes, void* stream,
                            const float* values_d);

/* ------------------------------------------------------------------------------------------
 * 8-bit feature storage: node features kept as OCP e4m3fn codes with one fp32 scale per row, a quarter of the fp32 bytes
 * (a 128-column row is ONE 128-byte cache line), and the products that read them directly.
 *
 * Format.  `format` = HCSPMM_FP8_E4M3 only: OCP e4m3fn -- bias 7, largest finite value 448, no infinities, NaN codes 0x7f /
 * 0xff (torch.float8_e4m3fn; what gfx950's v_cvt_pk_f32_fp8 / v_cvt_pk_fp8_f32 convert).  Any other value is HCSPMM_EINVAL;
 * e5m2 and the MI300 `fnuz` encodings are not served.
 *
 * Shapes.  embedding_dim % 4 == 0, the row strides of the code matrix % 4 == 0 (elements are bytes) and a 4-byte aligned
 * code base: every row starts on a dword, the kernels read dword-aligned vectors and a lane whose columns would run past the
 * row is moved back onto its last ones.  Anything else is HCSPMM_EINVAL before any device call.
 *
 * hcspmm_quantize_fp8: X_d fp32 [rows][ldx] (ldx >= embedding_dim) -> Xq_d codes [rows][ldq] (ldq >= embedding_dim), scale_out_d
 * fp32 [rows].  For each row r:
 *   amax = max |x| over the row's finite entries;
 *   s[r] = amax / 448.0f (IEEE fp32 division); 1.0f when amax == 0 or the row has no finite entry; raised to 2^-126 when the
 *          quotient is not a normal number;
 *   code = rne_e4m3(clamp(x / s[r], -448, 448)) with an IEEE fp32 division: +-inf saturates to +-448, NaN gives the NaN code
 *          (0x7f with x's sign bit).
 * scale_in_d != NULL (fp32 [rows]) replaces the computed scales -- the clamp then does real work -- and is copied to
 * scale_out_d, which may then be NULL.  rows == 0 returns HCSPMM_OK without a launch.
 *
 * hcspmm_forward_fp8: Z = A_w * (diag(row_scale) * widen(Xq)), Z fp32 [num_nodes][ldz]:
 *   Z[i][:] = sum over e in row i of  w_e * widen(Xq[column_index[e]][:]),  w_e = values[e] * row_scale[column_index[e]]
 * w_e is ONE fp32 multiplication, rounded once; every step is acc = fmaf(w_e, x, acc) in fp32; widening e4m3 -> fp32 is exact.
 * On each sub-path the order is the one hcspmm_forward_weighted uses there: CSR order on ordinary and tiny tasks, ascending
 * window columns on dense tiles (v_mfma_f32_16x16x4_f32 on widened operands), the same shuffle tree and fix-up order.  A NULL
 * values_d or row_scale_d counts as 1; with both NULL the binary kernels' plain adds are used.  row_scale_d has x_rows entries.
 * The launch layout (column panels -- a cache line is 128 columns --, wide threshold: hcspmm_wide_threshold_fp8) depends on
 * the element size, so bit equality with hcspmm_forward_weighted on dequantised input is NOT promised in general; sums that
 * are exact in fp32 in any order are, of course, the same bits.  The graph, plan and header arguments, their checks and error
 * codes are hcspmm_forward_weighted's (with a plan or plan-free); the workspace is hcspmm_workspace_bytes (partials are fp32).
 * ---------------------------------------------------------------------------------------- */
#define HCSPMM_FP8_E4M3 0
int hcspmm_quantize_fp8(const float* X_d, int64_t rows, int64_t ldx, int embedding_dim, int format,
                        const float* scale_in_d /* nullable */, void* Xq_d, int64_t ldq, float* scale_out_d, void* stream);
int hcspmm_forward_fp8(const void* Xq_d, int64_t x_rows, int64_t ldx, int format, const float* row_scale_d /* nullable */,
                       const float* values_d /* nullable */, float* Z_d, int64_t ldz, const int32_t* row_pointers_d,
                       const int32_t* column_index_d, const int32_t* blockPartition_d, const int32_t* edgeToColumn_d,
                       const int32_t* edgeToRow_d, const int32_t* hybrid_type_d, const int32_t* plan_d,
                       const hcspmm_plan_header* plan_header_h, int64_t num_nodes, int64_t num_edges, int embedding_dim,
                       void* workspace_d, size_t workspace_bytes, void* stream);
/* hcspmm_wide_threshold for the 8-bit launch (8 codes per lane from 32 columns up, else 4); INT32_MAX for a width off the
 * 4-column grid */
int32_t hcspmm_wide_threshold_fp8(const hcspmm_plan_header* header_h, int embedding_dim);

/* Multi-head edge-weighted forward: hcspmm_forward_weighted for `heads` heads of Dh = embedding_dim / heads columns each,
 * in one launch.  values_d is head-major fp32 [heads][E] (head h's values are the slice [h * E, (h + 1) * E)):
 *   Z[r][h * Dh + j] = sum over e in row r  values[h * E + e] * X[column_index[e]][h * Dh + j]
 * Columns [h * Dh, (h + 1) * Dh) of Z are bit for bit hcspmm_forward_weighted(X, values + h * E) on the same graph, plan and
 * full width embedding_dim, restricted to those columns (equal up to the sign of a zero; values must be finite: a dense-tile
 * window covering several heads adds the other heads' finite products with zero to each column).  So heads = 1 is
 * hcspmm_forward_weighted, and values of 1 give hcspmm_forward_typed's bits.  One column-index load per entry serves every
 * head.  fp32 features only: HCSPMM_DTYPE_F16 / BF16 are HCSPMM_EINVAL.  heads >= 1, embedding_dim % heads == 0 and
 * Dh % 4 == 0, else HCSPMM_EINVAL; every other argument as for hcspmm_forward_weighted (NULL values is HCSPMM_EINVAL);
 * all argument errors are reported before any device call.  Plan and preprocessing are those of the binary product. */
int hcspmm_forward_weighted_heads(const void* X_d, int64_t x_rows, int64_t ldx, void* Z_d, int64_t ldz, int dtype,
                                  const int32_t* row_pointers_d, const int32_t* column_index_d, const int32_t* blockPartition_d,
                                  const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d, const int32_t* hybrid_type_d,
                                  const int32_t* plan_d, const hcspmm_plan_header* plan_header_h, int64_t num_nodes,
                                  int64_t num_edges, int embedding_dim, void* workspace_d, size_t workspace_bytes, void* stream,
                                  const float* values_d, int heads);

/* Multi-head edge-weighted forward with indexed values: hcspmm_forward_weighted_heads whose weight for entry e is fetched
 * through value_index_d[e].  values_d is head-major fp32 [heads][num_values]:
 *   Z[r][h * Dh + j] = sum over e in row r  values[h * num_values + value_index[e]] * X[column_index[e]][h * Dh + j]
 * The result is bit for bit hcspmm_forward_weighted_heads (heads = 1: hcspmm_forward_weighted) called with the gathered
 * values[:, value_index] -- the same fma chains, combine trees, MFMA order and fix-up order on every launch path (ordinary,
 * wide, column-sliced, segmented and tiny tasks, dense-tile windows, plan-free, rectangular x_rows) -- so an identity index
 * reproduces those entry points exactly.  It is what a backward through A^T wants: on the transposed graph
 * (hcspmm_transpose_graph) with value_index = entry_index_t, or on a pattern-symmetric graph with value_index =
 * hcspmm_transpose_permutation's perm, dX = A_w^T * dZ reads A's values in place and no permuted copy is written.
 * value_index_d is int32 [num_edges]; every index must lie in [0, num_values) and is trusted on the device, as column ids
 * are on the plan-free paths (many-to-one indices and num_values != num_edges are fine).  fp32 only.  heads >= 1,
 * embedding_dim % heads == 0 and Dh % 4 == 0; heads = 1 takes every embedding_dim hcspmm_forward_weighted serves.  NULL
 * values_d, a NULL value_index_d or num_values == 0 with num_edges > 0, num_values < 0 and the argument errors of
 * hcspmm_forward_weighted_heads are HCSPMM_EINVAL before any device call.  Separate kernels
 * (spmm_weighted_indexed.hip) on the binary product's plan. */
int hcspmm_forward_weighted_indexed(const void* X_d, int64_t x_rows, int64_t ldx, void* Z_d, int64_t ldz, int dtype,
                                    const int32_t* row_pointers_d, const int32_t* column_index_d, const int32_t* blockPartition_d,
                                    const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d, const int32_t* hybrid_type_d,
                                    const int32_t* plan_d, const hcspmm_plan_header* plan_header_h, int64_t num_nodes,
                                    int64_t num_edges, int embedding_dim, void* workspace_d, size_t workspace_bytes, void* stream,
                                    const float* values_d, int heads, const int32_t* value_index_d /* [E] */, int64_t num_values);

/* ------------------------------------------------------------------------------------------
 * Max / min neighbour aggregation with its argmax (GraphSAGE-pool, GIN-max, PNA; PyG aggr = "max" / "min"):
 *   Z[r][d]   = max (HCSPMM_REDUCE_MAX) or min (HCSPMM_REDUCE_MIN) over e in [row_pointers[r], row_pointers[r+1]) of
 *               X[column_index[e]][d]
 *   arg[r][d] = the CSR position e of the winning entry
 * The winner is exact and does not depend on how a row is split (lanes, wide tasks, column slices, segments, panels,
 * plan-free): ties go to the lowest e (-0.0 and +0.0 compare equal, so the earlier entry's bits are the output), a NaN
 * beats every number for max and min alike (torch's amax / amin) and among NaNs the lowest e wins.  Rows without
 * entries get Z = +0.0 and arg = -1.  Z holds the winning entry's own bits.
 * Arguments of hcspmm_forward_weighted without values_d (strided X / Z, x_rows, rectangular blocks, with a plan or
 * plan-free), plus
 *   reduce       HCSPMM_REDUCE_MAX or HCSPMM_REDUCE_MIN
 *   arg_out_d    int32 [num_nodes][ldarg], or NULL: no positions are stored (inference)
 *   ldarg        row stride of arg_out_d in elements (>= embedding_dim when arg_out_d is set)
 *   workspace_d  >= hcspmm_extremum_workspace_bytes() (values and positions of split rows' partial slots)
 * fp32 only: HCSPMM_DTYPE_F16 / BF16, a bad reduce, short strides and the other argument errors of
 * hcspmm_forward_weighted are HCSPMM_EINVAL before any device call.  MFMA takes no maximum: dense-tile windows are served
 * from CSR by the sparse-row gather.  Separate kernels (spmm_extremum.hip) on the binary product's plan.
 * ---------------------------------------------------------------------------------------- */
#define HCSPMM_REDUCE_MAX 0
#define HCSPMM_REDUCE_MIN 1
size_t hcspmm_extremum_workspace_bytes(const hcspmm_plan_header* header_h, int embedding_dim); /* 2 x hcspmm_workspace_bytes */
int hcspmm_forward_extremum(const void* X_d, int64_t x_rows, int64_t ldx, void* Z_d, int64_t ldz, int dtype,
                            const int32_t* row_pointers_d, const int32_t* column_index_d, const int32_t* blockPartition_d,
                            const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d, const int32_t* hybrid_type_d,
                            const int32_t* plan_d, const hcspmm_plan_header* plan_header_h, int64_t num_nodes,
                            int64_t num_edges, int embedding_dim, void* workspace_d, size_t workspace_bytes, void* stream,
                            int reduce, int32_t* arg_out_d, int64_t ldarg);

/* Backward of hcspmm_forward_extremum on a square, pattern-symmetric graph:
 *   grad_X[j][d] = sum of grad_Z[i][d] over the entries e = (i, j) with arg[i][d] == e
 * computed by walking A^T -- A's own pattern: row j's entry e_t has i = column_index[e_t] and e = transpose_perm[e_t]
 * (hcspmm_transpose_permutation) -- on the forward's plan and schedule, so hubs stay balanced.  Each (j, d) is summed in
 * a fixed order (CSR order, the wide tasks' shuffle tree, split rows through the fp32 fix-up pass and workspace), with
 * no atomics: two calls give the same bits.  Columns no entry won get +0.0.  grad_Z_d, arg_d and grad_X_out_d are
 * [num_nodes] rows of ldg / ldarg / ldgx elements (each >= embedding_dim); arg_d is the forward's arg_out_d.
 * workspace_d >= hcspmm_workspace_bytes() (hcspmm_extremum_workspace_bytes also serves).  Argument errors as
 * hcspmm_forward_extremum, a NULL arg_d or transpose_perm_d (E > 0) included.  Asynchronous on `stream`.
 * Directed graphs: the launch walks whatever graph it is handed and assumes no symmetry of it.  Called with A^T's graph
 * tensors and plan (hcspmm_transpose_graph, then the preprocessing and plan of A^T) and entry_index_t as transpose_perm_d, row
 * j's entry e_t has i = column_index_t[e_t] and e = entry_index_t[e_t], which is the formula above for any square A. */
int hcspmm_forward_extremum_backward(const float* grad_Z_d, int64_t ldg, const int32_t* arg_d, int64_t ldarg,
                                     float* grad_X_out_d, int64_t ldgx, const int32_t* row_pointers_d,
                                     const int32_t* column_index_d, const int32_t* blockPartition_d,
                                     const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d, const int32_t* hybrid_type_d,
                                     const int32_t* plan_d, const hcspmm_plan_header* plan_header_h, int64_t num_nodes,
                                     int64_t num_edges, int embedding_dim, const int32_t* transpose_perm_d, void* workspace_d,
                                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sum, sum of squares, max and min of each row's neighbours in ONE gather pass (PNA's mean / std / max / min; any layer that
 * needs more than one of them).  With x_e = X[column_index[e]][d] over e in [row_pointers[r], row_pointers[r+1]):
 *   Z_sum[r][d]   = sum of x_e
 *   Z_sumsq[r][d] = sum of fl(x_e * x_e): the square is rounded to fp32 before it is added (never an fma), so a row summed by
 *                   one lane group has the bits of a sequential fp32 scan
 *   Z_max / arg_max, Z_min / arg_min: exactly hcspmm_forward_extremum's contract (ties to the lowest e, -0 == +0, NaN wins,
 *                   the winning entry's own bits, independent of the split)
 * Rows without entries get +0.0 in all four values and -1 in both args.  The sums run in a fixed order (CSR order inside a
 * lane group, the wide tasks' shuffle tree, split rows in slot order): deterministic, no atomics; combined rows are within
 * 1e-5 * sum|x_e| (1e-5 * sum x_e^2) of the exact value.
 * Each of the six outputs may be NULL and is then not written; at least one Z_* must be set.  The four Z_* share the row
 * stride ldz, the two args ldarg: one [num_nodes][4 * D] buffer is the call with pointers D apart and ldz = 4 * D.
 * Other arguments as hcspmm_forward_extremum (strided X, x_rows, rectangular blocks, with a plan or plan-free);
 * workspace_d >= hcspmm_multi_workspace_bytes() (six arrays per partial slot of a split row).
 * fp32 only: HCSPMM_DTYPE_F16 / BF16, all four Z_* NULL, ldx or ldz < embedding_dim, ldarg < embedding_dim with an arg set
 * and the other argument errors of hcspmm_forward_extremum are HCSPMM_EINVAL before any device call.  num_nodes == 0 returns
 * HCSPMM_OK without a launch.  Asynchronous on `stream`.  Separate kernels (spmm_multi.hip) on the binary product's plan.
 * ---------------------------------------------------------------------------------------- */
size_t hcspmm_multi_workspace_bytes(const hcspmm_plan_header* header_h, int embedding_dim); /* 6 x hcspmm_workspace_bytes */
int hcspmm_forward_multi(const void* X_d, int64_t x_rows, int64_t ldx, int dtype, float* Z_sum_d, float* Z_sumsq_d, float* Z_max_d,
                         float* Z_min_d, int64_t ldz, int32_t* arg_max_d, int32_t* arg_min_d, int64_t ldarg,
                         const int32_t* row_pointers_d, const int32_t* column_index_d, const int32_t* blockPartition_d,
                         const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d, const int32_t* hybrid_type_d,
                         const int32_t* plan_d, const hcspmm_plan_header* plan_header_h, int64_t num_nodes, int64_t num_edges,
                         int embedding_dim, void* workspace_d, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-channel softmax aggregation of each row's neighbours in ONE gather pass (DeeperGCN / GENConv, PyG SoftmaxAggregation).
 * With x_e = X[column_index[e]][d] and s_e = fl(beta[d] * x_e) over e in [row_pointers[r], row_pointers[r+1]):
 *   Z[r][d] = sum_e p_e x_e,   p_e = exp(s_e) / sum_e' exp(s_e')
 *   M[r][d] = max_e s_e (bit for bit)    L[r][d] = sum_e exp(s_e - M)    Q[r][d] = sum_e p_e fl(x_e * x_e)
 * beta -> +inf / -inf approaches the max / min, beta = 0 is the mean.  One online-softmax pass: a running maximum, ONE
 * exponential per gathered element, never with a positive argument, so any finite beta * x is safe.  Rows without entries
 * get Z = Q = +0, M = -inf, L = 0.  A column stored twice in a row counts twice.  Fixed order (CSR order inside a lane group,
 * the wide tasks' shuffle tree, split rows in slot order): deterministic, no atomics.  Defined for finite X and beta;
 * other inputs give unspecified values but no out-of-range access.
 * beta_d: [embedding_dim] fp32 on the device.  Z_d is required; M_d, L_d, Q_d may each be NULL and are then not written.  The
 * four share the row stride ldz.  Other arguments as hcspmm_forward_multi (strided X, x_rows, rectangular blocks, with a plan
 * or plan-free); workspace_d >= hcspmm_softmax_workspace_bytes() (four arrays per partial slot of a split row).
 * fp32 only: another dtype, NULL X_d / beta_d / Z_d, ldx or ldz < embedding_dim and the other argument errors of
 * hcspmm_forward_multi are HCSPMM_EINVAL before any device call.  num_nodes == 0 returns HCSPMM_OK without a launch.
 * Asynchronous on `stream`.  Separate kernels (spmm_softmax.hip) on the binary product's plan.
 *
 * hcspmm_softmax_backward: the gradient with respect to X from grad_Z and the forward's Z, M, L ([src_rows] rows of one
 * stride ld_in), on the graph the backward WALKS -- A^T's tensors and plan (hcspmm_transpose_graph), or A's own for a
 * symmetric pattern; num_nodes rows, column ids below src_rows:
 *   grad_X[j][d] = sum over the entries (j, i) of row j of
 *                  exp(fl(beta[d] X[j][d]) - M[i][d]) / L[i][d] * grad_Z[i][d] * (1 + beta[d] (X[j][d] - Z[i][d]))
 * X_d: the [num_nodes] rows the forward gathered (stride ldx).  The weight is recomputed, no per-entry tensor is read.  A
 * plain-sum launch in hcspmm_forward_weighted's order; workspace_d >= hcspmm_workspace_bytes().  The gradient with respect
 * to beta needs no kernel: sum_i grad_Z[i][d] (Q[i][d] - Z[i][d]^2).  Argument errors as above, for every operand.
 * ---------------------------------------------------------------------------------------- */
size_t hcspmm_softmax_workspace_bytes(const hcspmm_plan_header* header_h, int embedding_dim); /* 4 x hcspmm_workspace_bytes */
int hcspmm_forward_softmax(const void* X_d, int64_t x_rows, int64_t ldx, int dtype, const float* beta_d, float* Z_d, float* M_d,
                           float* L_d, float* Q_d, int64_t ldz, const int32_t* row_pointers_d, const int32_t* column_index_d,
                           const int32_t* blockPartition_d, const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d,
                           const int32_t* hybrid_type_d, const int32_t* plan_d, const hcspmm_plan_header* plan_header_h,
                           int64_t num_nodes, int64_t num_edges, int embedding_dim, void* workspace_d, size_t workspace_bytes,
                           void* stream);
int hcspmm_softmax_backward(const float* grad_Z_d, const float* Z_d, const float* M_d, const float* L_d, int64_t ld_in,
                            int64_t src_rows, const float* X_d, int64_t ldx, const float* beta_d, float* grad_X_d, int64_t ldgx,
                            const int32_t* row_pointers_d, const int32_t* column_index_d, const int32_t* blockPartition_d,
                            const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d, const int32_t* hybrid_type_d,
                            const int32_t* plan_d, const hcspmm_plan_header* plan_header_h, int64_t num_nodes, int64_t num_edges,
                            int embedding_dim, void* workspace_d, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gated neighbour aggregation (residual gated graph convolution, Bresson & Laurent; PyG ResGatedGraphConv): a message that
 * depends on the DESTINATION row as well as on the gathered one, with no per-entry tensor.  For entry e = (r, c) of row r,
 * c = column_index[e], and z = fl32(P[r][d] + Q[c][d]) (one fp32 add, never contracted):
 *   Z_gate [r][d] = sum_e sigma (z) * V[c][d]        sigma (z) = 1 / (1 + exp(-z))
 *   Z_dgate[r][d] = sum_e sigma'(z) * V[c][d]        sigma'(z) = sigma(z) (1 - sigma(z))
 * The exponential never takes a positive argument: t = exp(-|z|), r = 1 / (1 + t), sigma = z >= 0 ? r : t r, sigma' = t r r,
 * each product rounded once, then acc = fmaf(sigma, v, acc).  Where exp(-|z|) underflows to 0 (|z| >= 104) sigma is EXACTLY 1
 * for z > 0 and exactly 0 for z < 0, and sigma' is exactly 0; a NaN in z propagates; +-inf behaves as the limit.
 *   P_d      fp32 [num_nodes][ldp], indexed by the row itself
 *   Q_d, V_d fp32 [src_rows][ldq] / [src_rows][ldv], indexed by column ids (src_rows may differ from num_nodes: a rectangular
 *            block).  The three strides are independent: three column blocks of one projection pass as they are
 *   Z_gate_d, Z_dgate_d  fp32 [num_nodes][ldz]; either may be NULL and is then neither computed nor written, at least one
 *            must be set.  With both set, both sums come out of ONE gather pass, and each has the bits of its single-output call
 * It runs on the binary product's preprocessing and plan, or plan-free, every row served from CSR as in
 * hcspmm_forward_extremum (a matrix core takes no per-column gate).  Each (r, d) is summed in hcspmm_forward_weighted's order:
 * CSR order on ordinary and tiny tasks and on the rows of dense-tile windows, the wide tasks' shuffle tree on wide tasks, fp32
 * partials and a fix-up pass in fixed order for sliced and segmented rows.  No atomics: two calls give the same bits.  Rows
 * without entries get +0.0 in every set output.  A column stored twice in a row counts twice.
 * workspace_d >= hcspmm_gated_workspace_bytes() (one area of partial slots per output).  Every embedding_dim
 * hcspmm_forward_extremum serves.  NULL P_d / Q_d / V_d with rows to serve, both outputs NULL, ldp / ldq / ldv / ldz <
 * embedding_dim, embedding_dim <= 0, negative sizes and NULL graph arrays are HCSPMM_EINVAL before any device call; plan and
 * workspace errors as hcspmm_forward_softmax (src_rows against the rows the plan gathers).  num_nodes == 0 returns HCSPMM_OK
 * without a launch.  Asynchronous on `stream`, allocates nothing, capturable.  Separate kernels (spmm_gated.hip).
 * The gradients need no further kernel and no per-entry tensor.  With G = grad_Z_gate:
 *   grad_P = G * Z_dgate(P, Q, V)                      (element-wise; ask the forward call for both outputs)
 *   on the graph the backward walks (A^T's tensors and plan, or A's own for a symmetric pattern), one two-output call with
 *   own rows P := Q and gathered (Q, V) := (P, G):   grad_V = Y_gate,   grad_Q = V * Y_dgate
 * fl32(Q[j] + P[i]) has the bits of fl32(P[i] + Q[j]), so the gates are the forward's.
 * ---------------------------------------------------------------------------------------- */
size_t hcspmm_gated_workspace_bytes(const hcspmm_plan_header* header_h, int embedding_dim); /* 2 x hcspmm_workspace_bytes */
int hcspmm_forward_gated(const float* P_d, int64_t ldp, const float* Q_d, int64_t ldq, const float* V_d, int64_t ldv,
                         int64_t src_rows, float* Z_gate_d, float* Z_dgate_d, int64_t ldz, const int32_t* row_pointers_d,
                         const int32_t* column_index_d, const int32_t* blockPartition_d, const int32_t* edgeToColumn_d,
                         const int32_t* edgeToRow_d, const int32_t* hybrid_type_d, const int32_t* plan_d,
                         const hcspmm_plan_header* plan_header_h, int64_t num_nodes, int64_t num_edges, int embedding_dim,
                         void* workspace_d, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Edge-feature messages (GINE, SchNet / CFConv continuous filters, edge-gated convolutions, "sum the incident edge vectors"):
 * a neighbour's row combined with a feature VECTOR of the edge, one value per column instead of one per entry or head:
 *   Z[r][d] = sum over e in [row_pointers[r], row_pointers[r+1])  m(X[column_index[e]][d], F[fi(e)][d])
 *   fi(e)   = f_index[e] if f_index_d != NULL else e
 *   HCSPMM_EDGE_OP_MUL      : acc = fmaf(f, x, acc)
 *   HCSPMM_EDGE_OP_ADD_RELU : t = x + f (one fp32 add); m = (t < 0) ? +0 : t (a NaN propagates); acc = acc + m
 *   HCSPMM_EDGE_OP_COPY     : acc = acc + f                       (X_d is ignored and may be NULL)
 * fp32.  It runs on the binary product's preprocessing and plan, or plan-free, with hcspmm_forward_weighted's fp32 schedule
 * at the same width (ordinary, wide, column-sliced, segmented and tiny tasks; hcspmm_wide_threshold).  A matrix core takes no
 * per-column value: dense-tile windows are served from CSR by the sparse-row gather, as in hcspmm_forward_extremum.  Each
 * (r, d) is summed in CSR order on ordinary and tiny tasks and on the rows of dense-tile windows, by the wide tasks' shuffle
 * tree on wide tasks, and through fp32 partials in the workspace (hcspmm_workspace_bytes) and a fix-up pass in fixed order
 * for sliced and segmented rows.  No atomics: two calls give the same bits.  Rows without entries get +0.0.
 *   X_d      fp32 [x_rows][ldx], indexed by column ids (x_rows may differ from num_nodes: a rectangular block)
 *   F_d      fp32 [f_rows][ldf], ldf >= embedding_dim; read on every call.  F, Z and the partials are addressed in 64 bits
 *            (num_edges * ldf may pass 2^31)
 *   f_index_d  int32 [num_edges] or NULL; every index must lie in [0, f_rows) and is trusted on the device, as value_index is
 *            in hcspmm_forward_weighted_indexed (many-to-one indices and f_rows != num_edges are fine).  Without an index
 *            f_rows >= num_edges
 *   Z_d      fp32 [num_nodes][ldz]
 * Every embedding_dim hcspmm_forward_extremum serves (1, 3, 22, ... through the element-aligned 16-byte lanes, for X and F
 * alike).  A bad op, NULL F_d with num_edges > 0, NULL X_d for MUL / ADD_RELU, short strides, f_rows < num_edges without an
 * index, f_rows == 0 with num_edges > 0 and the argument errors of hcspmm_forward_weighted are HCSPMM_EINVAL before any
 * device call.  Separate kernels (spmm_edge_messages.hip).  Asynchronous on `stream`.
 * The gradient with respect to X needs no kernel of its own: it is this forward on A^T's graph and plan
 * (hcspmm_transpose_graph) with f_index = entry_index_t -- or, on a pattern-symmetric graph, on the same graph with f_index =
 * hcspmm_transpose_permutation's perm:
 *   MUL      : dX = forward(op = MUL, X := grad_Z, F, f_index)
 *   ADD_RELU : dX = forward(op = COPY, F := grad_F, f_index)       (grad_F from hcspmm_edge_messages_grad)
 * ---------------------------------------------------------------------------------------- */
#define HCSPMM_EDGE_OP_MUL 0
#define HCSPMM_EDGE_OP_ADD_RELU 1
#define HCSPMM_EDGE_OP_COPY 2
int hcspmm_forward_edge_messages(const void* X_d, int64_t x_rows, int64_t ldx, const float* F_d, int64_t f_rows, int64_t ldf,
                                 const int32_t* f_index_d /* [E] or NULL */, int op, void* Z_d, int64_t ldz,
                                 const int32_t* row_pointers_d, const int32_t* column_index_d, const int32_t* blockPartition_d,
                                 const int32_t* edgeToColumn_d, const int32_t* edgeToRow_d, const int32_t* hybrid_type_d,
                                 const int32_t* plan_d, const hcspmm_plan_header* plan_header_h, int64_t num_nodes,
                                 int64_t num_edges, int embedding_dim, void* workspace_d, size_t workspace_bytes, void* stream);

/* Gradient of hcspmm_forward_edge_messages with respect to F (direct form, F [num_edges][ldf]), fp32:
 *   MUL      : grad_F[e][d] = grad_Z[row(e)][d] * X[column_index[e]][d]                      (one fp32 multiplication)
 *   ADD_RELU : grad_F[e][d] = (X[column_index[e]][d] + F[e][d] > 0) ? grad_Z[row(e)][d] : +0  (the forward's own fp32 add)
 *   COPY     : grad_F[e][d] = grad_Z[row(e)][d]                                              (X_d and F_d may be NULL)
 * Edge-parallel over contiguous CSR chunks like hcspmm_sddmm (a row cursor, no search per entry), so a hub row is cut wherever
 * the chunks fall; every element of grad_F_out_d [num_edges][ldgf] is written exactly once; no atomics.  grad_Z_d is
 * [num_nodes][ldg], X_d [x_rows][ldx] (column ids are trusted), F_d [num_edges][ldf] (read by ADD_RELU only); all addressing
 * of F and grad_F is 64-bit.  A bad op, NULL pointers an op reads (num_edges > 0), short strides and negative sizes are
 * HCSPMM_EINVAL before any device call; num_edges = 0 launches nothing.  Asynchronous on `stream`. */
int hcspmm_edge_messages_grad(const float* grad_Z_d, int64_t ldg, const float* X_d, int64_t x_rows, int64_t ldx, const float* F_d,
                              int64_t ldf, float* grad_F_out_d, int64_t ldgf, int op, const int32_t* row_pointers_d,
                              const int32_t* column_index_d, int64_t num_nodes, int64_t num_edges, int embedding_dim,
                              void* stream);

/* Edge normalisations of a square graph, on the device (asynchronous on `stream`); deg(r) = stored entries of row r, so
 * self-loops count only when the graph stores them.  Rows of degree 0 own no entries.
 *   HCSPMM_NORM_SYM  : values[e] = 1 / sqrt(deg(r) * deg(c))  (GCN: D^-1/2 A D^-1/2)
 *   HCSPMM_NORM_MEAN : values[e] = 1 / deg(r)                 (GraphSAGE-mean: D^-1 A) */
#define HCSPMM_NORM_SYM 0
#define HCSPMM_NORM_MEAN 1
int hcspmm_edge_norm_device(const int32_t* row_pointers_d, const int32_t* column_index_d, int64_t num_nodes,
                            int64_t num_edges, int kind, float* values_out_d, void* stream);

/* Transpose of a pattern-symmetric weighted graph in A's own CSR order (host): perm_out_h[E] such that values[perm] are the
 * values of A_w^T entry by entry, so the backward dX = A_w^T * G is hcspmm_forward_weighted on the same graph and plan with
 * values[perm] -- also for asymmetric values such as the mean normalisation.  HCSPMM_EINVAL when the pattern is not
 * symmetric (or a row's columns are not strictly ascending). */
int hcspmm_transpose_permutation(const int32_t* row_pointers_h, const int32_t* column_index_h, int64_t num_nodes,
                                 int64_t num_edges, int32_t* perm_out_h);

/* Transpose of any CSR graph (host; a counting sort): A is num_rows x num_cols with num_edges entries, A^T is num_cols x
 * num_rows.  Entry e_t of row j of A^T is the entry (i, j) of A: column_index_t[e_t] = i and entry_index_t[e_t] = the CSR
 * position e of (i, j) in A, so values[entry_index_t] are A_w^T's values.  Within a row of A^T the entries ascend in i: A^T
 * has strictly ascending columns whenever A does.  On a pattern-symmetric square graph the three outputs are row_pointers,
 * column_index and hcspmm_transpose_permutation's perm, element for element.  HCSPMM_EINVAL for NULL outputs, negative
 * sizes, a column id outside [0, num_cols) or a row whose columns are not strictly ascending (nothing is written then);
 * num_edges = 0 fills row_pointers_t with zeros. */
int hcspmm_transpose_graph(const int32_t* row_pointers_h, const int32_t* column_index_h, int64_t num_rows, int64_t num_cols,
                           int64_t num_edges, int32_t* row_pointers_t_out_h /* [num_cols + 1] */,
                           int32_t* column_index_t_out_h /* [E]: the row i of A */,
                           int32_t* entry_index_t_out_h /* [E]: the CSR position e of (i, j) in A */);

/* hcspmm_transpose_graph on the device: the same three outputs, element for element, on every input the host function
 * accepts (rectangular ones included), asynchronous on `stream` with no host read -- for graphs that change from step to step
 * (a sample redrawn every epoch, below).  A stable radix sort of (column, e) by column: within a row of A^T the entries ascend
 * in e.  What the host version validates this one TRUSTS, as the plan-free kernels trust column_index: row_pointers[0] = 0,
 * row_pointers[num_rows] = num_edges, ids in [0, num_cols).  It never writes out of bounds whatever the ids are -- a column id
 * is never used as an address, only eight bits of it at a time as a digit -- and with an id outside [0, num_cols) the result is
 * unspecified.  workspace_d >= hcspmm_transpose_graph_device_workspace_bytes() (HCSPMM_EWORKSPACE otherwise; 0 bytes for
 * num_edges = 0, which fills row_pointers_t with zeros).  NULL pointers and negative sizes are HCSPMM_EINVAL before any device
 * call. */
size_t hcspmm_transpose_graph_device_workspace_bytes(int64_t num_rows, int64_t num_cols, int64_t num_edges);
int hcspmm_transpose_graph_device(const int32_t* row_pointers_d, const int32_t* column_index_d, int64_t num_rows, int64_t num_cols,
                                  int64_t num_edges, int32_t* row_pointers_t_out_d /* [num_cols + 1] */,
                                  int32_t* column_index_t_out_d /* [E] */, int32_t* entry_index_t_out_d /* [E] */,
                                  void* workspace_d, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fanout-limited neighbour sampling on the device (GraphSAGE's neighbourhood, on the full node set):
 *   fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16                 (uint32 arithmetic)
 *   key(e, seed) = fmix32(fmix32((uint32)e * 0x9E3779B1 + (uint32)seed) + (uint32)(seed >> 32))          e: CSR position
 * A row with at most `fanout` entries keeps them all; a longer one keeps the `fanout` entries with the smallest keys.  Kept
 * entries stay in ascending e, so ascending columns stay ascending.  For one seed, key is a bijection of e: no ties.  A key
 * depends on (e, seed) alone, so the sample is the same whatever the launch shape; no atomics, no floating point.
 *   row_pointers_s [num_nodes + 1]  the exclusive scan of min(deg, fanout): a function of the graph and the fanout, NOT of the
 *                                   seed -- hcspmm_sample_row_pointers_device, once per (graph, fanout); E_s = its last element
 *   column_index_s [E_s], entry_index_s [E_s]  the kept entries' column ids and their positions in A (values travel as
 *                                   values[entry_index_s], or through hcspmm_forward_weighted_indexed) --
 *                                   hcspmm_sample_neighbors_device, once per seed: fixed output shapes, no host read, no allocation
 * Rows longer than the fanout are selected by one wave up to HCSPMM_SAMPLE_WAVE_ROW_MAX entries and by a workgroup beyond.
 * hcspmm_sample_neighbors_device trusts row_pointers_s_d to be the scan for THIS graph and fanout.  fanout < 1, NULL pointers
 * and negative sizes are HCSPMM_EINVAL before any device call; a workspace below hcspmm_sample_workspace_bytes() is
 * HCSPMM_EWORKSPACE.  num_nodes = 0 or num_edges = 0 samples nothing (the scan still writes its zeros).  Asynchronous on
 * `stream`. */
#define HCSPMM_SAMPLE_WAVE_ROW_MAX 512
size_t hcspmm_sample_workspace_bytes(int64_t num_nodes);
int hcspmm_sample_row_pointers_device(const int32_t* row_pointers_d, int64_t num_nodes, int fanout,
                                      int32_t* row_pointers_s_out_d /* [num_nodes + 1] */, void* workspace_d,
                                      size_t workspace_bytes, void* stream);
int hcspmm_sample_neighbors_device(const int32_t* row_pointers_d, const int32_t* column_index_d,
                                   const int32_t* row_pointers_s_d, int64_t num_nodes, int64_t num_edges, int fanout,
                                   uint64_t seed, int32_t* column_index_s_out_d /* [E_s] */,
                                   int32_t* entry_index_s_out_d /* [E_s] */, void* stream);

/* ------------------------------------------------------------------------------------------
 * SDDMM (sampled dense-dense product) on the stored entries -- with the two edge softmax entry points below, the kernels
 * that produce and differentiate edge values (the gradient of hcspmm_forward_weighted with respect to its values is
 * hcspmm_sddmm(dZ, X); attention layers compute their values from the features):
 *   out_d[e] = sum_k A[row(e)][k] * B[column_index[e]][k]      for every e in [0, E), fp32, in CSR order
 *   A_d  [num_nodes][lda]  one row per CSR row;  B_d [b_rows][ldb]  indexed by column ids (may be rectangular: a row block)
 *   dtype HCSPMM_DTYPE_*: A and B of that type, 16-bit elements widened; the sum is accumulated in fp32 either way.
 * Every entry is written exactly once (rows without entries own nothing); no atomics.  The order is fixed -- each of L
 * lanes sums its own columns with fmaf in column order, then a fixed xor-butterfly over the L lanes -- so two calls give
 * the same bits, and the result is within (D + 1) * 2^-24 * sum_k |a_k b_k| of the exact product of the widened inputs.
 * plan_d / plan_header_h (both or neither): the header vouches for the column range -- HCSPMM_EINVAL when its num_columns
 * exceeds b_rows, HCSPMM_EPLAN when it does not match num_nodes / num_edges; plan-free, column_index is trusted, as in
 * hcspmm_forward_typed.  Argument errors (NULL pointers, D <= 0, lda / ldb < D, a bad dtype, negative sizes) are
 * HCSPMM_EINVAL before any device call; E = 0 launches nothing.  Asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------- */
int hcspmm_sddmm(const void* A_d, int64_t lda, const void* B_d, int64_t b_rows, int64_t ldb, int dtype, float* out_d,
                 const int32_t* row_pointers_d, const int32_t* column_index_d, const int32_t* plan_d,
                 const hcspmm_plan_header* plan_header_h, int64_t num_nodes, int64_t num_edges, int embedding_dim, void* stream);

/* Multi-head SDDMM: hcspmm_sddmm per head on the column slices of Dh = embedding_dim / heads columns, in one launch:
 *   out_d[h * E + e] = <A[row(e)][h * Dh : (h + 1) * Dh], B[column_index[e]][h * Dh : (h + 1) * Dh]>
 * head-major [heads][E].  Each head's result is bit for bit hcspmm_sddmm on the slice views A_d + h * Dh, B_d + h * Dh (same
 * lda / ldb) at width Dh: same lanes, vector width, column order and butterfly.  One column-index load per entry serves
 * every head; deterministic, no atomics.  fp32 only (F16 / BF16 are HCSPMM_EINVAL); heads >= 1, embedding_dim % heads == 0
 * and Dh % 4 == 0; the plan / b_rows checks and the other argument checks of hcspmm_sddmm, all before any device call. */
int hcspmm_sddmm_heads(const void* A_d, int64_t lda, const void* B_d, int64_t b_rows, int64_t ldb, int dtype, float* out_d,
                       const int32_t* row_pointers_d, const int32_t* column_index_d, const int32_t* plan_d,
                       const hcspmm_plan_header* plan_header_h, int64_t num_nodes, int64_t num_edges, int embedding_dim,
                       void* stream, int heads);

/* Edge softmax over each row's stored entries, per head, on head-major fp32 arrays [heads][E] (head h is the contiguous
 * slice [h * E, (h + 1) * E), which hcspmm_forward_weighted takes as its values as is):
 *   alpha[e] = exp(logits[e] - m_r) / sum_{j in row r} exp(logits[j] - m_r),   m_r = max_{j in row r} logits[j]
 * Logits must be finite.  Rows of up to 16 entries are taken by one thread, up to 2048 by one wave, longer ones by a
 * workgroup of 256 threads; each row's sums run in an order fixed by its length alone: deterministic.  Argument errors
 * (NULL pointers, heads <= 0, negative sizes) are HCSPMM_EINVAL before any device call.  Asynchronous on `stream`. */
int hcspmm_edge_softmax(const float* logits_d, float* alpha_out_d, const int32_t* row_pointers_d, int64_t num_nodes,
                        int64_t num_edges, int heads, void* stream);

/* Backward of hcspmm_edge_softmax, same layout and contract:
 *   grad_logits[e] = alpha[e] * (grad_alpha[e] - sum_{j in row r} alpha[j] * grad_alpha[j]) */
int hcspmm_edge_softmax_backward(const float* alpha_d, const float* grad_alpha_d, float* grad_logits_out_d,
                                 const int32_t* row_pointers_d, int64_t num_nodes, int64_t num_edges, int heads, void* stream);

/* GAT attention: the per-entry logits of a graph attention layer and their edge softmax in one launch for all heads, from
 * node-major fp32 scores s_dst [num_nodes][heads] and s_src [src_rows][heads]:
 *   z[h][e] = s_dst[r][h] + s_src[c][h],  l = z > 0 ? z : z * negative_slope,  alpha[h][e] = softmax of l[h] over row r
 * for entry e of row r with column c; alpha_out_d is head-major [heads][E], the layout of hcspmm_edge_softmax, and is bit
 * for bit hcspmm_edge_softmax applied to l (same row scheme and fold order; l is rounded as a separate product).  z and l
 * are never stored.  s_src may be rectangular (a row block): column ids are trusted to be below src_rows, as on the
 * plan-free paths.  Argument errors (NULL pointers, heads <= 0, negative sizes, a non-finite negative_slope) are
 * HCSPMM_EINVAL before any device call; E = 0 launches nothing.  Asynchronous on `stream`. */
int hcspmm_gat_attention(const float* s_dst_d, const float* s_src_d, int64_t src_rows, float negative_slope,
                         float* alpha_out_d, const int32_t* row_pointers_d, const int32_t* column_index_d,
                         int64_t num_nodes, int64_t num_edges, int heads, void* stream);

/* Backward of hcspmm_gat_attention on a square, pattern-symmetric graph (s_src has num_nodes rows), given grad_alpha
 * [heads][E]:
 *   g[h][e]          = alpha (grad_alpha - sum_{j in row r} alpha[h][j] grad_alpha[h][j]) * (z > 0 ? 1 : negative_slope)
 *   grad_s_dst[r][h] = sum_{e in row r} g[h][e];   grad_s_src[c][h] = sum_{e' in row c} g[h][transpose_perm[e']]
 * with transpose_perm_d [E] from hcspmm_transpose_permutation and z recomputed with the forward's bits (the derivative at
 * z == 0 is negative_slope).  grad_scores_out_d [heads][E] receives g.  Two launches, rows walked as in the forward, fixed
 * orders and no atomics: two calls give the same bits.  Rows without entries get zeros, so with E = 0 both grad_s_*
 * arrays are zeroed.  Argument errors as hcspmm_gat_attention.  Asynchronous on `stream`. */
int hcspmm_gat_attention_backward(const float* alpha_d, const float* grad_alpha_d, const float* s_dst_d,
                                  const float* s_src_d, float negative_slope, const int32_t* row_pointers_d,
                                  const int32_t* column_index_d, const int32_t* transpose_perm_d,
                                  int64_t num_nodes, int64_t num_edges, int heads,
                                  float* grad_scores_out_d /* g, [heads][E] */,
                                  float* grad_s_dst_out_d /* [N][heads] */, float* grad_s_src_out_d /* [N][heads] */,
                                  void* stream);

/* hcspmm_gat_attention_backward without the symmetry requirement: the column side walks A^T (hcspmm_transpose_graph),
 *   grad_s_src[c][h] = sum_{e_t in row c of A^T} g[h][entry_index_t[e_t]]
 * with s_src and grad_s_src of src_rows rows (A is num_nodes x src_rows, row_pointers_t_d has src_rows + 1 elements).  The
 * row-side launch is hcspmm_gat_attention_backward's; so is the column-side kernel, which only ever walked a row-pointer
 * array and an index array: passing (row_pointers, perm, num_nodes) of a pattern-symmetric graph gives that function's bits.
 * Same determinism contract and argument errors, NULL transposed arrays included. */
int hcspmm_gat_attention_backward_directed(const float* alpha_d, const float* grad_alpha_d, const float* s_dst_d,
                                           const float* s_src_d, float negative_slope, const int32_t* row_pointers_d,
                                           const int32_t* column_index_d, const int32_t* row_pointers_t_d,
                                           const int32_t* entry_index_t_d, int64_t src_rows, int64_t num_nodes,
                                           int64_t num_edges, int heads, float* grad_scores_out_d /* g, [heads][E] */,
                                           float* grad_s_dst_out_d /* [N][heads] */,
                                           float* grad_s_src_out_d /* [src_rows][heads] */, void* stream);

/* GATv2 attention logits (Brody et al.: the non-linearity inside the dot product), all heads in one launch, from fp32 node
 * features H_dst [num_nodes][ld_dst] and H_src [src_rows][ld_src] of embedding_dim = heads * Dh columns (Dh % 4 == 0; leading
 * dimensions >= embedding_dim in elements, so the two halves of one [N, 2 D] projection can be passed as views) and att
 * [heads][Dh]:
 *   z = H_dst[r][h*Dh + k] + H_src[c][h*Dh + k],  l = z > 0 ? z : z * negative_slope,  logits[h][e] = sum_k att[h][k] * l
 * for entry e of row r with column c; logits_out_d is head-major [heads][E], the layout of hcspmm_edge_softmax.  z and l
 * are each rounded once (never contracted into a neighbouring operation) and never stored; per entry and head the sum runs
 * over a lane's four columns in column order with fmaf, then over the head's lanes by a fixed xor butterfly, so two calls
 * give the same bits and every head has the bits of a single-head call on its column slice.  H_src may be rectangular (a
 * row block): column ids are trusted to be below src_rows, as on the plan-free paths.  Argument errors (NULL pointers,
 * heads <= 0, embedding_dim <= 0 or not a multiple of heads, Dh % 4 != 0, a leading dimension below embedding_dim,
 * negative sizes, a non-finite negative_slope) are HCSPMM_EINVAL before any device call; E = 0 launches nothing.
 * Asynchronous on `stream`, no allocation, no synchronisation: capturable into a HIP graph. */
int hcspmm_gatv2_scores(const float* H_dst_d, int64_t ld_dst, const float* H_src_d, int64_t src_rows, int64_t ld_src,
                        const float* att_d /* [heads][Dh] */, float negative_slope, float* logits_out_d /* [heads][E] */,
                        const int32_t* row_pointers_d, const int32_t* column_index_d, int64_t num_nodes,
                        int64_t num_edges, int embedding_dim, int heads, void* stream);

/* Bytes of workspace hcspmm_gatv2_scores_backward needs: one [embedding_dim] fp32 partial of grad_att per workgroup of its
 * row launches, whose grid (at most 4096 workgroups) depends on (num_nodes, embedding_dim) alone.  0 for shapes the
 * backward refuses. */
size_t hcspmm_gatv2_backward_workspace_bytes(int64_t num_nodes, int64_t num_edges, int embedding_dim, int heads);

/* Backward of hcspmm_gatv2_scores on a square, pattern-symmetric graph (H_src has num_nodes rows), given g = grad_logits
 * [heads][E], with d(z) = z > 0 ? 1 : negative_slope from the forward's z (the derivative at z == 0 is negative_slope) and
 * h(j) = j / Dh:
 *   grad_H_dst[r][j] = att[j] * sum_{e in row r}  g[h(j)][e]                   * d(H_dst[r][j] + H_src[col(e)][j])
 *   grad_H_src[c][j] = att[j] * sum_{e' in row c} g[h(j)][transpose_perm[e']] * d(H_dst[col(e')][j] + H_src[c][j])
 *   grad_att[h][k]   = sum_e g[h][e] * l[h][e][k]
 * with transpose_perm_d [E] from hcspmm_transpose_permutation.  Three launches.  Two row-parallel ones write every row of
 * grad_H_dst / grad_H_src exactly once (workgroup b takes the row tiles b, b + grid, ...): a row of up to 256 entries is
 * summed in entry order by one lane group, a longer
 * one by the lane groups of a workgroup (entry i by group i mod NG, in order), the partial rows folded by an xor butterfly
 * over a wave's groups and then in wave order.  The grad_H_dst launch also sums g * l per workgroup into workspace_d in a
 * fixed order; the third launch adds those partials in index order.  No atomics: every sum's order is a function of
 * (num_nodes, embedding_dim) and the row lengths, so two calls give the same bits.  Rows without entries get zeros; with
 * E = 0 all three gradients are zeroed.  Argument errors as hcspmm_gatv2_scores; a workspace below
 * hcspmm_gatv2_backward_workspace_bytes is HCSPMM_EWORKSPACE.  Asynchronous on `stream`, capturable into a HIP graph. */
int hcspmm_gatv2_scores_backward(const float* grad_logits_d, const float* H_dst_d, int64_t ld_dst, const float* H_src_d,
                                 int64_t ld_src, const float* att_d, float negative_slope, const int32_t* row_pointers_d,
                                 const int32_t* column_index_d, const int32_t* transpose_perm_d, int64_t num_nodes,
                                 int64_t num_edges, int embedding_dim, int heads, float* grad_H_dst_out_d, int64_t ld_gdst,
                                 float* grad_H_src_out_d, int64_t ld_gsrc, float* grad_att_out_d /* [heads][Dh] */,
                                 void* workspace_d, size_t workspace_bytes, void* stream);

/* hcspmm_gatv2_scores_backward without the symmetry requirement: grad_H_src walks A^T (hcspmm_transpose_graph),
 *   grad_H_src[c][j] = att[j] * sum_{e_t in row c of A^T} g[h(j)][entry_index_t[e_t]] * d(H_dst[column_index_t[e_t]][j] + H_src[c][j])
 * with H_src and grad_H_src of src_rows rows.  grad_H_dst and grad_att are hcspmm_gatv2_scores_backward's launches; the
 * grad_H_src launch is the same kernel on the transposed arrays (its row classes follow A^T's row lengths), so passing
 * (row_pointers, column_index, perm, num_nodes) of a pattern-symmetric graph gives that function's bits.  Same determinism
 * contract, workspace and argument errors, NULL transposed arrays included. */
int hcspmm_gatv2_scores_backward_directed(const float* grad_logits_d, const float* H_dst_d, int64_t ld_dst, const float* H_src_d,
                                          int64_t ld_src, const float* att_d, float negative_slope,
                                          const int32_t* row_pointers_d, const int32_t* column_index_d,
                                          const int32_t* row_pointers_t_d, const int32_t* column_index_t_d,
                                          const int32_t* entry_index_t_d, int64_t src_rows, int64_t num_nodes, int64_t num_edges,
                                          int embedding_dim, int heads, float* grad_H_dst_out_d, int64_t ld_gdst,
                                          float* grad_H_src_out_d, int64_t ld_gsrc, float* grad_att_out_d /* [heads][Dh] */,
                                          void* workspace_d, size_t workspace_bytes, void* stream);

/* hcspmm_wide_threshold for a feature type (lanes per row, hence the threshold, depend on the element size). */
int32_t hcspmm_wide_threshold_typed(const hcspmm_plan_header* header_h, int embedding_dim, int dtype);

/* 1 when the tiny tasks of this plan (header n_tiny: tasks of at most two entries, indices inline in the descriptor) run as
 * a launch of their own behind the hybrid launch, 0 when they stay a region of it: the one predicate hcspmm_forward*,
 * hcspmm_forward_weighted and hcspmm_forward_weighted_heads decide by (n_tiny at least 524 288, or what
 * HCSPMM_TINY_KERNEL_MIN_TASKS says: -1 never, 1 always).  fused != 0 asks about hcspmm_forward_fused, whose tiny tasks never
 * take that launch.  The results are the same bits either way; the query exists so that a caller -- a test -- can tell which
 * kernel a call reaches.  header_h == NULL (plan-free kernel): 0. */
int32_t hcspmm_own_tiny_launch(const hcspmm_plan_header* header_h, int fused);

/* ------------------------------------------------------------------------------------------
 * Fused aggregate + update: out2 = A * X (N x D), out = out2 * weights (N x H), weights row-major
 * D x H with row stride weights_ld_row and column stride weights_ld_col in elements (so a
 * transposed view, GNN_model.py:98,120, needs no copy).  Replaces spmm_forward_plus_fixed32_fused
 * K.cu:596, _fixed64_fused :651, _final_fused :701, _final_fused_64 :759, _GIN_final_fused :810
 * (bindings B.cpp:310-498) and their kernels K.cu:1639-2770.
 * `out_d` may be a caller-owned buffer (forward_final_fused writes the caller's `output`).
 *
 * Three forms, the same results (out2 bit-identical in all of them; out bit-identical in forms 0 and 2).
 * 0, two launches: the hybrid launch (out2 = A * X) followed by one streaming MFMA update launch over all rows.
 * 2, row tiles (fused_rows.hip; the reference keeps a window's aggregate in shared memory and multiplies it in the same
 *   block, K.cu:1807-1837): persistent launches take 16 CONSECUTIVE TASKS of the length-sorted task list (the update does
 *   not care which 16 rows share a tile), or one dense-tile window, sum them exactly as the plain kernel does, write the
 *   rows of out2 from the registers, park the 16 x D tile in a wave-private LDS area and run the update's MFMA chain on
 *   it (weights staged in LDS once per workgroup), so out2 is never read back.  Rows summed by whole waves or in pieces
 *   (wide tasks, split and column-sliced rows) stay in the hybrid launch and are multiplied by a small launch behind the
 *   fix-up pass.  fp32, D in [17, 128] and H <= 32 or 49 ... 64 (widths off the 16-column grid are zero-padded inside the launch), sparse region in one column pass (D < 64, or a
 *   short-row graph, or hcspmm_plan_params.panel_cols < 0); D = 128 is summed in two column chunks of 64 (eight-wave
 *   workgroups, `out` accumulated over the chunks in the same order).  +2 ... +34 % over form 0 wherever out2 is 80 MB or
 *   more at D <= 64, +5 ... +22 % on dense-heavy graphs up to D = 128 with H <= 32 (profiles/r03/ab_fused_rows.log) --
 *   chosen automatically there; opt-in elsewhere (slower on small graphs).
 * 1, in-launch (round 2; plans built with fuse_in_launch = 1, dense-tile windows only): the aggregation runs with
 *   exchanged MFMA operands, which leaves each lane holding one row of the 16 x D tile in the A-operand shape of the
 *   (tile x weights) MFMAs, so the tile goes from the accumulators straight into the update; windows on the sparse-row
 *   path are multiplied by a second launch restricted to them (off_sparse_windows).  128 registers, ~100 MFMAs on the
 *   critical path of latency-bound waves: 0-15 % slower than form 0 here (profiles/r02/ab_fused.log); kept for the record.
 * hcspmm_fused_in_launch() tells which form a (plan, D, H) gets; HCSPMM_FUSED_SINGLE_LAUNCH=0 / 1 / 2 in the environment
 * forces a form for every plan (shapes outside it fall back).
 * ---------------------------------------------------------------------------------------- */
int hcspmm_fused_in_launch(const hcspmm_plan_header* header_h, int embedding_dim, int hidden_dim);
int hcspmm_forward_fused(const float* X_d, float* out_d, float* out2_d, const float* weights_d,
                         int64_t weights_ld_row, int64_t weights_ld_col, int hidden_dim,
                         const int32_t* row_pointers_d, const int32_t* column_index_d,
                         const int32_t* blockPartition_d, const int32_t* edgeToColumn_d,
                         const int32_t* edgeToRow_d, const int32_t* hybrid_type_d, const int32_t* plan_d,
                         const hcspmm_plan_header* plan_header_h, int64_t num_nodes, int64_t num_edges,
                         int embedding_dim, void* workspace_d, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The update GEMM on its own:  out[N x H] = in[N x D] * W  (fp32; in / out row-major and contiguous, W with element
 * strides ldr / ldc, so a transposed view needs no copy).  Replaces torch.mm(X, weights) / torch.mm(d, weights.t()) in the
 * layers (GNN_model.py:67,87,110,134,194 and the backward passes): N is in the millions and D, H a few dozen, so the product
 * is a stream over `in`; the kernel of the fused operators' update launch (W staged in LDS once per workgroup, 16-byte loads,
 * fp32 MFMA) runs it at twice the rate of the library GEMM picked for such shapes on MI355X.  Any D, H >= 1 (shapes outside
 * the streaming kernel's take a plain MFMA kernel).  Deterministic.
 * ---------------------------------------------------------------------------------------- */
int hcspmm_dense_update(const float* in_d, const float* weights_d, int64_t ldr, int64_t ldc, float* out_d, int64_t N, int D,
                        int H, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight gradient of the update GEMM, for the autograd glue around the operators:
 *   dW[D x H] = A^T * B,  A = N x D (rows lda elements apart), B = N x H (rows ldb apart), fp32, dW row-major.
 * Replaces torch.mm(X.t(), d_out) of the reference's backward passes (GNN_model.py:79,101,124,160,181,205,230):
 * with K = N in the hundreds of thousands and a tiny output the library GEMM runs one tile over all of K; this
 * splits K over the grid (fp32 MFMA, partials added in a fixed order: deterministic).
 * Supported: ceil(D/16) <= 8, ceil(H/16) <= 4, their product <= 16 (else HCSPMM_EINVAL -- use a library GEMM).
 * ---------------------------------------------------------------------------------------- */
size_t hcspmm_weight_grad_workspace(int64_t N, int D, int H); /* bytes; 0 if the shape is unsupported */
int hcspmm_weight_grad(const float* A_d, int64_t lda, const float* B_d, int64_t ldb, float* dW_d, int64_t N, int D,
                       int H, void* workspace_d, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * LOI layout reorder (host).  Replaces reorder_plus_new_direct LOI.cpp:660-805 with the in-CSR
 * construction and output ordering of its main (LOI.cpp:826-841, :873-891): perm_out_h[N] lists
 * old vertex ids in their new order (full 16-row groups first, then short groups, then vertices
 * with no out-edges).  Bit-identical output, without the reference's O(N^2/16) per-group bitmap
 * reallocation (LOI.cpp:695) or its 18 269 000-vertex static limit (LOI.cpp:96).
 *   group_sizes_out_h : optional [N] buffer receiving the group sizes in creation order;
 *   n_groups_out      : optional.
 * ---------------------------------------------------------------------------------------- */
int hcspmm_loi_reorder(const int32_t* row_pointers_h, const int32_t* column_index_h, int64_t num_nodes,
                       int64_t num_edges, int32_t* perm_out_h, int32_t* group_sizes_out_h,
                       int64_t* n_groups_out);

/* The same with the reference's other un-windowed variant selectable: HCSPMM_LOI_NEW restates
 * reorder_plus_new (LOI.cpp:505-658), which finds candidate rows through the column's own out-list
 * (it assumes a symmetric graph); on symmetric input both variants give the same order. */
#define HCSPMM_LOI_NEW_DIRECT 0
#define HCSPMM_LOI_NEW 1
/* The reference's two windowed variants (not called by its main): reorder_plus_direct LOI.cpp:286-484 and
 * reorder_plus LOI.cpp:98-284 -- rows ordered by their smallest column id, a group grown from the next 300 rows of
 * that order.  Bit-identical to the reference compiled with this image's libstdc++ (its row order comes from a
 * non-stable std::sort) on the inputs where the reference is defined: at least 50 rows, no row without entries,
 * columns strictly ascending within a row; anything else is HCSPMM_EINVAL (the reference reads out of bounds). */
#define HCSPMM_LOI_WINDOWED_DIRECT 2
#define HCSPMM_LOI_WINDOWED 3
int hcspmm_loi_reorder_variant(const int32_t* row_pointers_h, const int32_t* column_index_h, int64_t num_nodes,
                               int64_t num_edges, int variant, int32_t* perm_out_h, int32_t* group_sizes_out_h,
                               int64_t* n_groups_out);

/* A RELAXED, parallel LOI reorder for graphs on which the exact one above costs more than the training run it is
 * meant to speed up (Reddit-scale: 6.7 s on one host core against 0.4 s for 200 epochs).  Same group growth, profit,
 * tie rule and output order as reorder_plus_new_direct (LOI.cpp:660-805, :873-891); NOT the reference's permutation:
 *   list_cap : a walk of one column's row list reads at most this many rows behind the list's leading run of placed
 *              rows (0 = 64; < 0 = the whole list, as the reference does); of a member's columns the first 4 * list_cap
 *              new ones are walked (hub rows);
 *   batch    : seeds grown concurrently per round against the placement state of the round's start; a row wanted by
 *              several groups of a round goes to the earliest seed (0 = clamp(num_nodes / 2048, 1, 2048); 1 = one seed
 *              at a time, as the reference does);
 *   threads  : host threads (0 = min(16, HCSPMM_THREADS or the hardware's)).
 * The permutation is a function of (graph, batch, list_cap) only -- not of `threads`, not of timing -- and with
 * batch = 1, list_cap < 0 it equals hcspmm_loi_reorder's bit for bit.  params = NULL: all automatic. */
typedef struct hcspmm_loi_fast_params {
  int32_t batch;
  int32_t list_cap;
  int32_t threads;
  int32_t reserved; /* 0 */
} hcspmm_loi_fast_params;
int hcspmm_loi_reorder_fast(const int32_t* row_pointers_h, const int32_t* column_index_h, int64_t num_nodes,
                            int64_t num_edges, const hcspmm_loi_fast_params* params, int32_t* perm_out_h,
                            int32_t* group_sizes_out_h, int64_t* n_groups_out);

/* Apply a LOI permutation to a CSR graph (the step missing from the reference repository,
 * SURVEY.md section 1 L0): new id of old vertex perm[i] is i; rows AND columns are relabelled,
 * columns re-sorted ascending.  Outputs have the sizes of the inputs. */
int hcspmm_apply_permutation(const int32_t* row_pointers_h, const int32_t* column_index_h, int64_t num_nodes,
                             int64_t num_edges, const int32_t* perm_h, int32_t* row_pointers_out_h,
                             int32_t* column_index_out_h);

#ifdef __cplusplus
}
#endif
#endif /* HCSPMM_H */
