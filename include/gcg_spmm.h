/*
 * gcg_spmm.h -- C-ABI of the MI355X (gfx950) graph-convolution hot path.
 *
 * This is the drop-in boundary for the one hot path of afcarl/graphconvgeo:
 * the normalized-adjacency x dense-features product Y = act(H . Z + b) that the
 * reference computes with `theano.sparse.dot` (S.dot) inside its two Lasagne
 * graph-convolution layers. Every entry point names the reference site it replaces.
 *
 *   reference                                   replaced by
 *   ------------------------------------------  -----------------------------------
 *   mlpconv.py:73   S.dot(self.H, activation)   gcg_spmm_csr_f32 / _planned
 *   mlpconv.py:90   S.dot(self.H, activation)   (same; width C instead of K)
 *   mlpconv.py:71   S.dot(input, self.W)        (same kernel: X (CSR N x F) . W1)
 *   mlpconv.py:75-77 + b, rectify               fused epilogue: bias != NULL, act = GCG_ACT_RELU
 *   mlpconv.py:92-94 + b, [target_indices, :]   fused epilogue: bias, out_rows subset
 *   Theano grad of S.dot (x.T . gz)             gcg_spmm_* on CSR(H^T) (= H, H symmetric)
 *                                               and CSR(X^T) from gcg_csr_transpose_f32
 *   Theano grad of Y[target_indices] (inc_subtensor, duplicates add)
 *                                               gcg_scatter_add_rows_f32
 *   data.py:226-250,364-370 graph projection    gcg_project_mention_graph
 *   tensormain.py:170-180 H = D^-1/2 (A+I) D^-1/2  gcg_normalize_adjacency_f32
 *   main.py:530 / tensormain.py:114 X_conv = H * X gcg_spgemm_products + gcg_spgemm
 *   data.py:399-419 assignClasses (kdtree.py)   gcg_kdtree_fit_f64, gcg_segment_medians_f64,
 *                                               gcg_class_medians_f64, gcg_nearest_class_f64
 *   tensormain.py:38-54 geo_eval                gcg_geo_eval_f64 (gcg_haversine_km_f64)
 *   data.py:378-397 DataLoader.tfidf            gcg_tfidf_count, gcg_tfidf_select,
 *                                               gcg_tfidf_compact, gcg_tfidf_weight_f32
 *
 * Conventions (scipy CSR layout, as `scipy.sparse.csr_matrix` holds it):
 *   indptr  int32[n_rows + 1], indices int32[nnz], vals float32[nnz]; dense operands
 *   are row-major float32 with an explicit leading dimension (elements, >= K), K <= 4,194,240.
 *   All pointers are DEVICE pointers (hipMalloc / torch CUDA tensors) unless the
 *   parameter name ends in `_host`. Nothing in the hot path allocates, synchronizes,
 *   or throws; every function returns a gcg_status (0 = ok). `stream` is a
 *   hipStream_t (NULL = the legacy default stream). Calls are reentrant per stream;
 *   the only global state is the per-thread last-error message.
 *
 * Numerics: per output element the products H[r,j]*Z[j,c] are accumulated in
 * CSR storage order, each product and each sum rounded separately (no FMA).
 * That is exactly scipy's `csr_matvecs` (the executor behind the reference's
 * S.dot), so the plan-less and ordered paths match scipy float32 bit for bit.
 * The planned fast path splits rows longer than its task size across waves and
 * adds the per-segment partials in order: equal to scipy within 1e-5 (abs, on
 * normalized-H inputs), not bitwise, for those rows only.
 */
#ifndef GCG_SPMM_H
#define GCG_SPMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gcg_stream_t; /* hipStream_t */

typedef enum {
  GCG_OK = 0,
  GCG_ERR_INVALID_ARG = 1,  /* null pointer, negative or inconsistent size   */
  GCG_ERR_MISALIGNED = 2,   /* pointer not 4-byte aligned                     */
  GCG_ERR_HIP = 3,          /* a HIP runtime call or kernel launch failed     */
  GCG_ERR_ALLOC = 4,        /* host or device allocation failed (plan create) */
  GCG_ERR_BAD_CSR = 5,      /* indptr not monotone / out of range, bad index  */
  GCG_ERR_WORKSPACE = 6     /* workspace missing or too small                 */
} gcg_status;

enum { GCG_ACT_NONE = 0, GCG_ACT_RELU = 1 };

/* Library version, "major.minor.patch". */
const char* gcg_version(void);
/* Content hash of the sources the library was built from (graphconvgeo_amd/_build.py
 * source_hash); the Python binding refuses a library whose hash differs from the tree's. */
const char* gcg_source_hash(void);
/* Text of the last error raised on this host thread ("" if none). */
const char* gcg_last_error(void);

/*
 * Plan-less SpMM, one 64-lane wave per output row, storage-order accumulation:
 *   for i in [0, n_out):  r = out_rows ? out_rows[i] : i
 *       Y[i, 0:K] = act( sum_{j in row r, storage order} vals[j] * Z[indices[j], 0:K] + bias )
 * n_out == n_rows when out_rows == NULL. Bitwise equal to scipy float32 `H @ Z`
 * (rows re-indexed by out_rows). Replaces S.dot at mlpconv.py:71,73,90 and the
 * row gather at mlpconv.py:94. The CSR must be valid (see gcg_csr_validate).
 * Vector width: 16-B gathers when ldz % 4 == 0, ldy % 4 == 0 and Z / Y / bias are 16-B
 * aligned. When K % 4 != 0 they still are (round 4): the last vector of a row also READS Z's
 * columns [K, round4(K)) -- inside the row, since ldz % 4 == 0 means ldz >= round4(K), and
 * never used -- so Z's buffer must extend to column round4(K) of its last row (any [n, ldz]
 * allocation does); bias, Y and gate are never touched past column K.
 */
gcg_status gcg_spmm_csr_f32(int64_t n_rows, int64_t n_cols, int64_t nnz,
                            const int32_t* indptr, const int32_t* indices,
                            const float* vals, const float* Z, int64_t ldz, int64_t K,
                            float* Y, int64_t ldy, const float* bias, int act,
                            const int32_t* out_rows, int64_t n_out,
                            gcg_stream_t stream);

/*
 * nnz-balanced launch plan for one CSR (and one optional output-row list).
 * Built once per H (H is shared by both layers and every epoch, mlpconv.py:214,293),
 * reused for every K. Reads indptr (and out_rows) back to the host once and
 * validates indptr; this call synchronizes `stream` -- it is NOT a hot-path call.
 *   task_nnz  : target nonzeros per wave task (0 = default: clamp(nnz / 8192, 32, 512), ordered
 *               plans clamp(nnz / 32768, 32, 128), or up to 256 when rows average >= 256
 *               nonzeros).
 *   ordered   : 1 = never split a row's sum (bitwise scipy order): rows longer than task_nnz
 *                   are scheduled first, those longer than 8 x task_nnz on a whole workgroup
 *                   each (the storage-order sum handed from wave to wave, still bitwise); one
 *                   also longer than 1/768 of the plan's nonzeros is cut into 2 column slices
 *                   on two workgroups when the launch is two 256-float chunks wide (256 < K
 *                   per 512-float panel, round 5): each slice sums all the row's nonzeros for
 *                   its columns, in storage order -- still bitwise;
 *               2 = ordered with every whole-workgroup row unsliced (A/B and tests);
 *               0 = split rows longer than task_nnz into segments (fast).
 */
typedef struct gcg_spmm_plan gcg_spmm_plan;

gcg_status gcg_spmm_plan_create(gcg_spmm_plan** plan, int64_t n_rows, int64_t n_cols,
                                int64_t nnz, const int32_t* indptr,
                                const int32_t* out_rows, int64_t n_out, int64_t task_nnz,
                                int ordered, gcg_stream_t stream);
gcg_status gcg_spmm_plan_destroy(gcg_spmm_plan* plan);
/* Bytes of device workspace gcg_spmm_csr_f32_planned needs for width K (0 if none). */
gcg_status gcg_spmm_plan_workspace_bytes(const gcg_spmm_plan* plan, int64_t K, size_t* bytes);
/* Plan statistics: tasks, long rows (split into segments in a fast plan, run on a whole
 * workgroup in an ordered plan), segments, max task nnz. */
gcg_status gcg_spmm_plan_info(const gcg_spmm_plan* plan, int64_t* n_tasks, int64_t* n_long_rows,
                              int64_t* n_segments, int64_t* max_task_nnz);
/* Whole-workgroup rows of an ordered plan: all of them, those cut into column slices, and the
 * slices per cut row. Ordered plans need no workspace. */
gcg_status gcg_spmm_plan_hub_rows(const gcg_spmm_plan* plan, int64_t* n_coop_rows,
                                  int64_t* n_sliced_rows, int64_t* n_slices);

/* Planned SpMM: same contract as gcg_spmm_csr_f32; out_rows/n_out come from the plan. */
gcg_status gcg_spmm_csr_f32_planned(const gcg_spmm_plan* plan, const int32_t* indptr,
                                    const int32_t* indices, const float* vals,
                                    const float* Z, int64_t ldz, int64_t K, float* Y,
                                    int64_t ldy, const float* bias, int act, void* workspace,
                                    size_t workspace_bytes, gcg_stream_t stream);

/*
 * The same two SpMMs with the rectify gate written beside Y (act must be GCG_ACT_RELU):
 * gate[i][c] (uint8, row stride ldgate >= K, ldgate % 4 == 0, 4-B aligned base) = 2, 1 or 0
 * for a pre-activation > 0, == 0 or < 0 (NaN: 0) -- twice the factor of Theano's rectify
 * gradient 0.5 * (1 + sgn(x)) (relu = 0.5*(x+|x|), mlpconv.py:77). It replaces keeping the
 * output for the backward mask, and unlike the output it tells an exact-zero pre-activation
 * (gradient g/2) from a negative one (gradient 0). Consumed by gcg_relu_backward_gate_f32.
 */
gcg_status gcg_spmm_csr_f32_gate(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                 const int32_t* indptr, const int32_t* indices,
                                 const float* vals, const float* Z, int64_t ldz, int64_t K,
                                 float* Y, int64_t ldy, const float* bias, int act,
                                 const int32_t* out_rows, int64_t n_out, uint8_t* gate,
                                 int64_t ldgate, gcg_stream_t stream);
gcg_status gcg_spmm_csr_f32_planned_gate(const gcg_spmm_plan* plan, const int32_t* indptr,
                                         const int32_t* indices, const float* vals,
                                         const float* Z, int64_t ldz, int64_t K, float* Y,
                                         int64_t ldy, const float* bias, int act, uint8_t* gate,
                                         int64_t ldgate, void* workspace,
                                         size_t workspace_bytes, gcg_stream_t stream);

/*
 * Planned SpMM with a gather hint (round 3): gather_hint (device, nullable, nnz int32) is the
 * column index array with bit 31 set on every "cold" column -- a column whose Z row the caller
 * expects to be gathered rarely. Cold rows are gathered with non-temporal loads, so they do not
 * displace the hot rows (hub nodes of a power-law graph) from the L2 / Infinity Cache; the
 * result is bitwise the one without the hint (only the cache policy of the loads changes).
 * Used by the dwordx4 launches of up to 512 columns per panel (ldz % 4 == 0 and 16-B aligned
 * Z / Y / bias, any K); every other launch reads `indices`. graphconvgeo_amd.sparse builds the
 * hint (DeviceCSR.gather_hint).
 */
gcg_status gcg_spmm_csr_f32_planned_hint(const gcg_spmm_plan* plan, const int32_t* indptr,
                                         const int32_t* indices, const float* vals,
                                         const float* Z, int64_t ldz, int64_t K, float* Y,
                                         int64_t ldy, const float* bias, int act, uint8_t* gate,
                                         int64_t ldgate, void* workspace,
                                         size_t workspace_bytes, const int32_t* gather_hint,
                                         gcg_stream_t stream);

/*
 * bf16 dense operand (opt-in). gcg_rows_f32_to_bf16 converts n rows of K floats (row stride lds)
 * to bf16 rows (uint16_t storage, row stride ldd >= K) with round-to-nearest-even: NaN stays NaN
 * (the quiet NaN 0x7FC0), +-Inf stays +-Inf, a finite value above the bf16 range rounds to Inf.
 * Destination columns [K, ldd) are written as zero, so a masked last vector of the SpMM never
 * reads garbage. 16-B loads and stores when lds % 4 == 0, ldd % 8 == 0 and both bases are 16-B
 * aligned; any other layout converts element by element (src 4-B, dst 2-B aligned). One pass,
 * allocates nothing.
 *
 * gcg_spmm_csr_bf16z_f32 / _planned: the contracts of gcg_spmm_csr_f32_gate and
 * gcg_spmm_csr_f32_planned_hint with Z stored as bf16:
 *       Y[i, 0:K] = act( sum_{j in row r, storage order} vals[j] * widen(Zb[indices[j], 0:K]) + bias )
 * widen (bf16 -> f32) is exact, product and sum are f32, each rounded, in storage order: for
 * Zr = widen(Zb) the result is bitwise scipy float32 `H @ Zr` (planned: ordered plans; fast plans
 * within 1e-5 of it, bitwise on rows they do not split). vals, bias, Y, the gate bytes and the
 * workspace stay as in the f32 calls (gcg_spmm_plan_workspace_bytes is valid as it is; plans
 * depend on H only and serve both operand types). gate and gather_hint are nullable; the hint's
 * hot set should be sized for the bf16 row bytes.
 * Layout: 16-B gathers (8 bf16 per lane) when ldz % 8 == 0 and Zb is 16-B aligned, ldy % 4 == 0
 * and Y / bias (/ workspace) are 16-B aligned; when K % 8 != 0 the last vector of a row also
 * READS Zb's columns [K, round8(K)) -- inside the row since ldz % 8 == 0, never used. Any other
 * layout (any ldz >= K, Zb 2-B aligned) takes the narrower fallback that gathers single elements:
 * the same result, bitwise. GCG_ERR_INVALID_ARG for ldz < K or ldy < K, GCG_ERR_MISALIGNED for a
 * Zb that is not 2-B or a Y / bias that is not 4-B aligned.
 */
gcg_status gcg_rows_f32_to_bf16(int64_t n, int64_t K, const float* src, int64_t lds,
                                uint16_t* dst, int64_t ldd, gcg_stream_t stream);
gcg_status gcg_spmm_csr_bf16z_f32(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                  const int32_t* indptr, const int32_t* indices,
                                  const float* vals, const uint16_t* Zb, int64_t ldz, int64_t K,
                                  float* Y, int64_t ldy, const float* bias, int act,
                                  const int32_t* out_rows, int64_t n_out, uint8_t* gate,
                                  int64_t ldgate, gcg_stream_t stream);
gcg_status gcg_spmm_csr_bf16z_f32_planned(const gcg_spmm_plan* plan, const int32_t* indptr,
                                          const int32_t* indices, const float* vals,
                                          const uint16_t* Zb, int64_t ldz, int64_t K, float* Y,
                                          int64_t ldy, const float* bias, int act, uint8_t* gate,
                                          int64_t ldgate, void* workspace,
                                          size_t workspace_bytes, const int32_t* gather_hint,
                                          gcg_stream_t stream);

/*
 * Host-only planner (no device memory, no HIP calls): the task list the plan uses,
 * exposed for testing and for host-side tools. `tasks_host` receives n_tasks int32
 * quadruples {a, b, c, d}: c == -4 -> column slice b of d of the row at position a (ordered);
 * otherwise d < 0 -> rows of positions [a, b) (c == -2: one row on a whole workgroup);
 * d >= 0 -> segment of position a covering nonzeros [b, c) into workspace slot d. `long_host` receives
 * n_long quadruples {position, first_slot, n_slots, 0}. Pass NULL buffers to size.
 */
gcg_status gcg_spmm_plan_host(int64_t n_rows, const int32_t* indptr_host,
                              const int32_t* out_rows_host, int64_t n_out, int64_t task_nnz,
                              int ordered, int32_t* tasks_host, int64_t tasks_cap,
                              int64_t* n_tasks, int32_t* long_host, int64_t long_cap,
                              int64_t* n_long, int64_t* n_slots);

/*
 * Device CSR check: indptr[0] == 0, monotone, indptr[n_rows] == nnz, every
 * index in [0, n_cols). Writes 0 (ok) or a gcg_status code to *status_dev
 * (a device int32). Asynchronous on `stream`.
 */
gcg_status gcg_csr_validate(int64_t n_rows, int64_t n_cols, int64_t nnz,
                            const int32_t* indptr, const int32_t* indices,
                            int32_t* status_dev, gcg_stream_t stream);

/*
 * Scatter-add of rows (backward of Y[target_indices] at mlpconv.py:94, where
 * target indices repeat because train indices are drawn with replacement,
 * tensormain.py:226):  for i in [0, n_idx): out[idx[i], 0:K] += src[i, 0:K].
 * Deterministic: duplicates are added in increasing i, via the CSR of idx built
 * by gcg_index_csr (sorted_pos/seg_ptr). `out` is NOT zeroed first.
 */
gcg_status gcg_index_csr(int64_t n_idx, const int32_t* idx, int64_t n_rows, int32_t* seg_ptr,
                         int32_t* sorted_pos, void* workspace, size_t workspace_bytes,
                         size_t* workspace_needed, gcg_stream_t stream);
gcg_status gcg_scatter_add_rows_f32(int64_t n_rows, const int32_t* seg_ptr,
                                    const int32_t* sorted_pos, const float* src, int64_t lds,
                                    int64_t K, float* out, int64_t ldo, gcg_stream_t stream);

/*
 * Rectify backward with the bias gradient in one pass (Theano's grad of
 * rectify(S.dot(H, Z) + b), mlpconv.py:75-77): g = gY where Y > 0 else 0 (g_out may alias gY),
 * bias_grad[c] = sum_r g[r][c] (nullable; deterministic: per-block partials in the workspace,
 * summed in block order). K <= 1024. The workspace (size from _workspace_bytes) is required.
 */
gcg_status gcg_relu_backward_f32_workspace_bytes(int64_t M, int64_t K, size_t* bytes);
gcg_status gcg_relu_backward_f32(int64_t M, int64_t K, const float* gY, int64_t ldg,
                                 const float* Y, int64_t ldy, float* g_out, int64_t ldo,
                                 float* bias_grad /*nullable*/, void* workspace,
                                 size_t workspace_bytes, gcg_stream_t stream);

/*
 * Theano's rectify backward from the gate bytes of gcg_spmm_*_gate, with the bias gradient:
 * g = gY, gY/2 or 0 for gate 2, 1, 0 (the gradient of 0.5*(x+|x|) at x > 0, x == 0, x < 0),
 * bias_grad as gcg_relu_backward_f32 (same workspace size). K <= 1024.
 */
gcg_status gcg_relu_backward_gate_f32(int64_t M, int64_t K, const float* gY, int64_t ldg,
                                      const uint8_t* gate, int64_t ldgate, float* g_out,
                                      int64_t ldo, float* bias_grad /*nullable*/,
                                      void* workspace, size_t workspace_bytes,
                                      gcg_stream_t stream);

/*
 * Dropout (lasagne.layers.DropoutLayer and the reference's SparseInputDropoutLayer,
 * mlpconv.py:37-58, 199-201, 210-211) with a counter-based mask: no mask is stored, every
 * kernel that needs the decision of an element recomputes it from the element's coordinates.
 * Element (i, j) (logical row, logical column) is kept iff
 *     philox4x32_10(counter = (uint32 i, uint32 (j >> 2), uint32 *step_dev, stream_id),
 *                   key = (seed & 0xffffffff, seed >> 32))[j & 3] >= threshold
 * (Philox4x32-10 of Random123: multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 /
 * 0xBB67AE85). threshold = floor(p * 2^32) and scale = 1 / (1 - p) (or 1: rescale off) are
 * computed by the caller. A kept element is fl32(v * scale); a dropped one is written as +0.0
 * (never v * 0: NaN / Inf do not pass a dropped slot). *step_dev is a device int32 read by the
 * kernel, so a captured HIP graph draws a new mask on every replay (the convention of
 * gcg_adam_step_f32). All three calls validate on the host, allocate nothing, and return
 * GCG_OK without a launch on an empty problem.
 *
 * gcg_dropout_f32: Y[r][c] = drop(X[r][c]) for an M x K block whose logical rows are
 * row0 + r and logical columns col_ids ? col_ids[c] : c (col_ids: K device int32, for a block
 * of gathered columns). Y may alias X. Columns >= K of a padded row are never written.
 *
 * gcg_dropout_relu_backward_f32: the backward of drop(rectify(.)) in one pass:
 * t = keep ? fl32(gY * scale) : 0, g = t, t/2, 0 for gate byte 2, 1, 0 (as
 * gcg_relu_backward_gate_f32; gate NULL: g = t), bias_grad = column sums of g (nullable).
 * Same row blocks, partial layout, workspace size (gcg_relu_backward_f32_workspace_bytes) and
 * final reduction as gcg_relu_backward_gate_f32: bitwise what that call gives on the
 * pre-masked gradient. g_out may alias gY. K <= 1024.
 *
 * gcg_csr_dropout_f32: vals_out[k] = drop(vals[k]) for every stored entry of a CSR, structure
 * untouched (dropped entries stay as explicit zeros). transposed = 1: the arrays are CSR(X^T),
 * an entry in storage row r with index c is the logical element (i, j) = (c, r), so X and X^T
 * drop the same elements. vals_out may alias vals. Work is split by nonzeros, not rows.
 */
gcg_status gcg_dropout_f32(int64_t M, int64_t K, const float* X, int64_t ldx, float* Y,
                           int64_t ldy, uint32_t threshold, float scale, uint64_t seed,
                           const int32_t* step_dev, uint32_t stream_id, int64_t row0,
                           const int32_t* col_ids /*nullable*/, gcg_stream_t stream);
gcg_status gcg_dropout_relu_backward_f32(int64_t M, int64_t K, const float* gY, int64_t ldg,
                                         const uint8_t* gate /*nullable*/, int64_t ldgate,
                                         float* g_out, int64_t ldo,
                                         float* bias_grad /*nullable*/, void* workspace,
                                         size_t workspace_bytes, uint32_t threshold, float scale,
                                         uint64_t seed, const int32_t* step_dev,
                                         uint32_t stream_id, int64_t row0, gcg_stream_t stream);
gcg_status gcg_csr_dropout_f32(int64_t n_rows, int64_t n_cols, int64_t nnz,
                               const int32_t* indptr, const int32_t* indices, const float* vals,
                               float* vals_out, int transposed, uint32_t threshold, float scale,
                               uint64_t seed, const int32_t* step_dev, uint32_t stream_id,
                               gcg_stream_t stream);

/*
 * gcg_rectify_backward_wide_f32: the one pass of gcg_relu_backward_gate_f32 and
 * gcg_dropout_relu_backward_f32 for any K (at most 65535 * 1024): the backward of a hidden
 * layer wider than 1024 units. step_dev NULL: no mask (g = gY, gY/2, 0 by the gate byte; the
 * other dropout arguments are ignored); step_dev given: t = keep ? fl32(gY * scale) : 0 first,
 * and gate may then be NULL (g = t). Neither a gate nor a mask is GCG_ERR_INVALID_ARG: plain
 * column sums are gcg_column_sum_f32's.
 *
 * The slab rule: the columns are cut into slabs of 1024, and slab s (columns 1024 s .. ) is
 * processed exactly as the narrow entries process a matrix of that slab's columns -- the same
 * row blocks, wave interleave, accumulation order and per-block partials, then the same final
 * reduction -- with the mask of logical column 1024 s + c, i.e. the one gcg_dropout_f32 applied
 * to the whole row. So g is what the rule above states element by element, and
 * bias_grad[1024 s .. ] is bitwise gcg_column_sum_f32 of that slab of g. For K <= 1024 the
 * results are bitwise the narrow entries'.
 *
 * Workspace: gcg_relu_backward_f32_workspace_bytes(M, K), required. Alignment as the narrow
 * entries: 4-B bases; K > 256 needs 16-B aligned rows (16-B bases, ldg % 4 == 0, ldo % 4 == 0),
 * else GCG_ERR_MISALIGNED; the gate a 4-B base and ldgate % 4 == 0. g_out may alias gY.
 * M == 0 zeroes bias_grad.
 */
gcg_status gcg_rectify_backward_wide_f32(int64_t M, int64_t K, const float* gY, int64_t ldg,
                                         const uint8_t* gate /*nullable*/, int64_t ldgate,
                                         float* g_out, int64_t ldo,
                                         float* bias_grad /*nullable*/, void* workspace,
                                         size_t workspace_bytes, uint32_t threshold, float scale,
                                         uint64_t seed, const int32_t* step_dev /*nullable*/,
                                         uint32_t stream_id, int64_t row0, gcg_stream_t stream);

/*
 * Column sums out[c] = sum_r X[r][c] (the bias gradient of a dense projection, colsum of the
 * logits gradient; Theano's grad of T.dot(h, W) + b, mlpconv.py:88-93), deterministic, same
 * kernels and workspace (gcg_relu_backward_f32_workspace_bytes) as gcg_relu_backward_f32.
 */
gcg_status gcg_column_sum_f32(int64_t M, int64_t K, const float* X, int64_t ldx, float* out,
                              void* workspace, size_t workspace_bytes, gcg_stream_t stream);

/*
 * lasagne.updates.adam (mlpconv.py:263) for one float32 parameter of n elements, in place:
 *   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= a_t*m / (sqrt(v) + eps),
 * with a_t = lr*sqrt(1-b2^t)/(1-b1^t) read from the device scalar *step_dev (so the call can
 * sit inside a captured HIP graph and be replayed with a new step size).
 */
gcg_status gcg_adam_step_f32(int64_t n, float* p, const float* g, float* m, float* v,
                             const float* step_dev, float beta1, float beta2, float eps,
                             gcg_stream_t stream);

/*
 * lasagne.updates.adamax (loc2lang.py:207) for one float32 parameter of n elements, in place and
 * in one pass:
 *   m = b1*m + (1-b1)*g;  u = max(b2*u, |g|);  p -= a_t*m / (u + eps),
 * with a_t = lr/(1-b1^t) read from the device scalar *step_dev, as gcg_adam_step_f32 reads its
 * step size. Returns GCG_OK without a launch when n == 0.
 */
gcg_status gcg_adamax_step_f32(int64_t n, float* p, const float* g, float* m, float* u,
                               const float* step_dev, float beta1, float beta2, float eps,
                               gcg_stream_t stream);

/*
 * The weight penalty of the MLPCONV loss (mlpconv.py:235-243: lasagne.regularization l1 =
 * sum|W|, l2 = sum W^2, scaled by regul_coef * share) for one float32 weight of n elements:
 *   *out = ((acc_in ? *acc_in : 0) + l1 * sum|W|) + l2 * sum W^2
 * acc_in (nullable, may alias out) chains the weights of one loss in order. Deterministic
 * (fixed grid, partials added in order); workspace >= GCG_L1L2_WORKSPACE_BYTES device bytes.
 * gcg_l1l2_grad_f32 writes its gradient dW = s * (l1 * sgn(W) + 2 * l2 * W), sgn(0) = 0 (Theano's
 * grad of abs), s = *scale_dev (the upstream gradient, a device scalar) or 1 when NULL.
 */
#define GCG_L1L2_WORKSPACE_BYTES 2048
gcg_status gcg_l1l2_penalty_f32(int64_t n, const float* W, float l1, float l2,
                                const float* acc_in, float* out, void* workspace,
                                size_t workspace_bytes, gcg_stream_t stream);
gcg_status gcg_l1l2_grad_f32(int64_t n, const float* W, float l1, float l2,
                             const float* scale_dev, float* dW, gcg_stream_t stream);

/*
 * The mini-batch MLP trainer (reference mlp.py:96-311: a sparse-input MLP trained on shuffled
 * mini-batches, mlp.py:77-92, 268-270; driven by tensormain.py:141-149 on X_conv = H * X).
 *
 * gcg_minibatch_segment: the column grouping of all the batches of an epoch (or of a run of its
 * batches) at once. perm (device, n_sel = n_batches * batch row ids of X, the epoch's order
 * with its tail dropped) cuts into n_batches consecutive batches. For batch b it produces the
 * segments batch_seg_ptr[b] .. batch_seg_ptr[b + 1] of one global segment list: segment s has
 * the column seg_col[s] (ascending inside a batch) and the entries seg_ptr[s] .. seg_ptr[s + 1];
 * entry e is (ent_pos[e] = the row's position in its batch, in [0, batch); ent_val[e]). Inside
 * a segment the entries keep batch order and, within one row, storage order -- the stable order
 * of scipy's X[rows].T.tocsr() (duplicate entries stay separate, empty rows give none).
 *   nnz_sel   the number of stored entries of the selected rows, known on the host (X's indptr
 *             is there); it sizes the entry arrays and the launches. Slots past the rows' real
 *             total end up outside every batch's range, entries past nnz_sel are dropped; a row
 *             id outside [0, n_rows) counts as an empty row.
 *   sizes     batch_seg_ptr int32[n_batches + 1], seg_col int32[seg_capacity], seg_ptr
 *             int32[seg_capacity + 1], ent_pos int32[nnz_sel], ent_val float32[nnz_sel];
 *             seg_capacity = min(nnz_sel, n_batches * n_cols) + 1 and the workspace size come
 *             from gcg_minibatch_segment_sizes (either output may be NULL; seg_capacity is host
 *             arithmetic, workspace_bytes asks hipcub and so needs a HIP device: rocPRIM sizes
 *             its temporary per architecture). The number of segments stays on the device.
 * The sort key is batch * n_cols + column in 32 bits: n_batches * n_cols >= 2^32 - 1 (or more
 * than INT32_MAX entries) is GCG_ERR_INVALID_ARG. Asynchronous on `stream`: no allocation, no
 * host synchronisation.
 *
 * gcg_minibatch_w1_step_f32: the whole update of the sparse-input weight W (F x K, contiguous)
 * for one mini-batch in one pass over W, m, v -- no F x K gradient exists. For every element
 *     d = sum over the entries e of row r's segment, in order, of ent_val[e] * G[ent_pos[e]][c]
 *         (from +0.0, product and sum rounded separately; +0.0 for a row without a segment)
 *     g = d + (l1 * sgn(w) + 2 * l2 * w)            the expression of gcg_l1l2_grad_f32, s = 1
 *     m, v, w updated as gcg_adam_step_f32 does     a_t read from *step_dev
 * -- bitwise the composition of (X[batch])^T . G scattered into zeros, gcg_l1l2_grad_f32 and
 * gcg_adam_step_f32, and reproducible (no atomics). G: batch x K gradient of the layer's
 * pre-activation (ldg >= K); seg_range: device int32[2], this batch's segment range
 * (batch_seg_ptr + b); the other arrays as gcg_minibatch_segment wrote them. 16-B accesses when
 * K % 4 == 0, ldg % 4 == 0 and W, m, v, G are 16-B aligned, dword accesses otherwise (any K).
 */
gcg_status gcg_minibatch_segment_sizes(int64_t n_sel, int64_t batch, int64_t n_cols,
                                       int64_t nnz_sel, int64_t* seg_capacity,
                                       size_t* workspace_bytes);
gcg_status gcg_minibatch_segment(int64_t n_rows, int64_t n_cols, const int32_t* indptr,
                                 const int32_t* indices, const float* vals, const int32_t* perm,
                                 int64_t n_sel, int64_t batch, int64_t nnz_sel,
                                 int32_t* batch_seg_ptr, int32_t* seg_col, int32_t* seg_ptr,
                                 int32_t* ent_pos, float* ent_val, void* workspace,
                                 size_t workspace_bytes, gcg_stream_t stream);
gcg_status gcg_minibatch_w1_step_f32(int64_t F, int64_t K, float* W, float* m, float* v,
                                     const float* G, int64_t ldg, int64_t batch,
                                     const int32_t* seg_range, const int32_t* seg_col,
                                     const int32_t* seg_ptr, const int32_t* ent_pos,
                                     const float* ent_val, float l1, float l2,
                                     const float* step_dev, float beta1, float beta2, float eps,
                                     gcg_stream_t stream);

/*
 * gcg_minibatch_w1_adamax_step_f32: the same pass with the second update rule, for the sparse
 * (grid) first layer of loc2lang's no-MDN baseline, which trains with Adamax and no penalty:
 *     d as above;  m, u, w updated as gcg_adamax_step_f32 does with g = d
 * -- bitwise the composition of (X[batch])^T . G scattered into zeros and gcg_adamax_step_f32.
 * Every row whose m is non-zero moves on every step, so the pass covers all of W here too. The
 * kernel is gcg_minibatch_w1_step_f32's, instantiated on the rule; arguments and vector widths
 * as there.
 */
gcg_status gcg_minibatch_w1_adamax_step_f32(int64_t F, int64_t K, float* W, float* m, float* u,
                                            const float* G, int64_t ldg, int64_t batch,
                                            const int32_t* seg_range, const int32_t* seg_col,
                                            const int32_t* seg_ptr, const int32_t* ent_pos,
                                            const float* ent_val, const float* step_dev,
                                            float beta1, float beta2, float eps,
                                            gcg_stream_t stream);

/*
 * gcg_minibatch_segment_dropout: gcg_minibatch_segment with input dropout on X (the reference's
 * SparseInputDropoutLayer in front of a mini-batch trainer, lang2loc.py:280-281), the dropout
 * parameters of gcg_csr_dropout_f32 appended. Every selected entry is masked with the keep rule
 * above: logical row = the row's id in X, logical column = its column, step = *step_dev + the
 * batch's index in the call (so one call draws an independent mask per batch, and the host
 * advances its step counter by n_batches afterwards). The masked value -- keep ? fl32(v * scale)
 * : +0.0 -- is written twice: as the entry's ent_val (the W1 step sees the masked batch) and
 * into vals_drop (float32[nnz of X]) at the entry's own CSR slot, so the forward of batch b is
 * gcg_spmm_csr_f32_gate(indptr, indices, vals_drop, out_rows = the batch's rows). Each row of an
 * epoch's order is in at most one batch, so one vals_drop serves every batch of the call; slots
 * of rows outside perm are not written. Dropped entries stay explicit zeros; the segment
 * structure (batch_seg_ptr, seg_col, seg_ptr, ent_pos) is bitwise gcg_minibatch_segment's.
 * Sizes and workspace as gcg_minibatch_segment (gcg_minibatch_segment_sizes).
 */
gcg_status gcg_minibatch_segment_dropout(int64_t n_rows, int64_t n_cols, const int32_t* indptr,
                                         const int32_t* indices, const float* vals,
                                         const int32_t* perm, int64_t n_sel, int64_t batch,
                                         int64_t nnz_sel, int32_t* batch_seg_ptr, int32_t* seg_col,
                                         int32_t* seg_ptr, int32_t* ent_pos, float* ent_val,
                                         float* vals_drop, void* workspace, size_t workspace_bytes,
                                         uint32_t threshold, float scale, uint64_t seed,
                                         const int32_t* step_dev, uint32_t stream_id,
                                         gcg_stream_t stream);

/*
 * The mixture-density location head (reference lang2loc.py:143-244): a network output row of
 * 6 * C float32 values read as a mixture of C bivariate Gaussians over (lat, lon). The layout is
 * the reference's output.reshape(-1, 6, C): row r of O (B x 6C, row stride ldo >= 6C) holds six
 * planes of C columns,
 *     plane 0, 1   means         mu    = (90, 180) * tanh(.)
 *     plane 2, 3   sigmas        sigma = 10 * softplus(.)
 *     plane 4      correlation   rho   = softsign(.) = t / (1 + |t|)
 *     plane 5      mixture logits   pi = softmax(.) over the C components
 * with 1 <= C <= 1024. softplus is evaluated as max(x, 0) + log1p(exp(-|x|)), log pi as
 * log-softmax, and 1 - rho^2 from the raw value as (1 + 2|t|) / (1 + |t|)^2: the same functions
 * as the reference's expressions wherever those are finite, without their overflow (softplus,
 * log(softmax)) and cancellation (1 - rho^2 as |rho| -> 1). Arithmetic is float32 with the
 * device library's expf / logf / log1pf / tanhf (no fast intrinsics), with one exception in
 * gcg_mdn_nll_f32: the difference y - mu is formed in double (tanh included) and rounded once,
 * because mu rounded to float32 (|mu| up to 180) is off by up to 8e-6 and y - mu amplifies that
 * as a mean closes in on its target. The calls validate on the host, allocate nothing, and
 * return GCG_OK without a launch when B == 0.
 *
 * gcg_mdn_nll_f32: the negative log-likelihood of Y (B x 2 float32, contiguous: lat, lon) and
 * its gradient (lang2loc.py:166-196). With d = y - mu, u_i = d_i / sigma_i,
 *     z_c = u1^2 + u2^2 - 2 rho u1 u2
 *     e_c = -z_c / (2 (1 - rho^2)) - log(2 pi) - log(sigma1 sigma2) - log(1 - rho^2) / 2 + log pi_c
 *     loss_r = -logsumexp_c(e_c)
 * One launch computes every row's loss and gradient: one wave per row, lanes striding over the
 * components, the wave reductions by __shfl in a fixed order. loss_rows (nullable) receives
 * loss_r; *loss (device scalar) the mean, reduced by a second one-workgroup launch in a fixed
 * order with no atomics -- thread t of 256 adds the rows t, t + 256, ... in order, the 256
 * partials are added by a halving tree (p[t] += p[t + h], h = 128 .. 1), the sum is divided by
 * B -- so it is reproducible bit for bit. dO (B x 6C, row stride ldd >= 6C; NULL: no gradient,
 * for validation) receives s / B * d loss_r / d O[r][.], s = *scale_dev (the upstream gradient,
 * a device scalar) or 1 when NULL -- the convention of gcg_l1l2_grad_f32. workspace: B floats,
 * needed only when loss_rows is NULL (the row losses the mean is taken of live there).
 *
 * gcg_mdn_unpack_f32: the four arrays of the reference's f_predict, contiguous float32:
 * mus [B, 2, C], sigmas [B, 2, C], corxy [B, C], pis [B, C] -- computed with the device
 * functions the other two calls use, so gcg_mdn_predict_f32's latlon is bitwise a mus entry.
 *
 * gcg_mdn_predict_f32: the reference's pred (lang2loc.py:198-244). method 0 ("mixture"): every
 * component mean mu_c of a row is a candidate, its score the mixture density there,
 *     sum_k pi_k / (2 pi sigma1_k sigma2_k sqrt(1 - rho_k^2)) * exp(-z_ck / (2 (1 - rho_k^2)))
 * summed over k ascending in float32 (non-log form; the candidate's own component contributes
 * exp(0), so the score is positive unless its weight underflows); method 1 ("pi"): the score is
 * the component's logit. idx[r] (int32, nullable) is the first maximiser (numpy.argmax: the
 * lower index on a tie), latlon[r] = (mu_lat, mu_lon) of it (float32 B x 2). One workgroup per
 * row, the row's six transformed planes staged once in LDS (24 C bytes); C^2 evaluations per row.
 */
gcg_status gcg_mdn_nll_f32(int64_t B, int64_t C, const float* O, int64_t ldo, const float* Y,
                           const float* scale_dev /*nullable*/, float* dO /*nullable*/,
                           int64_t ldd, float* loss_rows /*nullable*/, float* loss,
                           void* workspace /*nullable*/, size_t workspace_bytes,
                           gcg_stream_t stream);
gcg_status gcg_mdn_unpack_f32(int64_t B, int64_t C, const float* O, int64_t ldo, float* mus,
                              float* sigmas, float* corxy, float* pis, gcg_stream_t stream);
gcg_status gcg_mdn_predict_f32(int64_t B, int64_t C, const float* O, int64_t ldo, int method,
                               int32_t* idx /*nullable*/, float* latlon, gcg_stream_t stream);

/*
 * The shared-component mixture-density model (reference lang2loc_mdnshared.py:306-327, 379-414,
 * 482-487; lasagne_layers.MDNSharedParams): one set of C bivariate Gaussians for the whole
 * model, 1 <= C <= 1024, held as float32 parameters
 *     mus [C, 2]          means (lat, lon), used as they are
 *     sigmas_raw [C, 2]   sigma = softplus(.)            (no factor 10)
 *     corxy_raw [C]       rho   = softsign(.) = t / (1 + |t|)
 * all contiguous; the network gives only the mixture logits L (B x C, row stride ldl >= C),
 * pi = softmax(L) over the C components. softplus, log pi and q = 1 - rho^2 are evaluated in the
 * stable forms stated above for the per-row head; the difference d_i = y_i - mus[c][i] is plain
 * float32 (the mean is a parameter, exact in float32, not a rounded tanh). Arithmetic is float32
 * as for the per-row head, with one exception in gcg_mdn_shared_nll_f32: e_rc is formed in
 * double -- s, rho, q and the row-independent part of e once per call from the raw parameters,
 * u_i = d_i / s_i, z and e per row -- its maximum over the row is taken in double, and e - max
 * is rounded to float32 once. Two components that compete for a row have |e| of 30 .. 1e4
 * there and their responsibilities hang on the difference; a float32 e leaves ulp(|e|) in it.
 * The exponentials, the sums and the gradient terms are float32. The calls validate on the
 * host, allocate nothing, use no atomics, and return GCG_OK without a launch when B == 0.
 *
 * gcg_mdn_shared_nll_f32: with s_i = sigma_i, u_i = d_i / s_i,
 *     z_rc = u1^2 + u2^2 - 2 rho u1 u2
 *     e_rc = -0.5 z_rc / q - log(2 pi) - log s1 - log s2 - 0.5 log q + log_softmax(L_r)_c
 *     loss_r = -logsumexp_c(e_rc),   w_rc = exp(e_rc - max_c) / sum_c   (the responsibility)
 * loss_rows (nullable) receives loss_r and *loss (device scalar) the mean, in the fixed order of
 * gcg_mdn_nll_f32. dL (B x C, row stride lddl >= C, nullable) receives s / B * (pi - w),
 * s = *scale_dev or 1 when NULL. dparams (nullable) receives the gradient of s * mean loss in
 * five planes of C: d mus lat, d mus lon, d sigmas_raw lat, d sigmas_raw lon, d corxy_raw. With
 * a_1 = (u1 - rho u2) / q, a_2 = (u2 - rho u1) / q the sums over the rows are
 *     sum_r w a_i / s_i,   sum_r w (u_i a_i - 1) / s_i,   sum_r w (u1 u2 + rho (1 - z / q)) / q
 * times -s / B, -s / B * sigmoid(sigmas_raw), -s / B / (1 + |corxy_raw|)^2, the factors applied
 * once after the sum. The order of every sum is fixed, so the result is reproducible bit for bit:
 * with R = 4 * max(1, ceil(B / 2048)) rows per workgroup (a function of B alone; at most 512
 * workgroups), workgroup g takes the rows [g R, (g + 1) R) and its wave w (of 4) the R / 4 rows
 * from g R + w R / 4, one row at a time with the lanes across the components. A lane adds its
 * components' terms in row order; the four waves are added as ((w0 + w1) + w2) + w3; a second
 * launch adds the workgroups' partials in ascending g and applies the factors. loss_rows[r] and
 * dL[r] depend on row r alone, not on B or the grouping (s / B aside).
 * workspace: gcg_mdn_shared_nll_f32_workspace_bytes(B, C) bytes, 8-byte aligned, always required
 * (the components' constants, the workgroups' partials, and the row losses when loss_rows is
 * NULL).
 *
 * gcg_mdn_shared_density_f32: Dt (C x C, contiguous), Dt[j C + i] = the density of component j
 * at the mean of component i,
 *     1 / (2 pi s1_j s2_j sqrt(q_j)) * exp(-(v1^2 + v2^2 - 2 rho_j v1 v2)),
 *     v_i = (mus[i] - mus[j]) * sqrt(0.5 / q_j) / s_j
 * (gcg_mdn_predict_f32's factoring): C^2 exponentials once per parameter set, not per row.
 *
 * gcg_mdn_shared_predict_f32: the reference's pred_sharedparams. method 0 ("mixture"):
 * score[r][i] = sum_j pi[r][j] * Dt[j C + i], summed over j ascending in float32, with
 * pi = exp(L - max) / sum (lane l of a wave adds the components l, l + 64, ..., then a butterfly
 * over the wave); method 1 ("pi"): the score is the logit (Dt may be NULL). idx[r] (int32,
 * nullable) is the first maximiser (the lower index on a tie; component 0 when every score is
 * NaN) and latlon[r] (float32 B x 2) = mus[idx[r]], copied bit for bit. A workgroup takes a tile
 * of 4 rows and reads each Dt element once for the tile; a row's result does not depend on the
 * tile or the grid.
 */
gcg_status gcg_mdn_shared_nll_f32_workspace_bytes(int64_t B, int64_t C, size_t* bytes);
gcg_status gcg_mdn_shared_nll_f32(int64_t B, int64_t C, const float* L, int64_t ldl,
                                  const float* Y, const float* mus, const float* sigmas_raw,
                                  const float* corxy_raw, const float* scale_dev /*nullable*/,
                                  float* dL /*nullable*/, int64_t lddl,
                                  float* dparams /*nullable*/, float* loss_rows /*nullable*/,
                                  float* loss, void* workspace, size_t workspace_bytes,
                                  gcg_stream_t stream);
gcg_status gcg_mdn_shared_density_f32(int64_t C, const float* mus, const float* sigmas_raw,
                                      const float* corxy_raw, float* Dt, gcg_stream_t stream);
gcg_status gcg_mdn_shared_predict_f32(int64_t B, int64_t C, const float* L, int64_t ldl,
                                      const float* Dt /*nullable for method 1*/,
                                      const float* mus, int method, int32_t* idx /*nullable*/,
                                      float* latlon, gcg_stream_t stream);

/*
 * The Gaussian layer of the inverse model (reference loc2lang.py:174; lasagne_layers.py:156-214,
 * BivariateGaussianLayer): the C Gaussians of the shared-component model above -- the same three
 * parameter tensors, transforms and stable forms, 1 <= C <= 1024 -- as a layer over coordinates
 * X (B x 2 float32, contiguous: lat, lon). With u_i = (x_i - mus[c][i]) / s_i,
 *     z = u1^2 + u2^2 - 2 rho u1 u2
 *     G[r][c] = exp(-log(2 pi) - log s1 - log s2 - 0.5 log q - 0.5 z / q)
 * the reference's log-domain form (lasagne_layers.py:207-212). Both calls compute in double from
 * the float32 inputs -- the constants once per component from the raw parameters, and per
 * element the difference x - mu (exact), u, z, the exponent, the exponential and the gradient
 * terms -- and round a result to float32 once. Unlike the responsibilities of the NLL, an
 * upstream dG has either sign, and a parameter's sum over the rows may cancel by orders of
 * magnitude; float32 terms would leave their rounding in what remains. The calls validate on the
 * host, allocate nothing, use no atomics, and return GCG_OK without a launch when B == 0.
 *
 * gcg_bigaus_layer_f32: G (B x C, row stride ldg >= C). G[r][c] depends on row r and component
 * c alone, not on B, ldg or the grid.
 *
 * gcg_bigaus_layer_backward_f32: dparams receives the gradient of the three parameter tensors
 * from an upstream dG (B x C, row stride lddg >= C), in gcg_mdn_shared_nll_f32's five planes of
 * C (d mus lat, d mus lon, d sigmas_raw lat, d sigmas_raw lon, d corxy_raw). G is recomputed as
 * the forward computes it, so no stride of it needs agreeing. With a_1 = (u1 - rho u2) / q,
 * a_2 = (u2 - rho u1) / q the sums over the rows are
 *     sum_r dG G a_i / s_i,   sum_r dG G (u_i a_i - 1) / s_i,
 *     sum_r dG G (u1 u2 + rho (1 - z / q)) / q
 * times s, s * sigmoid(sigmas_raw), s / (1 + |corxy_raw|)^2, s = *scale_dev or 1 when NULL, the
 * factors applied once after the sum. X has no gradient. The order of every sum is fixed: the
 * rows are grouped as in gcg_mdn_shared_nll_f32, R = 4 * max(1, ceil(B / 2048)) rows per
 * workgroup (a function of B alone; at most 512 workgroups), workgroup g the rows
 * [g R, (g + 1) R). Within a workgroup a component belongs to one thread, which adds its terms
 * over the workgroup's rows in row order -- the double accumulators of all components do not fit
 * a wave's registers at C = 1024, so the components, not the rows, are spread over the four
 * waves and no sum crosses a wave. A second launch adds the workgroups' partials in ascending g,
 * applies the factor and rounds to float32. dparams is reproducible bit for bit.
 * workspace: gcg_bigaus_layer_backward_f32_workspace_bytes(B, C) bytes, 8-byte aligned (the
 * components' constants and the workgroups' partials, doubles).
 */
gcg_status gcg_bigaus_layer_f32(int64_t B, int64_t C, const float* X, const float* mus,
                                const float* sigmas_raw, const float* corxy_raw, float* G,
                                int64_t ldg, gcg_stream_t stream);
gcg_status gcg_bigaus_layer_backward_f32_workspace_bytes(int64_t B, int64_t C, size_t* bytes);
gcg_status gcg_bigaus_layer_backward_f32(int64_t B, int64_t C, const float* X, const float* mus,
                                         const float* sigmas_raw, const float* corxy_raw,
                                         const float* dG, int64_t lddg,
                                         const float* scale_dev /*nullable*/, float* dparams,
                                         void* workspace, size_t workspace_bytes,
                                         gcg_stream_t stream);

/*
 * Softmax cross-entropy of wide logits rows against sparse soft targets (reference
 * loc2lang.py:193-196 on the bag of words of loc2lang.py:253, which it densifies per batch).
 * logits: M x N float32, row stride ldl >= N, 1 <= N <= 2^24; the columns [N, ldl) are never
 * read. The target Y is a CSR of y_rows x N (int32 y_indptr / y_indices, float32 y_vals); row i
 * of the logits is paired with row rows[i] of Y (rows: M device int32, may repeat, any order),
 * or with row i when rows is NULL (then y_rows >= M). With
 *     lse = max + log sum_j exp(z_j - max),   T = sum_k y_k   over the entries of the paired row
 *     loss_rows[i] = sum_k y_k * (lse - z[col_k])
 *     out[i][j]    = s * (T * softmax(z)_j - y_ij),   s = scale * (*scale_dev or 1 when NULL)
 * which is the reference's -sum_j y_j log softmax(z)_j and its gradient wherever that is finite
 * (0 * log 0 does not arise here). An empty target row gives loss 0 and a zero gradient row.
 * y_indptr == NULL: out = softmax(logits) (predict; loss_rows is not written). out == NULL: the
 * losses only (evaluation). out (M x N, row stride ldo >= N) may be the logits themselves: every
 * z[col_k] is read before the row is overwritten.
 * One workgroup of 256 threads owns a row: (1) one pass over the row with 16-B loads (4-B loads
 * where the row is not 16-B aligned, same values) in which thread t folds the column quads
 * t, t + 256, ... in order into a running (max, sum) pair -- per quad its maximum first, one
 * rescale of the sum, then the four terms in column order -- the lanes' pairs merged by an xor
 * butterfly (32, 16, .., 1) and the four waves' as ((w0 + w1) + w2) + w3, a merge being
 * max = max(m1, m2), sum = s1 exp(m1 - max) + s2 exp(m2 - max); (2) the loss gather, thread t
 * adding the entries t, t + 256, ... of the target row, lanes by the butterfly and waves in
 * order; (3) a second pass over the row (cache-resident up to a few 10^5 columns) that writes
 * s T softmax; (4) after a workgroup barrier the same workgroup subtracts s y_k at column col_k.
 * The order is a fixed function of N: a row's results do not depend on M, the grid or its
 * position, and two calls agree bit for bit. No atomics.
 * The rows of Y must be free of duplicate columns: step (4) is a plain read-modify-write, and of
 * two entries on one column one update would be lost. An entry whose column is outside [0, N) is
 * skipped, and a row whose rows[i] is outside [0, y_rows) gets a NaN loss and a zero gradient
 * row; neither is ever used as an index. y_indptr itself (monotone, within the arrays) is the
 * caller's to validate (gcg_csr_validate). Validates on the host, allocates nothing, returns
 * GCG_OK without a launch when M == 0.
 */
gcg_status gcg_softmax_xent_csr_f32(int64_t M, int64_t N, const float* logits, int64_t ldl,
                                    int64_t y_rows, const int32_t* y_indptr /*nullable*/,
                                    const int32_t* y_indices, const float* y_vals,
                                    const int32_t* rows /*nullable*/, float scale,
                                    const float* scale_dev /*nullable*/, float* out /*nullable*/,
                                    int64_t ldo, float* loss_rows, gcg_stream_t stream);

/*
 * What the analyses of the location-to-language model need of a chunk of logits (reference
 * loc2lang.py:516-614 state_dialect_words, 755-766 get_local_words): the row log-sum-exp and,
 * per word, two column sums of p = softmax(z). The M x N probabilities are never written.
 * logits: M x N float32, row stride ldl >= N, 1 <= N <= 2^24; the columns [N, ldl) are never
 * read. Both calls validate on the host, allocate nothing, use no atomics, and return GCG_OK
 * without a launch when M == 0.
 *
 * gcg_row_lse_f64: lse[i] = max_j z_ij + log sum_j exp(z_ij - max), float64[M]. One workgroup of
 * 256 threads owns a row and folds it as gcg_softmax_xent_csr_f32's first pass does (the same
 * code: a float32 running (max, sum) pair per thread over the column quads t, t + 256, ..., the
 * lanes merged by an xor butterfly, the waves as ((w0 + w1) + w2) + w3; 4-B loads of the same
 * values where the row is not 16-B aligned); the final log and the final add are in double. A
 * row's result is a fixed function of its N values: it does not depend on M, the grid, the row's
 * position or its alignment, and two calls agree bit for bit. A row holding NaN or +inf gives
 * NaN, a row of -inf gives -inf, and no other row is affected.
 *
 * gcg_softmax_column_stats_f64: S and T are float64[N] and are accumulated INTO -- the caller
 * zeroes them before the first chunk. For every column j, and the rows i = 0 .. M - 1 in
 * ascending order, with a = double(z_ij) - lse[i] and p = exp(a) in double:
 *     S[j] = S[j] + p;     T[j] = T[j] + (p > 0 ? p * a : 0)
 * (a logit of -inf, or an underflow, contributes 0 log 0 = 0, as scipy.stats.entropy counts it).
 * The entropy of the l1-normalised column is then log S - T / S. A column belongs to one thread
 * (64 consecutive columns to a wave, one wave per workgroup), which adds the rows one at a time
 * in row order onto the value it read from S[j] / T[j]: any split of the rows into consecutive
 * calls leaves S and T bitwise equal to one call over all of them, whatever the chunk size. The
 * loads of 8 rows are in flight while the previous 8 are added. lse: float64[M], e.g. from
 * gcg_row_lse_f64 on the same rows; a NaN lse[i] (a non-finite row) makes S NaN in every column.
 */
gcg_status gcg_row_lse_f64(int64_t M, int64_t N, const float* logits, int64_t ldl, double* lse,
                           gcg_stream_t stream);
gcg_status gcg_softmax_column_stats_f64(int64_t M, int64_t N, const float* logits, int64_t ldl,
                                        const double* lse, double* S, double* T,
                                        gcg_stream_t stream);

/*
 * CSR transpose on the device (CSR(X^T) for the X^T . dZ1 gradient of
 * mlpconv.py:71). Output is sorted by (row, col) with stable order for equal
 * entries. out_indptr int32[n_cols+1], out_indices int32[nnz], out_vals f32[nnz].
 */
gcg_status gcg_csr_transpose_f32(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                 const int32_t* indptr, const int32_t* indices,
                                 const float* vals, int32_t* out_indptr, int32_t* out_indices,
                                 float* out_vals, void* workspace, size_t workspace_bytes,
                                 size_t* workspace_needed, gcg_stream_t stream);

/*
 * Graph operator on the device (tensormain.py:170-180): from an undirected edge list
 * (u[e], v[e]) build H = D^-1/2 (A + I) D^-1/2 as a canonical CSR (rows and columns
 * sorted; duplicate edges collapse to one binary entry, as networkx stores one edge per
 * pair). H_ij = float32(float64(d_i^-1/2) * float64(d_j^-1/2)) with d = row degree incl.
 * the self loop: bitwise the reference's float64 D*adj*D product after .astype(float32)
 * (tensormain.py:221). Capacity: indices/vals hold 2*n_edges + n entries; the actual nnz
 * is written to *nnz_dev (device int64). *status_dev = GCG_ERR_BAD_CSR on an endpoint out
 * of [0, n). Pass all-NULL outputs to size the workspace.
 */
gcg_status gcg_normalize_adjacency_f32(int64_t n, int64_t n_edges, const int32_t* u,
                                       const int32_t* v, int self_loops, int32_t* indptr,
                                       int32_t* indices, float* vals, int64_t* nnz_dev,
                                       void* workspace, size_t workspace_bytes,
                                       size_t* workspace_needed, int32_t* status_dev,
                                       gcg_stream_t stream);

/*
 * SpGEMM C = A . B for the host "input convolution" X_conv = H * X (main.py:530,
 * tensormain.py:114; then .tocsr().astype('float32')). A: m x n CSR (values float32, or
 * float64 when a_is_f64 -- the reference's H is float64 there), B: n x p CSR float32.
 * Every C entry is summed in scipy csr_matmat's traversal order (A row order, then B row
 * order), each product and sum rounded in the accumulation type (accumulate_f64 = 1:
 * float64, the reference's H64 * X32 upcast), exact zero sums dropped (as scipy), then
 * rounded to float32. Output CSR is canonical (sorted columns), as astype() leaves it.
 * Step 1: gcg_spgemm_products -> number of products P (synchronizes). Step 2: gcg_spgemm
 * with c_idx/c_val of capacity P, c_ptr of m+1; actual nnz to *nnz_c_dev (<= INT32_MAX).
 * Not a hot-path call: it allocates stream-ordered temporaries and synchronizes. The
 * row-wise path (p within 8 LDS slabs) uses c_idx/c_val themselves as its products-sized
 * scratch (C rows written at their product offsets, then compacted in place), so it only
 * allocates ~30 B per row of A; the expand-sort-reduce path used for wider p allocates ~40 B
 * per product per 2^29-product row chunk. Entries of c_idx/c_val past nnz(C) are undefined.
 */
gcg_status gcg_spgemm_products(int64_t m, int64_t nnz_a, const int32_t* a_ptr, const int32_t* a_idx,
                               int64_t n, const int32_t* b_ptr, int64_t* n_products,
                               gcg_stream_t stream);
gcg_status gcg_spgemm(int64_t m, int64_t n, int64_t p, int64_t nnz_a, const int32_t* a_ptr,
                      const int32_t* a_idx, const void* a_val, int a_is_f64, int64_t nnz_b,
                      const int32_t* b_ptr, const int32_t* b_idx, const float* b_val,
                      int accumulate_f64, int64_t n_products, int32_t* c_ptr, int32_t* c_idx,
                      float* c_val, int64_t* nnz_c_dev, gcg_stream_t stream);
/* gcg_spgemm with the path forced (tests, measurement; every path gives the same C, bitwise):
 * flags GCG_SPGEMM_EXPAND_SORT = the expand-sort-reduce path at any p, GCG_SPGEMM_DENSE_SLABS =
 * every row on the dense LDS slabs (no short-row radix-sort kernel), GCG_SPGEMM_COMPACT_TEMPORARY
 * = compact C through an nnz(C)-sized temporary instead of in place; chunk_products > 0 caps the
 * products per expand-sort-reduce row chunk (0 = 2^29). gcg_spgemm = flags 0, chunk 0. */
enum { GCG_SPGEMM_EXPAND_SORT = 1, GCG_SPGEMM_DENSE_SLABS = 2, GCG_SPGEMM_COMPACT_TEMPORARY = 4 };
gcg_status gcg_spgemm_ex(int64_t m, int64_t n, int64_t p, int64_t nnz_a, const int32_t* a_ptr,
                         const int32_t* a_idx, const void* a_val, int a_is_f64, int64_t nnz_b,
                         const int32_t* b_ptr, const int32_t* b_idx, const float* b_val,
                         int accumulate_f64, int64_t n_products, int32_t* c_ptr, int32_t* c_idx,
                         float* c_val, int64_t* nnz_c_dev, int32_t flags, int64_t chunk_products,
                         gcg_stream_t stream);

/*
 * Mention-graph projection on the device (DataLoader.get_graph's celebrity filter,
 * data.py:364-370, then efficient_collaboration_weighted_projected_graph2, data.py:226-250).
 * Input: the bipartite user/mention graph as incidences (a[e], b[e]) over n_nodes ids, ids <
 * n_targets are users (their self loops are implicit, as get_graph adds them), ids >= n_targets
 * mention-only names. A mention node survives iff 1 < degree <= celebrity_threshold. Output:
 * every pair of users that share a surviving neighbour (a user node's own self loop makes it a
 * neighbour of itself), deduplicated, u < v, sorted, into caller-owned device arrays out_u /
 * out_v of `capacity` entries; *n_edges = the edge count. Pass out_u = out_v = NULL to size:
 * *n_edges then receives the number of pairs before deduplication, an upper bound. Allocates
 * stream-ordered temporaries and synchronizes `stream`; not a hot-path call.
 */
gcg_status gcg_project_mention_graph(int64_t n_targets, int64_t n_nodes, int64_t n_inc,
                                     const int32_t* a, const int32_t* b, int celebrity_threshold,
                                     int32_t* out_u, int32_t* out_v, int64_t capacity,
                                     int64_t* n_edges, int32_t* status_dev, gcg_stream_t stream);

/*
 * Dense side of the output layer on the matrix cores. Row-major operands; A: M x K (lda),
 * B: K x N (ldb), C: M x N (ldc). A and B need 16-B aligned bases and ld % 4 == 0; B is read at
 * columns < round4(N), so ldb >= round4(N) (pad the weight, as graphconvgeo_amd.dense does).
 *
 * Arithmetic and tile are explicit per call (round 5) -- no environment variable changes what a
 * dense entry computes:
 *   math  GCG_MATH_F32     v_mfma_f32_16x16x4_f32: exact f32 products, f32 accumulation; the k
 *                          order inside a 16-deep step is permuted (step s takes k = k0 + 4q + s),
 *                          so results equal a BLAS sgemm within f32 rounding, not bit for bit.
 *         GCG_MATH_BF16X6  f32 on the bf16 matrix cores: every f32 operand split into three bf16
 *                          planes x = x0 + x1 + x2 (round to nearest, 8 significant bits each), the
 *                          six plane products of order <= 2^-16 accumulated in f32
 *                          (v_mfma_f32_16x16x32_bf16), each exact. The planes hold x exactly
 *                          (3 x 8 significant bits), |x1| <= 2^-8 |x|, |x2| <= 2^-17 |x|, so the
 *                          dropped a1b2 + a2b1 + a2b2 are <= (2^-24 + 2^-34) |a||b| per product --
 *                          one f32 rounding of the product (tests/test_bf16x6_numerics.py pins
 *                          these bounds; tests/test_dense_gpu.py the whole product's error against
 *                          float64, <= 1.25 x the f32 kernel's). A last k chunk with <= 16 live
 *                          k carries two plane products per MFMA (the fragments' zero high halves
 *                          hold another plane of the low halves' k): 3 MFMAs instead of 6 there,
 *                          every product still exact, the same in every bf16x6 form.
 *                          f32 semantics at the edges: a tile whose bf16x6 result is not finite
 *                          (an infinite operand, |x| above bf16's largest finite 3.39e38, NaN, or
 *                          overflow) is recomputed on the f32 MFMA in the f32 kernel's k order, so
 *                          +-Inf propagates and Inf * 0 gives NaN exactly as with GCG_MATH_F32.
 *   tile  0 = the default tile, a pure function of (M, N, K); 1..gcg_dense_tile_count(op, math)
 *         = a measured alternative (tests, measurement); the same products except where noted.
 */
enum { GCG_MATH_F32 = 0, GCG_MATH_BF16X6 = 1 };
enum { GCG_DENSE_GEMM = 0, GCG_DENSE_GEMM_NT = 1, GCG_DENSE_FUSED = 2, GCG_DENSE_GEMM_TN = 3 };
/* Alternative tiles of product op (GCG_DENSE_*) in arithmetic math: tile indices 1..n are valid;
 * -1 when that arithmetic is not available for the product. */
int32_t gcg_dense_tile_count(int32_t op, int32_t math);

/*
 * gcg_gemm: C = act(A . B + bias)        T.dot(h, W) (+ b) at mlpconv.py:88 / the propagate-first
 *   form of mlpconv.py:88-93, and Theano's g . W^T (W^T passed as B). GCG_MATH_F32 only; tile 0
 *   stages B through LDS (gemm_bl_kernel), tile 1 reads it straight into registers (gemm_kernel):
 *   the same k order, bitwise equal.
 * gcg_gemm_f32 = gcg_gemm(..., GCG_MATH_F32, 0, ...).
 */
gcg_status gcg_gemm(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B,
                    int64_t ldb, const float* bias /*nullable*/, int act, float* C, int64_t ldc,
                    int32_t math, int32_t tile, gcg_stream_t stream);
gcg_status gcg_gemm_f32(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                        const float* B, int64_t ldb, const float* bias /*nullable*/, int act,
                        float* C, int64_t ldc, gcg_stream_t stream);

/*
 * gcg_gemm_nt: C = act(A . Bt^T + bias) with the second operand stored transposed (Bt: N x K
 * row-major, ldbt >= round4(K), ldbt % 4 == 0, 16-B aligned base; A likewise with lda). The
 * projection T.dot(h, W) (mlpconv.py:88) with Bt = W^T, and Theano's input gradient g . W^T with
 * Bt = W itself. In the k step that reaches past K the fragment elements at k >= K are zeroed in
 * registers, so operand padding may hold anything (NaN included).
 *   GCG_MATH_F32: both operands through the asynchronous LDS-DMA (global_load_lds) into a ring of
 *     k chunks (tile 0: 16-deep chunks, 4 stages); every tile the same k order.
 *   GCG_MATH_BF16X6: ws != NULL (gcg_gemm_nt_workspace(N, K, math) bytes, 16-B aligned): Bt's
 *     three planes split once per call into it by a small kernel on the same stream, A split in
 *     registers (tile 0: A in registers, 128 x 64 G columns with G padding N least, or -- where
 *     that pads less -- 128 x 192 tiles over N's whole 192-column blocks and the narrowest tile
 *     over the rest, as two launches on the stream); ws == NULL: both operands split in the loop
 *     (tile 0 only). Every bf16x6 form accumulates the same six plane products in the same order:
 *     bitwise equal to each other.
 * gcg_gemm_nt_f32 = gcg_gemm_nt(..., GCG_MATH_F32, 0, NULL, 0, ...);
 * gcg_gemm_nt_f32_bf16x6 = gcg_gemm_nt(..., GCG_MATH_BF16X6, 0, ws, ws_bytes, ...).
 */
gcg_status gcg_gemm_nt(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                       const float* Bt, int64_t ldbt, const float* bias /*nullable*/, int act,
                       float* C, int64_t ldc, int32_t math, int32_t tile, void* ws /*nullable*/,
                       int64_t ws_bytes, gcg_stream_t stream);
int64_t gcg_gemm_nt_workspace(int64_t N, int64_t K, int32_t math);
gcg_status gcg_gemm_nt_f32(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                           const float* Bt, int64_t ldbt, const float* bias /*nullable*/,
                           int act, float* C, int64_t ldc, gcg_stream_t stream);
gcg_status gcg_gemm_nt_f32_bf16x6(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                                  const float* Bt, int64_t ldbt, const float* bias /*nullable*/,
                                  int act, float* C, int64_t ldc, void* ws /*nullable*/,
                                  int64_t ws_bytes, gcg_stream_t stream);
/* = gcg_gemm_nt_workspace(N, K, GCG_MATH_BF16X6) */
int64_t gcg_gemm_nt_bf16x6_workspace(int64_t N, int64_t K);

/*
 * Fused output layer + loss (N <= 1024; one workgroup owns whole rows):
 *   logits = A . W + bias                                       mlpconv.py:88-93
 *   labels != NULL: out = (softmax(logits) - onehot(labels)) * scale * row_weight[i]  (the logits
 *     gradient of categorical_crossentropy(...).mean() with scale = 1/M, mlpconv.py:229-230),
 *     loss_rows[i] = -log softmax(logits)[i, labels[i]] * row_weight[i],
 *     correct_rows[i] (nullable) = row_weight[i] if the first-index argmax equals labels[i] else 0
 *     (argmax + T.eq accuracy, mlpconv.py:227,252);
 *   labels == NULL: out = softmax(logits) (predict_proba, mlpconv.py:329-335);
 *   out may be NULL when labels are given (evaluation: loss and accuracy only).
 * row_weight (device, nullable = all 1, then bitwise the unweighted result): with the distinct
 * targets as rows and their multiplicities as weights, one call computes the loss and gradient of
 * a target list drawn with replacement (tensormain.py:226) over its distinct rows only.
 * scale_dev (nullable, device): multiplies scale (the upstream gradient of the loss, read on the
 * device so the call can sit inside a captured HIP graph). The logits never reach HBM. out needs
 * ldo % 4 == 0 and a 16-B aligned base; its padding columns [N, round4(N)) are written with zeros
 * (whole dwordx4 row stores). W's padding columns [N, ldw) may hold anything (NaN included): they
 * never reach a logit. A label outside [0, N) gives that row a NaN loss, no hit, no onehot.
 *   GCG_MATH_F32 (gemm_kernel): 32 rows x 4 waves; tiles 1..5 split the weight's register set
 *     into 0 / 2 / 4 / 8 / 16 rotating parts (tile 0: 8 at N > 768, else 4) -- bitwise equal.
 *   GCG_MATH_BF16X6 (gemm_fused6_kernel): ws != NULL (gcg_project_softmax_xent_workspace(N, K,
 *     math) bytes, 16-B aligned): the weight's three bf16 planes split once per call into it;
 *     tile 0 = tile 3 = 64 rows x 8 waves at N > 768 (row sums over 8 column waves), else 32
 *     rows x 4 waves, the A chunk split once per workgroup into LDS planes; tile 1 = 32 rows x 4
 *     waves at any N (bitwise the ws == NULL form); tile 2 = the 64-row form (N > 768 only);
 *     tiles 1 / 2 split A in every wave's registers, bitwise equal to tile 3 of their shape.
 *     ws == NULL: the weight split in every workgroup's registers,
 *     32 rows x 4 waves (tile 0 only). The 64-row form is within f32 rounding of the 32-row one
 *     (another association of the row sums), with the same hits.
 * Legacy entries: gcg_project_softmax_xent_f32 and _weighted_f32 = GCG_MATH_F32, tile 0;
 * _weighted_ws_f32 = GCG_MATH_BF16X6, tile 0 (with ws, or the in-register split when NULL).
 */
gcg_status gcg_project_softmax_xent(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                                    const float* W, int64_t ldw, const float* bias /*nullable*/,
                                    const int32_t* labels /*nullable*/, float scale,
                                    const float* scale_dev /*nullable*/, float* out /*nullable*/,
                                    int64_t ldo, float* loss_rows,
                                    float* correct_rows /*nullable*/,
                                    const float* row_weight /*nullable*/, int32_t math,
                                    int32_t tile, void* ws /*nullable*/, int64_t ws_bytes,
                                    gcg_stream_t stream);
int64_t gcg_project_softmax_xent_workspace(int64_t N, int64_t K, int32_t math);
gcg_status gcg_project_softmax_xent_f32(int64_t M, int64_t N, int64_t K, const float* A,
                                        int64_t lda, const float* W, int64_t ldw,
                                        const float* bias /*nullable*/,
                                        const int32_t* labels /*nullable*/, float scale,
                                        const float* scale_dev /*nullable*/,
                                        float* out /*nullable*/, int64_t ldo, float* loss_rows,
                                        float* correct_rows /*nullable*/, gcg_stream_t stream);
/* = gcg_project_softmax_xent_workspace(N, K, GCG_MATH_BF16X6) */
int64_t gcg_project_softmax_xent_bf16x6_workspace(int64_t N, int64_t K);
gcg_status gcg_project_softmax_xent_weighted_ws_f32(
    int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* W, int64_t ldw,
    const float* bias /*nullable*/, const int32_t* labels /*nullable*/, float scale,
    const float* scale_dev /*nullable*/, float* out /*nullable*/, int64_t ldo, float* loss_rows,
    float* correct_rows /*nullable*/, const float* row_weight /*nullable*/, void* ws /*nullable*/,
    int64_t ws_bytes, gcg_stream_t stream);

/*
 * The same row epilogue for logits that already exist (the reference order, where the
 * logits are the H SpMM's output rows, mlpconv.py:90-94): one wave per row, N <= 4096,
 * out may alias logits; out == NULL computes loss_rows / correct_rows only (the forward
 * half; the gradient pass then runs with out set and scale_dev = the upstream gradient).
 */
gcg_status gcg_softmax_xent_f32(int64_t M, int64_t N, const float* logits, int64_t ldl,
                                const int32_t* labels /*nullable*/, float scale,
                                const float* scale_dev /*nullable*/, float* out /*nullable*/,
                                int64_t ldo, float* loss_rows, float* correct_rows /*nullable*/,
                                gcg_stream_t stream);

/*
 * Weighted forms of the two above: row i's loss, hit and gradient row are multiplied by
 * row_weight[i] (device, nullable = all 1 -- then bitwise the unweighted calls). With the
 * distinct targets as rows and their multiplicities as weights, one call computes the loss
 * and gradient of a target list drawn with replacement (tensormain.py:226) over its distinct
 * rows only: sum_i w_i loss_i = the sum over the full list, and the gradient of a distinct row
 * is the sum of its duplicates' gradients (Theano's inc_subtensor adds them, mlpconv.py:94).
 */
gcg_status gcg_project_softmax_xent_weighted_f32(int64_t M, int64_t N, int64_t K,
                                                 const float* A, int64_t lda, const float* W,
                                                 int64_t ldw, const float* bias /*nullable*/,
                                                 const int32_t* labels /*nullable*/, float scale,
                                                 const float* scale_dev /*nullable*/,
                                                 float* out /*nullable*/, int64_t ldo,
                                                 float* loss_rows,
                                                 float* correct_rows /*nullable*/,
                                                 const float* row_weight /*nullable*/,
                                                 gcg_stream_t stream);
gcg_status gcg_softmax_xent_weighted_f32(int64_t M, int64_t N, const float* logits, int64_t ldl,
                                         const int32_t* labels /*nullable*/, float scale,
                                         const float* scale_dev /*nullable*/,
                                         float* out /*nullable*/, int64_t ldo, float* loss_rows,
                                         float* correct_rows /*nullable*/,
                                         const float* row_weight /*nullable*/,
                                         gcg_stream_t stream);

/*
 * Weight gradient C = scale * A^T . B (Theano's grad of T.dot(h, W) w.r.t. W: h^T . gz,
 * mlpconv.py:88; P^T . G in the propagate-first order), A: R x M, B: R x N, C: M x N, the
 * reduction over R (~10^6 rows) split across waves; the per-split partials (caller-owned
 * workspace, size from gcg_gemm_tn_workspace_bytes for the same math and tile) are summed in
 * split order, so the result is deterministic (equal to a BLAS sgemm within f32 rounding). A and
 * B: 16-B aligned, lda >= round4(M), ldb >= round4(N), ld % 4 == 0. scale_dev: nullable device
 * scalar.
 *   GCG_MATH_F32 (f32 MFMA): tile 0 = per-wave 64 x 64 NG tiles (NG padding N least) or, for
 *     M <= 256 in 64-row bands with N <= 512, waves stacked along M; tiles 1..7 = other wave
 *     layouts and split counts (another summation order: within f32 rounding).
 *   GCG_MATH_BF16X6 (tile 0 only): per-wave 64 x 64 tiles on the bf16 matrix cores, each
 *     32-row chunk's six plane products summed apart and added to the split's running sum once
 *     (error against float64 at or below the f32 form's); non-finite tiles recomputed in f32.
 * gcg_gemm_tn_f32[_workspace_bytes] = the GCG_MATH_F32, tile 0 forms.
 */
gcg_status gcg_gemm_tn_workspace_bytes(int64_t R, int64_t M, int64_t N, int32_t math,
                                       int32_t tile, size_t* bytes);
gcg_status gcg_gemm_tn(int64_t R, int64_t M, int64_t N, const float* A, int64_t lda,
                       const float* B, int64_t ldb, const float* scale_dev /*nullable*/, float* C,
                       int64_t ldc, int32_t math, int32_t tile, void* workspace,
                       size_t workspace_bytes, gcg_stream_t stream);
gcg_status gcg_gemm_tn_f32_workspace_bytes(int64_t R, int64_t M, int64_t N, size_t* bytes);
gcg_status gcg_gemm_tn_f32(int64_t R, int64_t M, int64_t N, const float* A, int64_t lda,
                           const float* B, int64_t ldb, const float* scale_dev /*nullable*/,
                           float* C, int64_t ldc, void* workspace, size_t workspace_bytes,
                           gcg_stream_t stream);

/*
 * Geolocation labels and metrics (csrc/geo.hip). Coordinates are row-major N x 2 float64
 * [latitude, longitude] in degrees, 8-B aligned; all arithmetic is float64. Unlike the hot-path
 * entries above, gcg_kdtree_fit_f64 and gcg_class_medians_f64 allocate their scratch with
 * hipMallocAsync on `stream`, and gcg_kdtree_fit_f64 synchronizes the stream once per tree level.
 *
 * gcg_kdtree_fit_f64: the region labels of kdtree.KDTreeClustering(bucket_size).fit(locs)
 * (kdtree.py:84-151), exactly: a node of more than bucket_size points splits on the axis of the
 * larger max - min (a tie gives latitude) at np.median of that axis (split == max -> min; zero
 * width -> leaf), `value > split` goes right, and leaves are numbered in pre-order, left first.
 * Built level by level over two id lists kept sorted by latitude / longitude inside every node.
 *   labels[N]      the leaf number of every point
 *   perm_lat[N], perm_lon[N]  the point ids grouped by leaf, sorted by latitude / longitude
 *                  inside each leaf
 *   leaf_ptr[N+1]  capacity N + 1; leaf c is [leaf_ptr[c], leaf_ptr[c+1]) of both lists
 *                  (entries 0 .. n_clusters are written)
 *   n_clusters_host, depth_host (levels on which a node split; nullable), readbacks_host (the
 *                  stream synchronizations made: depth + 2; nullable): HOST outputs
 *   status_dev     device int32, set to 1 for a non-finite coordinate (the call then returns
 *                  GCG_ERR_INVALID_ARG after the first level's readback; outputs undefined)
 * N = 0 gives 0 clusters; bucket_size < 1 is GCG_ERR_INVALID_ARG. N <= 2^30 - 2.
 */
gcg_status gcg_kdtree_fit_f64(int64_t N, const double* locs, int64_t bucket_size,
                              int32_t* labels, int32_t* perm_lat, int32_t* perm_lon,
                              int32_t* leaf_ptr, int64_t* n_clusters_host,
                              int64_t* depth_host /*nullable*/,
                              int64_t* readbacks_host /*nullable*/, int32_t* status_dev,
                              gcg_stream_t stream);

/*
 * medians[c] = (np.median of the latitudes, np.median of the longitudes) of segment
 * [ptr[c], ptr[c+1]) of perm_lat / perm_lon (point ids sorted by that coordinate inside every
 * segment, as gcg_kdtree_fit_f64 leaves them): a selection, or (a + b) / 2 of the two middle
 * values, so bitwise numpy's. An empty or out-of-range segment gives NaN. medians: C x 2.
 */
gcg_status gcg_segment_medians_f64(int64_t C, int64_t N, const double* locs, const int32_t* ptr,
                                   const int32_t* perm_lat, const int32_t* perm_lon,
                                   double* medians, gcg_stream_t stream);

/*
 * Per-class medians of DataLoader.assignClasses (data.py:408-413) for any labels[N] in [0, C):
 * a radix sort by coordinate, a stable one by class, then gcg_segment_medians_f64's lookup.
 * A class without points gives NaN (np.median of nothing). *status_dev = 1 for a label outside
 * [0, C) or a non-finite coordinate (medians are then undefined).
 */
gcg_status gcg_class_medians_f64(int64_t N, const double* locs, const int32_t* labels, int64_t C,
                                 double* medians, int32_t* status_dev, gcg_stream_t stream);

/*
 * out[i] = great-circle distance in km between a[i] and b[i], as the `haversine` package the
 * reference imports: 2 R asin(sqrt(sin^2(dlat/2) + cos(lat1) cos(lat2) sin^2(dlon/2))), with the
 * square root's argument clamped to 1. The package's radius differs between its versions
 * (6371 / 6371.0088), so it is an argument.
 */
gcg_status gcg_haversine_km_f64(int64_t M, const double* a, const double* b,
                                double earth_radius_km, double* out, gcg_stream_t stream);

/*
 * The brute-force 1-nearest-neighbour of data.py:416-419: index[i] = argmin_c
 * haversine(locs[i], medians[c]), the first index on ties; distance (nullable) = that minimum.
 * One kernel, one query per thread, the medians staged through LDS in tiles of 2048. A NaN
 * median is never the nearest. C >= 1 unless M = 0.
 */
gcg_status gcg_nearest_class_f64(int64_t M, const double* locs, int64_t C, const double* medians,
                                 double earth_radius_km, int32_t* index,
                                 double* distance /*nullable*/, gcg_stream_t stream);

/*
 * tensormain.geo_eval's per-user work (tensormain.py:38-50): distance[i] = haversine(locs[i],
 * medians[pred[i]]) and *count_dev = the number of rows with distance < threshold_km (strict).
 * pred: int32 (pred_is_int64 = 0) or int64 (1) device array. *status_dev = 1 when a prediction
 * lies outside [0, C) (its distance is NaN and it is not counted). Both scalars are reset first.
 */
gcg_status gcg_geo_eval_f64(int64_t M, const void* pred, int pred_is_int64, const double* locs,
                            int64_t C, const double* medians, double earth_radius_km,
                            double threshold_km, double* distance, int64_t* count_dev,
                            int32_t* status_dev, gcg_stream_t stream);

/*
 * The grid representation of loc2lang's no-MDN baseline (csrc/grid.hip; loc2lang.py:298-322):
 * row i of an n x P CSR, P = n_lat * n_lon, holds an entry for every grid point nearer than
 * radius_km to coords[i] (strict <), column i_lat * n_lon + i_lon ascending, with the value
 * float32((1 / d) / sum of the row's 1 / d), d the distance of gcg_haversine_km_f64 -- float64
 * throughout, one rounding at the store. When Z >= 1 columns lie at distance zero they hold 1 / Z
 * and the row's other in-range columns an explicit +0.0 (the limit; the reference divides by
 * zero). A row with no grid point in range is empty. coords: n x 2 [lat, lon] degrees; lats, lons:
 * the grid's coordinate tables in degrees, ascending, as the host computed them (they are never
 * re-derived from a start and a step); 2 * n_lat + n_lon <= 6144 (the tables live in LDS).
 *
 * gcg_grid_count_f64 writes indptr (int32[n + 1]; clamped at INT32_MAX), norm (float64[n]: the
 * row's sum of 1 / d, or -Z) and info_dev (int64[2]: the total number of entries, summed in
 * int64; 1 when a coordinate is not finite or |lat| > 90 -- such a row counts nothing and the
 * result is to be dropped). The row sum adds the k-th entry of the row into slot k % 64 and folds
 * the 64 slots by a fixed butterfly, so it depends on nothing but the row. gcg_grid_fill_f64,
 * given the same arguments and count's indptr and norm, writes indices and values (nnz slots
 * each; nnz = info_dev[0], which has to be below 2^31). One wave per coordinate.
 *
 * The window. A wave looks only at columns that can be in range, a superset by these bounds:
 * d >= R |dlat|, so |dlat| < radius / R; and a >= cos(lat1) cos(lat2) sin^2(dlon / 2) with
 * a < sin^2(radius / 2R), so inside a latitude row |sin(dlon / 2)| < sin(radius / 2R) /
 * sqrt(cos(lat1) cos(lat2)) for dlon reduced to [-pi, pi] -- every longitude when that bound
 * reaches 1 or the cosine product is 0 (near a pole). Both windows are widened by one cell, and
 * the longitude window is taken around lon + 2 pi k for every k that reaches the table, lowest
 * columns first. exhaustive = 1 makes the window the whole grid on the same code path; the
 * results are bitwise the same.
 *
 * Asynchronous on `stream`, no allocation; n = 0 succeeds without a launch. The workspace
 * (8-B aligned) is sized by gcg_grid_count_f64_workspace_bytes, which asks hipcub and so needs a
 * HIP device for n > 0.
 */
gcg_status gcg_grid_count_f64_workspace_bytes(int64_t n, size_t* bytes);
gcg_status gcg_grid_count_f64(int64_t n, const double* coords, int64_t n_lat, const double* lats,
                              int64_t n_lon, const double* lons, double radius_km,
                              double earth_radius_km, int exhaustive, int32_t* indptr,
                              double* norm, int64_t* info_dev, void* workspace,
                              size_t workspace_bytes, gcg_stream_t stream);
gcg_status gcg_grid_fill_f64(int64_t n, const double* coords, int64_t n_lat, const double* lats,
                             int64_t n_lon, const double* lons, double radius_km,
                             double earth_radius_km, int exhaustive, const int32_t* indptr,
                             const double* norm, int64_t nnz, int32_t* indices, float* values,
                             gcg_stream_t stream);

/*
 * k-means initialisation of the Gaussian components (csrc/kmeans.hip): get_cluster_centers of
 * lang2loc.py:473-478, lang2loc_mdnshared.py:127-185 and loc2lang.py:326-371 as full Lloyd
 * k-means (the reference runs MiniBatchKMeans on the host). Coordinates as above: N x 2 float64,
 * N <= 2^30 - 2; labels, indices and counts are int32; the metric is Euclidean on raw degrees,
 * as the reference's. Every squared distance is
 *     d = (x0 - c0) * (x0 - c0) + (x1 - c1) * (x1 - c1)
 * with each operation rounded once, in that order (no fused multiply-add), and strict < keeps
 * the lowest index on a tie. No result depends on the launch grid or on timing; there are no
 * floating-point atomics. Scratch is the caller's: every *_workspace_bytes function gives the
 * size for (N, C), the workspace is 256-B aligned, and no entry synchronizes the stream.
 * *status_dev (device int32, reset by every call) reports data errors.
 *
 * gcg_kmeans_assign_f64: labels[i] = the nearest centre of point i; dist2[i] (nullable) = that
 * squared distance. One kernel: 4 points per thread (point g * 1024 + t + 256 p for thread t of
 * workgroup g), the centres staged through LDS in tiles of gcg_kmeans_centre_tile() = 1024.
 *   changed_dev (nullable)  1 when prev_labels is given and some label differs from it, else 0
 *   inertia_dev (nullable)  the sum of the minima: a thread adds its points in ascending p, a
 *                 workgroup its threads in the tree s[t] += s[t + h], h = 128 .. 1, and one
 *                 workgroup adds the per-workgroup partials the same way (thread t takes
 *                 partials t, t + 256, ... in ascending order). Needs the workspace.
 *   status_dev    1 for a non-finite coordinate in locs
 * A NaN centre is never the nearest. N = 0 is a no-op (inertia 0); C >= 1 unless N = 0.
 */
int32_t gcg_kmeans_centre_tile(void);
gcg_status gcg_kmeans_assign_f64_workspace_bytes(int64_t N, size_t* bytes);
gcg_status gcg_kmeans_assign_f64(int64_t N, const double* locs, int64_t C, const double* centers,
                                 const int32_t* prev_labels /*nullable*/, int32_t* labels,
                                 double* dist2 /*nullable*/, double* inertia_dev /*nullable*/,
                                 int32_t* changed_dev /*nullable*/, int32_t* status_dev,
                                 void* workspace, size_t workspace_bytes, gcg_stream_t stream);

/*
 * centers[c] = the float64 sum of the members of cluster c divided by counts[c]; an empty
 * cluster keeps prev_centers[c] and gets count 0 (centers may be prev_centers). Reduction order:
 * a stable radix sort of (label, index) groups the members by cluster in ascending index; one
 * workgroup of 256 threads per cluster, thread t adding members t, t + 256, ... of the segment
 * in that order, then the tree s[t] += s[t + h], h = 128 .. 1. The grid only decides which
 * workgroup takes which cluster, so the result is bitwise the same from call to call.
 * *status_dev = 1 for a label outside [0, C) (it counts as cluster 0).
 */
gcg_status gcg_kmeans_update_f64_workspace_bytes(int64_t N, int64_t C, size_t* bytes);
gcg_status gcg_kmeans_update_f64(int64_t N, const double* locs, const int32_t* labels, int64_t C,
                                 const double* prev_centers, double* centers, int32_t* counts,
                                 int32_t* status_dev, void* workspace, size_t workspace_bytes,
                                 gcg_stream_t stream);

/*
 * k-means++ seeding, one trial per centre, as a pure function of the uniform draws u_dev[C]
 * (device float64 in [0, 1)): indices[0] = floor(u[0] * N); for k >= 1, D2[i] = the minimum over
 * the chosen centres of the squared distance above, S = the inclusive prefix sum of D2 in index
 * order, and indices[k] = the first i with S_i > u[k] * S_{N-1}, clamped to the last i with
 * D2[i] > 0 -- a point at distance 0 from a chosen centre is never picked. S is summed in fixed
 * levels, each in ascending order: the 8 consecutive points of a thread, the 256 threads of a
 * workgroup (2048 points), the workgroups of a chunk of ceil(nb / 256), the 256 chunks. The C
 * rounds are two launches each, sequential on the stream; the chosen index stays on the device.
 *   status_dev  1: S_{N-1} = 0 before all C were chosen (fewer distinct points than C);
 *               2: a non-finite coordinate; 3: a draw outside [0, 1). indices are then undefined
 *               (but inside [0, N)).
 * 1 <= C <= N.
 */
gcg_status gcg_kmeans_pp_f64_workspace_bytes(int64_t N, size_t* bytes);
gcg_status gcg_kmeans_pp_f64(int64_t N, const double* locs, int64_t C, const double* u_dev,
                             int32_t* indices, int32_t* status_dev, void* workspace,
                             size_t workspace_bytes, gcg_stream_t stream);

/*
 * The per-cluster statistics of get_cluster_centers for any labels[N] in [0, C): counts
 * (nullable), means (C x 2), the ddof-1 standard deviations sigmas (C x 2) and the correlation
 * corxys (C). Members are grouped and summed as in gcg_kmeans_update_f64, in two passes: the
 * deviations from the segment's first member f give the mean f + sum / n, the deviations from
 * that mean the (co)variances -- identical points have variance exactly 0. A single member, a
 * zero variance, a NaN or an empty cluster give (1, 1, 0); an empty cluster leaves means[c] as
 * passed in. raw = 1 stores s + log1p(-exp(-s)) and c / (1 - |c|), the inverses of the models'
 * softplus and softsign. *status_dev = 1 for a label outside [0, C).
 */
gcg_status gcg_cluster_stats_f64_workspace_bytes(int64_t N, int64_t C, size_t* bytes);
gcg_status gcg_cluster_stats_f64(int64_t N, const double* locs, const int32_t* labels, int64_t C,
                                 int raw, double* means /*in, out*/, double* sigmas,
                                 double* corxys, int32_t* counts /*nullable*/,
                                 int32_t* status_dev, void* workspace, size_t workspace_bytes,
                                 gcg_stream_t stream);

/*
 * The dialect-embedding evaluation (csrc/neighbours.hip): main.py's eval_embeddings (364-384),
 * nearest_neighbours (108-162) and what recall_at_k (230-281) needs of it, on resident float32
 * embeddings E (V x D, row stride lde >= D, V <= 2^31 - 2) and queries (Q x D, row stride ldq).
 *
 * The distance and the order, everywhere below: d2(q, e) = one float32 accumulator, from +0,
 * taking acc = fma(d, d, acc) with d = q_j - e_j (rounded once) for j = 0, 1, ..., D - 1 in
 * that order. It is the difference form (no cancellation: relative error at most
 * (D + 2) 2^-24 / (1 - (D + 2) 2^-24), exact on small integers) and the same (query, row) pair
 * has the same bits in every entry. Words are ordered by (d2 as float32, row index) ascending.
 *
 * Conventions as above: caller-owned buffers and workspaces (*_workspace_bytes; 256-B aligned),
 * no entry synchronizes the stream, *status_dev (device int32, reset by every call) reports
 * data errors, and every result is bitwise the same from call to call: sums run in a fixed
 * order and the only atomics add integers.
 *
 * gcg_neighbours_tile(which): the sizes a caller's tests want to sit on.
 */
enum {
  GCG_NEIGHBOURS_ROW_TILE = 0,         /* rows of E per workgroup of the distance pass (256) */
  GCG_NEIGHBOURS_QUERY_TILE = 1,       /* queries per workgroup, Q > the small tile (32) */
  GCG_NEIGHBOURS_QUERY_TILE_SMALL = 2, /* ... for Q <= 8 (8) */
  GCG_NEIGHBOURS_SLOT_CAP = 3,         /* pairs of a query tile counted in LDS; more go to HBM */
  GCG_NEIGHBOURS_COL_CHUNK = 4,        /* columns staged through LDS per step (32) */
  GCG_NEIGHBOURS_MAX_K = 5,            /* the largest k of gcg_kneighbors_f32 (1024) */
  GCG_NEIGHBOURS_MINMAX_ROWS = 6,      /* rows per workgroup of the column min / max (1024) */
  GCG_NEIGHBOURS_MERGE_SLICE = 7       /* kneighbors candidates per first-level merge (8192) */
};
int32_t gcg_neighbours_tile(int32_t which); /* 0 for an unknown `which` */

/*
 * eval_embeddings' preprocessing (main.py:373-377): sklearn's MinMaxScaler(0, 1) and
 * normalize(norm='l1'). Two passes over E. The first takes every column's minimum and maximum
 * (row blocks of 1024 in ascending order, no atomics). The second is fused, one wave per row:
 * y_j = x_j * scale_j + (0 - min_j * scale_j), scale_j = 1 / (max_j - min_j) or 1 where
 * max_j == min_j, in float64; the row's sum of |y_j| in a fixed order; out_j = y_j / sum rounded
 * to float32. A row whose sum is 0 keeps y. `out` (V x D, row stride ldo) must not overlap E;
 * columns past D of either are neither read nor written. *status_dev = 1 for a non-finite
 * element of E (the output is then meaningless).
 */
gcg_status gcg_minmax_l1_rows_f32_workspace_bytes(int64_t V, int64_t D, size_t* bytes);
gcg_status gcg_minmax_l1_rows_f32(int64_t V, int64_t D, const float* E, int64_t lde, float* out,
                                  int64_t ldo, int32_t* status_dev, void* workspace,
                                  size_t workspace_bytes, gcg_stream_t stream);

/*
 * rank[p] = #{v in [0, V) : (d2(q_p, v), v) < (d2(q_p, w_p), w_p)} for the P pairs
 * (q_p, w_p = pair_word[p]) grouped by query: query q owns pairs [pair_ptr[q], pair_ptr[q + 1]).
 * That is the 0-based position of word w_p in the full ordering of the V words for query q_p,
 * which is all recall@k needs. The thresholds d2(q_p, w_p) are computed first and sorted inside
 * each query; then E is read once per tile of 32 queries (8 when Q <= 8): a workgroup owns 256
 * rows, computes each d2(q, v) once, finds by binary search the first threshold of q above it
 * and adds 1 to that slot (in LDS when the tile has at most GCG_NEIGHBOURS_SLOT_CAP pairs); a
 * prefix sum over each query's slots gives the ranks. No Q x V array is written. A query tile
 * without pairs costs nothing.
 *   status_dev  1 a non-finite element or distance, 2 a word outside [0, V), 3 pair_ptr is not
 *               0 = ptr[0] <= ... <= ptr[Q] = P (no rank is then computed); ranks are
 *               meaningless unless it is 0
 */
gcg_status gcg_neighbour_ranks_f32_workspace_bytes(int64_t Q, int64_t P, size_t* bytes);
gcg_status gcg_neighbour_ranks_f32(int64_t V, int64_t D, const float* E, int64_t lde, int64_t Q,
                                   const float* queries, int64_t ldq, int64_t P,
                                   const int32_t* pair_ptr, const int32_t* pair_word,
                                   int32_t* rank, int32_t* status_dev, void* workspace,
                                   size_t workspace_bytes, gcg_stream_t stream);

/*
 * The k smallest (d2, row) of every query in order: dist2[Q x k] and index[Q x k], so that
 * index[q * k + r] == w exactly when rank(q, w) == r. 1 <= k <= min(V, 1024), else
 * GCG_ERR_INVALID_ARG (the full ordering is what gcg_neighbour_ranks_f32 is for). The distance
 * pass is the rank entry's (the same query tiles); every tile of 256 rows then sorts its keys in
 * LDS and keeps its first min(k, 256) per query, and one workgroup per query merges them (in
 * two levels above 8192 candidates: up to 64 slices, then the slices' k each). The workspace
 * holds the candidates, Q * ceil(V / 256) * min(k, 256) * 8 bytes, and the slices' results.
 * *status_dev = 1 for a non-finite element.
 */
gcg_status gcg_kneighbors_f32_workspace_bytes(int64_t V, int64_t Q, int64_t k, size_t* bytes);
gcg_status gcg_kneighbors_f32(int64_t V, int64_t D, const float* E, int64_t lde, int64_t Q,
                              const float* queries, int64_t ldq, int64_t k, float* dist2,
                              int32_t* index, int32_t* status_dev, void* workspace,
                              size_t workspace_bytes, gcg_stream_t stream);

/*
 * TF-IDF features over token ids (DataLoader.tfidf, data.py:378-397: sklearn's TfidfVectorizer at
 * ngram_range (1, 1), smooth_idf). The host tokenises and owns the term dictionary; these entries
 * do what is arithmetic over ids. None of them synchronizes or allocates.
 *
 * gcg_tfidf_count: one chunk of n_docs whole documents into a canonical count CSR (columns
 * sorted and unique per row, int32 counts). doc_ptr[0 .. n_docs] (int64) are token offsets, and
 * `tokens` points at token doc_ptr[0]: the chunk's n_tokens = doc_ptr[n_docs] - doc_ptr[0] ids.
 * With `rank` (int32[n_terms]) an id t in [0, n_terms) is replaced by rank[t] first (the
 * lexicographic position of a first-seen id). An id outside [0, n_terms), before or after the
 * map, is dropped. The keys (document << bits(n_terms)) | term are 64-bit and sorted over their
 * significant bits only, so n_docs * n_terms may exceed 2^32.
 *   Chunks append: *nnz_dev holds the entries written so far (set it to 0 before the first
 * chunk); the chunk's entries go to indices / counts [*nnz_dev ...), indptr[0 .. n_docs]
 * receives *nnz_dev + the rows' offsets (pass the global indptr + the chunk's first document;
 * the next chunk rewrites the shared boundary with the same value), and *nnz_dev moves on. A
 * chunk has at most n_tokens entries, so capacity = the corpus' token count always suffices;
 * where *nnz_dev + the chunk's entries would exceed `capacity` nothing is written and
 * *status_dev = GCG_ERR_WORKSPACE (status_dev is only ever set, never cleared). To size exactly
 * instead, pass indptr = indices = counts = NULL: the call then only moves *nnz_dev on by the
 * chunk's entry count and leaves df alone.
 *   df (int64[n_terms], or NULL) accumulates the number of rows that hold each term, by
 * df_mode 0 = one integer atomic per entry, 1 = from a term-ordered copy of the chunk's columns
 * (a second, 32-bit sort; one plain add per distinct term). Both are exact.
 */
gcg_status gcg_tfidf_count_workspace_bytes(int64_t n_docs, int64_t n_tokens, int64_t n_terms,
                                           size_t* bytes);
gcg_status gcg_tfidf_count(int64_t n_docs, int64_t n_terms, int64_t n_tokens,
                           const int64_t* doc_ptr, const int32_t* tokens, const int32_t* rank,
                           int32_t* indptr, int32_t* indices, int32_t* counts, int64_t capacity,
                           int64_t* nnz_dev, int64_t* df, int32_t df_mode, int32_t* status_dev,
                           void* workspace, size_t workspace_bytes, gcg_stream_t stream);
/*
 * Vocabulary pruning (CountVectorizer._limit_features with the bounds already integers): term t
 * is kept iff lo <= df[t] <= hi. new_id[t] = the number of kept terms below t, or -1;
 * kept_df[new_id[t]] = df[t] (capacity n_terms); *n_kept_dev = the number kept.
 * gcg_tfidf_idf_f64: idf[t] = ln((1 + n_docs) / (1 + df[t])) + 1 in float64.
 */
gcg_status gcg_tfidf_select_workspace_bytes(int64_t n_terms, size_t* bytes);
gcg_status gcg_tfidf_select(int64_t n_terms, const int64_t* df, int64_t lo, int64_t hi,
                            int32_t* new_id, int64_t* kept_df, int64_t* n_kept_dev,
                            void* workspace, size_t workspace_bytes, gcg_stream_t stream);
gcg_status gcg_tfidf_idf_f64(int64_t n_terms, const int64_t* df, int64_t n_docs, double* idf,
                             gcg_stream_t stream);
/*
 * Column compaction: the entries of the count CSR whose column has new_id >= 0, relabelled, in
 * their order; a row may become empty. Two calls: with out_indices = out_counts = NULL the new
 * out_indptr[0 .. n_rows] is written (out_indptr[n_rows] = the entry count, the capacity the
 * second call needs; this call uses the workspace); with them the entries are written from
 * that out_indptr (no workspace). An entry past `capacity` is not written.
 */
gcg_status gcg_tfidf_compact_workspace_bytes(int64_t n_rows, size_t* bytes);
gcg_status gcg_tfidf_compact(int64_t n_rows, int64_t n_terms, int64_t nnz, const int32_t* indptr,
                             const int32_t* indices, const int32_t* counts, const int32_t* new_id,
                             int32_t* out_indptr, int32_t* out_indices, int32_t* out_counts,
                             int64_t capacity, void* workspace, size_t workspace_bytes,
                             gcg_stream_t stream);
/*
 * Counts -> float32 values of the same CSR (TfidfTransformer.transform): tf = 1 if binary else
 * the count; tf = ln(tf) + 1 if sublinear_tf; tf *= idf[column] if idf != NULL; then the row is
 * divided by its l2 or l1 norm (norm = GCG_TFIDF_NORM_*); an empty or zero-norm row is left as
 * it is. All in float64, the row sum in a fixed order without atomics (one wave per row: lane l
 * folds entries l, l + 64, ... in order, then a butterfly over the lanes), one rounding to
 * float32 at the store.
 */
enum { GCG_TFIDF_NORM_NONE = 0, GCG_TFIDF_NORM_L1 = 1, GCG_TFIDF_NORM_L2 = 2 };
gcg_status gcg_tfidf_weight_f32(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* indptr,
                                const int32_t* indices, const int32_t* counts, const double* idf,
                                int32_t binary, int32_t sublinear_tf, int32_t norm, float* vals,
                                gcg_stream_t stream);

/*
 * Tokenising a corpus on the device (csrc/tokenize.hip): sklearn's analyzer at ngram_range
 * (1, 1) for the token patterns (?u)\b\w\w+\b (lookbehind = 0) and (?u)(?<![#@])\b\w\w+\b
 * (lookbehind = 1) over UTF-8 bytes. A token is a maximal run of word characters of at least two
 * code points; with the lookbehind a run preceded by '#' or '@' is dropped whole. `text` is the
 * documents (lowercased by the caller where wanted) joined by one NUL byte each: n_bytes bytes,
 * 16-byte aligned and readable up to n_bytes rounded up to 16 (what lies past n_bytes is not
 * looked at), at most 2^33. `word_table` is the word class as a bitmap over the code points
 * U+0000 .. U+10FFFF (bit cp & 31 of word cp >> 5; 34816 words), taken from the regex engine
 * whose findall is to be matched. Integers only: the outputs are the same on every run. None
 * of the entries synchronizes or allocates; sizes the host needs are read from the *_dev outputs.
 *
 * gcg_tokenize_mark: flags[0 .. round16(n_bytes)) (16-byte aligned) per byte, tile_base
 * [0 .. tiles] with tiles = ceil(n_bytes / GCG_TOKENIZE_TILE_BYTES) (the tiles' running counts),
 * totals_dev[0] = the number of tokens, totals_dev[1] = the number of NUL bytes (n_docs - 1
 * unless a document contains one).
 *
 * gcg_tokenize_terms: the term dictionary of the n_tokens tokens marked. Each token's bytes
 * are hashed to 64 bits, cut to the low hash_bits (1 .. 64; less than 64 is for tests), the
 * hashes sorted stably with the token index, and every token is compared byte by byte with the
 * first token of its run, so the result is exact whatever the hash does: tokens with different
 * bytes under one hash set result_dev[1] = 1 and the caller discards the outputs. Otherwise
 * tok_term[t] (int32[n_tokens]) = token t's term, the terms numbered in order of first
 * appearance; term_start / term_len (capacity n_tokens) = byte offset and byte length of each
 * term's first occurrence; result_dev[0] = the number of terms. doc_ptr[0 .. n_docs] = the
 * documents' token offsets: with doc_off = NULL the documents are what the NULs separate (the
 * caller has checked totals_dev[1] = n_docs - 1), else document d starts at byte doc_off[d]
 * (int64[n_docs + 1], doc_off[n_docs] = n_bytes + 1), which is exact for documents that contain
 * NUL. n_docs >= 1.
 *
 * gcg_tokenize_remap: the caller's action per term (int32[n_terms]): GCG_TOKENIZE_DROP removes
 * the term's tokens (a stop word), any other value replaces the token (-1, or a column).
 * tokens (capacity n_tokens) receives the kept tokens in order, doc_ptr[0 .. n_docs] the
 * documents' offsets among them (doc_ptr[n_docs] = the number kept).
 */
#define GCG_TOKENIZE_TILE_BYTES 4096
#define GCG_TOKENIZE_DROP (-2)
int32_t gcg_tokenize_tile_bytes(void);
gcg_status gcg_tokenize_mark_workspace_bytes(int64_t n_bytes, size_t* bytes);
gcg_status gcg_tokenize_mark(int64_t n_bytes, const uint8_t* text, const uint32_t* word_table,
                             int32_t lookbehind, uint8_t* flags, uint64_t* tile_base,
                             int64_t* totals_dev, void* workspace, size_t workspace_bytes,
                             gcg_stream_t stream);
gcg_status gcg_tokenize_terms_workspace_bytes(int64_t n_tokens, int32_t hash_bits, size_t* bytes);
gcg_status gcg_tokenize_terms(int64_t n_bytes, const uint8_t* text, const uint8_t* flags,
                              const uint64_t* tile_base, int64_t n_tokens, int64_t n_docs,
                              const int64_t* doc_off, int32_t hash_bits, int64_t* doc_ptr,
                              int32_t* tok_term, int64_t* term_start, int32_t* term_len,
                              int64_t* result_dev, void* workspace, size_t workspace_bytes,
                              gcg_stream_t stream);
gcg_status gcg_tokenize_remap_workspace_bytes(int64_t n_tokens, size_t* bytes);
gcg_status gcg_tokenize_remap(int64_t n_tokens, const int32_t* tok_term, int64_t n_terms,
                              const int32_t* action, int64_t n_docs, const int64_t* doc_ptr_in,
                              int32_t* tokens, int64_t* doc_ptr, void* workspace,
                              size_t workspace_bytes, gcg_stream_t stream);
/*
 * The @mentions of the mention graph by the same stages (graphconvgeo_amd/mentions.py,
 * mention_incidences_device): the regex (?<=^|(?<=[^a-zA-Z0-9-_\.]))@([A-Za-z]+[A-Za-z0-9_]+)
 * of the reference's data.py:311 as a rule over bytes. With L = [A-Za-z], N = [A-Za-z0-9_] and
 * P = N, '-' and '.', the byte '@' opens a mention iff the byte before it is not in P (or it is
 * the first byte of its document), the byte after it is in L and the one after that in N; the
 * name is the maximal run of N from the byte after the '@'. The classes are ASCII, so the rule
 * over UTF-8 bytes is the rule over code points. `text` as for gcg_tokenize_mark but NOT
 * lowercased: lowering changes what matches (U+212A becomes 'k').
 *
 * gcg_mention_mark: the outputs of gcg_tokenize_mark (same sizes, same workspace size), a token
 * being a name: its start is the byte after the '@'. They go to gcg_tokenize_terms_folded.
 *
 * gcg_tokenize_terms_folded: gcg_tokenize_terms, and with fold_ascii != 0 the bytes A-Z are
 * hashed and compared as a-z, so the spellings of a name are one term, numbered where the
 * first of them appears; term_start / term_len are that first spelling's (the caller lowers
 * it). The comparison stays exact: names that differ after folding under one hash set
 * result_dev[1]. fold_ascii = 0 is gcg_tokenize_terms. The workspace is
 * gcg_tokenize_terms_workspace_bytes'.
 *
 * The incidences are then a remap (action = the node id of each name) and a gcg_tfidf_count
 * over the remapped tokens: its indices are each document's distinct ids in ascending order.
 */
gcg_status gcg_mention_mark_workspace_bytes(int64_t n_bytes, size_t* bytes);
gcg_status gcg_mention_mark(int64_t n_bytes, const uint8_t* text, uint8_t* flags,
                            uint64_t* tile_base, int64_t* totals_dev, void* workspace,
                            size_t workspace_bytes, gcg_stream_t stream);
gcg_status gcg_tokenize_terms_folded(int64_t n_bytes, const uint8_t* text, const uint8_t* flags,
                                     const uint64_t* tile_base, int64_t n_tokens, int64_t n_docs,
                                     const int64_t* doc_off, int32_t hash_bits, int32_t fold_ascii,
                                     int64_t* doc_ptr, int32_t* tok_term, int64_t* term_start,
                                     int32_t* term_len, int64_t* result_dev, void* workspace,
                                     size_t workspace_bytes, gcg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GCG_SPMM_H */
