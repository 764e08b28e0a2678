/*
 * coldbrew_hip.h — C ABI of libcoldbrew_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary of the Cold Brew TeacherGNN hot path.  The reference has no FFI
 * of its own: its hot path bottoms out in third-party Python packages (dgl 0.7.0's
 * gspmm behind `graph.update_all`, torch's matmul / elementwise / Adam).  Each entry
 * point below replaces one of those call sites; the citation names the reference line
 * (paths relative to the reference root) whose work it does.
 *
 * Conventions (all functions):
 *   - plain pointers are DEVICE pointers unless the name says `host`; sizes are element counts;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call is
 *     asynchronous on that stream and re-entrant across streams;
 *   - nothing is allocated or freed: scratch memory comes from the caller
 *     (cb_*_workspace_bytes) and must stay alive until the stream has passed the call;
 *   - row-major matrices, leading dimension `ld` in elements; fp32 rows must be 4-byte
 *     aligned (16-byte alignment + ld % 4 == 0 enables the vector paths);
 *   - indices are int32 (E < 2^31, N < 2^31); edge_index arrives as int64 (PyG contract);
 *   - return value 0 = ok, negative = error (CB_E_*); cb_last_error() gives the
 *     thread-local message of the last failing call.
 */
#ifndef COLDBREW_HIP_H
#define COLDBREW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CB_OK 0
#define CB_E_INVALID (-1)   /* bad argument (null pointer, negative size, misaligned)  */
#define CB_E_RANGE (-2)     /* size does not fit the int32 index contract              */
#define CB_E_WORKSPACE (-3) /* workspace too small                                     */
#define CB_E_HIP (-4)       /* a HIP runtime call / kernel launch failed               */
#define CB_E_DEVICE (-5)    /* a kernel recorded a device-side error (cb_device_status) */

/* device-side error codes (first int of the device error word) */
#define CB_DEVERR_HANDOVER 1 /* the LDS tile hand-over of the aggregation + GEMM kernel gave up its bounded wait */
#define CB_DEVERR_GRADROWS 2 /* cb_rows_zero_outside_mask_f32 found a non-zero gradient row outside the loss rows */

int cb_version(void);
const char* cb_last_error(void);
/* Device-side errors are never silent: a kernel that gives up a bounded wait (the only such wait is the LDS tile hand-over of the
 * cb_spmm_gemm_* kernels: a lost hand-over would otherwise mean wrong numbers in a training run that has no parity test beside it)
 * records the reason in a word of device-visible host memory.  Every later cb_spmm_gemm_* call returns CB_E_DEVICE until
 * cb_device_status() has been called; cb_device_status() returns CB_OK, or CB_E_DEVICE with the reason in cb_last_error(), and clears
 * the word.  It does not synchronise — call it after the synchronisation that ends a step.  New relative to the reference (torch raises
 * on device faults by itself; GNN_model/GCN.py:238 + :225 are the work of those kernels). */
int cb_device_status(void);

/* Row-sparse backward (new; autograd of trainer_node_classification.py:390-391 `nll_loss(log_softmax(out[train_mask]))`): the gradient that
 * enters the model is zero in every row outside the loss rows, and so is everything the head and the last trunk store make of it — the
 * first reverse aggregation of the backward (autograd of GCN.py:238) then only has to gather the loss rows (graph.CSRGraph.filtered_t).
 * This call verifies the claim on the device: any non-zero element of g [rows, d] in a row with mask[row] == 0 records
 * CB_DEVERR_GRADROWS in the device error word (cb_device_status).  guard (may be NULL): an int32 in DEVICE memory the caller owns; a
 * violation also sets it to 1.  Handed to the optimiser launch that follows on the same stream (cb_adam_multi_norm_f32), it keeps the
 * truncated gradients of such a step away from the parameters and the moments without a host synchronisation in between; the caller
 * clears it when it handles the error. */
int cb_rows_zero_outside_mask_f32(const float* g, int64_t ld, int64_t rows, int64_t d, const uint8_t* mask, int32_t* guard, void* stream);

/* ------------------------------------------------------------------------------------
 * Graph ingest — replaces `dgl.graph((src_list, dst_list))` built through Python lists
 * (GNN_model/GCN.py:92-95) and the degree queries (GCN.py:188,206,243).
 *
 * src = edge_index[0], dst = edge_index[1], E columns, multigraph (duplicates kept).
 * Produces the by-dst CSR (rowptr/col: row v lists the sources u of edges u->v — the
 * forward aggregation) and the by-src CSR (rowptr_t/col_t: the reverse graph used by the
 * backward).  In-row order is ascending column id, so the arrays are a deterministic
 * function of the edge multiset.
 * flags[0] = #nodes with in-degree 0   (GCN.py:187-197 raises if non-zero)
 * flags[1] = #edges with an endpoint outside [0, N)  (arrays are invalid if non-zero)
 * flags[2] = 1 if the edge multiset is symmetric (by-src CSR == by-dst CSR), else 0
 * flags[3] = max in-degree
 * ---------------------------------------------------------------------------------- */
size_t cb_csr_workspace_bytes(int64_t E, int64_t N);
int cb_csr_from_coo_i64(const int64_t* src, const int64_t* dst, int64_t E, int64_t N,
                        int32_t* rowptr, int32_t* col, int32_t* rowptr_t, int32_t* col_t,
                        int32_t* flags /*[4]*/, void* workspace, size_t workspace_bytes, void* stream);

/* norm[v] = max(rowptr[v+1]-rowptr[v], 1)^-1/2 as fp32 — `degs.float().clamp(min=1)` then
 * `th.pow(degs, -0.5)` (GCN.py:206-208 with the by-src rowptr, GCN.py:243-245 with the by-dst rowptr). */
int cb_deg_norm_f32(const int32_t* rowptr, int64_t N, float* norm, void* stream);

/* E >= 2^31 on one device ("indices int32 (int64 rowptr if E >= 2^31)"; the reference's graph is int64 throughout,
 * GCN.py:93-94): the same ingest with int64 row pointers (column ids stay int32: N < 2^31; E < 2^32), the degree norms from them, and
 * cb_csr_rebase_i64: out[i] = rowptr[row0 + i] - rowptr[row0], i <= n_rows — the int32 row pointers of a row block with fewer than 2^31
 * edges, whose column ids start at col + rowptr[row0].  The aggregation kernels index edges with 32 bits inside a launch; the host cuts the
 * rows into such blocks (graph.SegmentedCSRGraph) and every entry point above runs per block, as it does on a rank's row block of the
 * node-sharded path. */
int cb_csr64_from_coo_i64(const int64_t* src, const int64_t* dst, int64_t E, int64_t N, int64_t* rowptr, int32_t* col, int64_t* rowptr_t,
                          int32_t* col_t, int32_t* flags /*[4]*/, void* workspace, size_t workspace_bytes, void* stream);
int cb_csr_rebase_i64(const int64_t* rowptr, int64_t row0, int64_t n_rows, int32_t* out, void* stream);
int cb_deg_norm_i64ptr_f32(const int64_t* rowptr, int64_t N, float* norm, void* stream);

/* ------------------------------------------------------------------------------------
 * Hub plan for the aggregation: rows longer than `hub_threshold` edges are split into
 * chunks of `hub_threshold` edges that separate wavefronts reduce (power-law graphs).
 * counts[0] = #hub rows, counts[1] = #chunks.  Call cb_spmm_hub_count, read counts on the
 * host, allocate hub_rows[counts[0]] and hub_chunk_ptr[counts[0]+1], call cb_spmm_hub_fill.
 * hub_rows comes back in ASCENDING row order (no atomics: the plan — and with it the order of every
 * sum a kernel takes over the hub rows — is the same in every process); scratch: int32
 * [cb_spmm_hub_fill_scratch_ints(N)].
 * ---------------------------------------------------------------------------------- */
int cb_spmm_hub_count(const int32_t* rowptr, int64_t N, int32_t hub_threshold, int32_t* counts /*[2]*/, void* stream);
int64_t cb_spmm_hub_fill_scratch_ints(int64_t N);
int cb_spmm_hub_fill(const int32_t* rowptr, int64_t N, int32_t hub_threshold, int32_t n_hubs,
                     int32_t* hub_rows, int32_t* hub_chunk_ptr, int32_t* scratch, void* stream);

/* ------------------------------------------------------------------------------------
 * The graph side of every aggregation call: one orientation's CSR, its hub plan and the workspace for the hub partial sums.
 * A HOST struct, passed by pointer and read during the call only (nothing retains it); the pointers inside are device pointers.
 * rowptr [n_rows + 1] / col [n_edges]: row v lists the rows that are summed into output row v.
 * hub_threshold / n_hubs / n_chunks / hub_rows / hub_chunk_ptr: the plan of cb_spmm_hub_count / cb_spmm_hub_fill above, made with this
 * rowptr and this hub_threshold.  With n_hubs == 0 (no plan) every row is reduced whole by one wavefront — correct for any graph, slow
 * for power-law hubs — and hub_rows / hub_chunk_ptr / ws may be NULL.
 * ws holds the hub partial sums: ws_bytes >= cb_spmm_workspace_bytes(n_chunks, d) for the d of the call.
 * col_flags = 0: `col` holds plain column ids.  col_flags = 1 (d % 256 == 0, fp32 rows 16-byte / bf16 rows 8-byte aligned only): bit 31 of
 * every id marks a HOT source row (one of the most-referenced rows, chosen at graph build so that together they fit the 256 MiB
 * Infinity Cache); hot rows are gathered with the default cache policy, all others with the streaming (nt) policy, which
 * keeps the re-used rows resident instead of letting 1e8 single-use 1 KiB rows evict them (-11 % per launch on the
 * 10M-node power-law graph, profiles/r02_spmm_gather_policy.md).  Results do not depend on the flags.  cb_spmm_csr_lp_f32 and
 * cb_spmm_csr_prop_f32 (narrow rows) take plain ids only.
 * ---------------------------------------------------------------------------------- */
typedef struct cb_csr_view {
  const int32_t* rowptr; const int32_t* col; int32_t col_flags;
  int64_t n_rows, n_edges;
  int32_t hub_threshold, n_hubs, n_chunks;
  const int32_t* hub_rows; const int32_t* hub_chunk_ptr;
  void* ws; size_t ws_bytes;
} cb_csr_view;
size_t cb_spmm_workspace_bytes(int64_t n_chunks, int64_t d);

/* ------------------------------------------------------------------------------------
 * Sum aggregation — replaces `graph.update_all(fn.copy_src('h','m'), fn.sum('m','h'))`
 * (GCN.py:198,238: DGL gspmm copy_lhs/sum) with the post-scale, bias (GCN.py:242-253) and
 * the ReLU that follows it in TricksComb.forward (GCN.py:127-128) fused as an epilogue:
 *
 *     out[v, :] = act( row_scale[v] * (acc_init[v, :] + sum_{j in [rowptr[v], rowptr[v+1])} col_scale[col[j]] * h[col[j], :]) + bias[:] )
 *
 * row_scale / bias / col_scale / acc_init may be NULL (factor 1 / no bias / factor 1 / sums start from 0); relu = 0/1 (here and in every
 * entry of this header the ReLU is torch.relu's function: +0 for every v <= 0, v above, and a NaN stays a NaN).  Called with the
 * by-dst CSR for the forward and with the by-src CSR (no epilogue) for the backward (autograd of gspmm = SpMM on the reverse graph).
 * Deterministic: every row is reduced in CSR order by one wavefront, hub rows in chunk order.
 * h_bf16 != 0: h holds bf16-stored rows (uint16_t, round-to-nearest-even; ld_h in bf16 elements, 8-byte aligned for the vector paths) —
 * the gathered rows (Z in the forward, b*dY' in the backward; the halo rows of the bf16 wire, COLDBREW_HALO_WIRE=bf16) take half the
 * traffic, accumulation and outputs stay fp32 (build extension = BASELINE config 2; the reference is fp32-only).
 * col_scale ([number of columns]; fp32 rows, d % 256 == 0, 16-byte aligned, no acc_init / bias / ReLU): a factor per SOURCE row, applied
 * as the row is gathered.  New: the row-sparse backward takes A (a * X_l) on the loss rows with it, i.e. the weight gradient
 * X_l^T (a * A^T dY) of GCN.py:213,238 contracted over the loss rows as ((A (a * X_l))[S_0])^T dY[S_0] — without a scaled copy of X_l.
 * acc_init ([n_rows, ld_init] fp32, read once, may alias out): the node-sharded aggregation in passes (new; the reference is
 * single-device).  A rank's row block of the CSR is split by column owner: the interior-column pass (no epilogue) runs
 * while the halo rows travel over xGMI; the halo-column pass starts from those raw sums and applies the epilogue once.  A raw in-place
 * pass — acc_init == out, no row scale / bias / ReLU: the intermediate halo slices — neither reads nor writes rows that have no edge
 * in this CSR.
 * ---------------------------------------------------------------------------------- */
int cb_spmm_csr_f32(const cb_csr_view* g, const void* h, int32_t h_bf16, int64_t ld_h, int64_t d, const float* col_scale,
                    const float* row_scale, const float* bias, int relu, const float* acc_init, int64_t ld_init,
                    float* out, int64_t ld_out, void* stream);


/* ------------------------------------------------------------------------------------
 * Elementwise / reduction stages around the GEMM + aggregation pairs (HBM-bound).
 * ---------------------------------------------------------------------------------- */

/* out[i] = x[i] * keep(seed, offset + i) / (1 - p) — `F.dropout(x, p, training=True)` of GCN.py:104,110,133.
 * keep() is a counter-based Philox4x32-10 draw of (seed, flat index): the backward calls the same
 * function on the gradient with the same seed instead of storing a mask; `offset` = flat index of x[0]
 * in the unsharded tensor (0 on one GPU), so row shards draw the mask of the full tensor.
 * In-place (out == x) is allowed. */
int cb_dropout_f32(const float* x, float* out, int64_t n, float p, uint64_t seed, const uint64_t* seed_dev, int64_t offset,
                   void* stream);
/* seed_dev (all dropout-bearing entry points; may be NULL): a device word added to `seed` at kernel time, so a step
 * captured in a hipGraph draws fresh masks on every replay (the host advances *seed_dev inside the graph). */

/* out = a*x + b*y — ResidualConnection / InitialConnection (res_tricks.py:14,23) and gradient sums. */
int cb_axpby_f32(float a, const float* x, float b, const float* y, float* out, int64_t n, void* stream);

/* Backward of the aggregation epilogue  Y = act(row_scale * R + bias)  (autograd of GCN.py:250,253 and
 * F.relu GCN.py:128) in one pass over [rows, d] contiguous matrices:
 *     gm = g * (act > 0)  (act == NULL: gm = g);  colsum[c] = sum_r gm[r,c]  (= dbias; NULL to skip);
 *     out[r,c] = gm[r,c] * row_scale[r]  (row_scale NULL: factor 1; out NULL: column sums only).
 * Column sums are reduced in a fixed order (ws: cb_colsum_workspace_bytes(rows, d)). */
size_t cb_colsum_workspace_bytes(int64_t rows, int64_t d);
int cb_act_bwd_f32(const float* g, const float* act, const float* row_scale, float* out, int64_t rows, int64_t d,
                   float* colsum, void* ws, size_t ws_bytes, void* stream);

/* out2[0] = ||x||_F (`th.norm(self.le)`, GCN.py:232), out2[1] = sum x^2; ws: cb_reduce_workspace_bytes(). */
size_t cb_reduce_workspace_bytes(void);
int cb_frobenius_norm_f32(const float* x, int64_t n, float* out2, void* ws, size_t ws_bytes, void* stream);

/* Fused `F.nll_loss(F.log_softmax(logits[mask], 1), y[mask])` (trainer_node_classification.py:390-391)
 * and its gradient: loss[0] = mean over the `count` rows with mask != 0 (mask NULL: all rows);
 * grad [rows, C] contiguous (NULL to skip) = (softmax - onehot) / count on masked rows, 0 elsewhere.
 * mask is one byte per row (torch.bool).  The label of a row that counts is range-checked as int64 before any use: outside [0, C) it is
 * never an index and never narrowed — the loss is NaN and so is that row of grad (the rule of the gathering kernels: a bad index is a NaN
 * row, not a read elsewhere).  Labels of rows with mask == 0 are not read (unlabeled nodes carry -1).  No ABI change. */
int cb_nll_logsoftmax_f32(const float* logits, int64_t ld, const int64_t* y, const uint8_t* mask, int64_t rows, int64_t C,
                          int64_t count, float* loss, float* grad, void* ws, size_t ws_bytes, void* stream);

/* One fused Adam update of a parameter tensor — `torch.optim.Adam(params, lr, weight_decay)` of
 * trainer_node_classification.py:310,430 (L2-style weight decay added to the gradient, bias-corrected
 * moments, step >= 1). */
int cb_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int64_t step, const int64_t* step_dev, void* stream);
/* The same update for n_tensors parameter tensors in ONE launch (host arrays of device pointers; the table travels in the
 * kernel arguments, 24 tensors per launch).  Identical arithmetic to cb_adam_step_f32.
 * extra_decay (may be NULL, entries may be NULL): per tensor, a device float added to weight_decay for that tensor.  With
 * extra_decay[i] = se_reg / ||le_i||_F the update of a structural-embedding table includes the gradient of the regulariser
 * `se_reg * ||le||_F` (GCN.py:232,236; trainer_node_classification.py:393) without materialising `le / ||le||` and without the
 * autograd accumulation into le.grad: 50 bytes / element less HBM traffic per table per step. */
int cb_adam_multi_f32(int32_t n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel,
                      const float* const* extra_decay, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                      const int64_t* step_dev, const int32_t* guard, void* stream);
/* step_dev (may be NULL): the step count read from device memory instead of `step` (hipGraph replay).
 * guard (may be NULL): int32 in device memory; while it is non-zero the launch leaves parameters and moments as they are (see
 * cb_rows_zero_outside_mask_f32); a norm requested from cb_adam_multi_norm_f32 is then the norm of those unchanged values. */
/* The same, and for every tensor with norm_out[i] != NULL also norm_out[i][0] = ||p_i||_F, [1] = ||p_i||_F^2 of the UPDATED tensor
 * (cb_frobenius_norm_f32's pair, same thread-to-element map and summation order when the tensor is the largest of its launch): the
 * next forward's `th.norm(self.le)` (GCN.py:232) costs no pass of its own over the table.  ws: cb_adam_norm_workspace_bytes(number of
 * non-NULL entries). */
size_t cb_adam_norm_workspace_bytes(int32_t n_norms);
int cb_adam_multi_norm_f32(int32_t n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel,
                           const float* const* extra_decay, float* const* norm_out, float lr, float beta1, float beta2, float eps,
                           float weight_decay, int64_t step, const int64_t* step_dev, const int32_t* guard, void* ws, size_t ws_bytes,
                           void* stream);

/* ------------------------------------------------------------------------------------
 * Dense fp32 contractions on the matrix cores.  Default: every fp32 operand is decomposed exactly into three
 * bf16 limbs and the six leading limb products run as v_mfma_f32_32x32x16_bf16 with fp32 accumulation (error
 * at the level of an fp32 GEMM, csrc/cb_gemm_limb.hip).  Operands that are not 16-byte aligned, or whose leading
 * dimensions / K / N are not multiples of 4, and every call when CB_GEMM_PLAIN_F32=1 is set in the environment,
 * use the fp32-input MFMA (v_mfma_f32_32x32x2_f32) instead.
 * Differences from an IEEE fp32 GEMM on the limb path: an infinite operand, or one above the largest bf16
 * (|x| > 3.39e38), yields NaN (inf - inf in the split) where fp32 would yield +-inf / a finite value; limbs that
 * fall below the smallest normal fp32 (|x| < ~2^-110) are flushed (absolute error < 2^-126).
 * ---------------------------------------------------------------------------------- */

/* C[M,N] = act( rowscale[m] * (A[M,K] @ B[K,N]) + addend[m,n] + bias[n] ) — `feat_src = feat * norm`,
 * `th.matmul(feat_src, weight)`, `+ self.le` (GCN.py:213,225,231) in one kernel (the row scale commutes
 * with the product); with bias/relu it is also nn.Linear + F.relu (GCN.py:105-106,138) and, fed with
 * gradients, the dX GEMMs of their backward.  rowscale/addend/bias may be NULL.
 * ws (optional, cb_gemm_nn_workspace_bytes(N, K) = 6 * K * N bytes + padding): room for B split ONCE per launch into its three
 * bf16 planes, pre-arranged as the kernel's LDS image — B is the small weight matrix, so this replaces the per-block,
 * per-K-step split of the same values by a straight 16-byte copy.  ws == NULL: every block splits its own copy. */
size_t cb_gemm_nn_workspace_bytes(int64_t N, int64_t K);
/* Few output tiles, long contraction (x @ W_0 of a Cora-sized graph, 2 708 x 1 433 x 64: GCN.py:105) on the fp32-input
 * fallback kernel: with ws of cb_gemm_nn_splitk_workspace_bytes(M, N, K) bytes (0 = the shape is not split) the K range is
 * cut into chunks contracted by different blocks and summed in a fixed order before the epilogue.  Without ws: one block
 * per output tile walks the whole K range (same result up to the summation order). */
size_t cb_gemm_nn_splitk_workspace_bytes(int64_t M, int64_t N, int64_t K);
int cb_gemm_nn_f32(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int64_t N,
                   int64_t K, const float* rowscale, const float* addend, int64_t ld_add, const float* bias, int relu,
                   void* ws, size_t ws_bytes, void* stream);
/* The same contraction with a second output C2 = dropout_p(C) written by the same epilogue (the value is in registers
 * anyway): `X = relu(Linear_0(x)); X_dropped = F.dropout(X)` of the residual trunk (GCN.py:105-107,110) without re-reading
 * X.  C2's keep-mask equals the one cb_dropout_f32 draws for (seed, seed_dev, offset = row0 * N).  Falls back to
 * cb_gemm_nn_f32 + cb_dropout_f32 (contiguous outputs) when the fused epilogue does not cover the shape. */
int cb_gemm_nn_drop2_f32(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, float* C2, int64_t ldc2,
                         int64_t M, int64_t N, int64_t K, const float* rowscale, const float* addend, int64_t ld_add, const float* bias,
                         int relu, float drop_p, uint64_t seed, const uint64_t* seed_dev, int64_t row0, void* ws, size_t ws_bytes, void* stream);
/* C[K1,K2] = sum_m A[m,K1] * rowscale[m] * G[m,K2] — the weight gradients (autograd of GCN.py:225 and
 * of nn.Linear): a reduction over the node axis, split into row slabs whose partial products are summed
 * in a fixed order (ws: cb_gemm_tn_workspace_bytes).  rowscale may be NULL. */
size_t cb_gemm_tn_workspace_bytes(int64_t M, int64_t K1, int64_t K2);
int cb_gemm_tn_f32(const float* A, int64_t lda, const float* G, int64_t ldg, const float* rowscale, float* C, int64_t M,
                   int64_t K1, int64_t K2, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused residual trunk (type_trick with 'Initial', no bare norm: the default configs of
 * Pubmed / ogbn-arxiv / the synthetic power-law benchmark).
 *
 * The trunk's STORE — GCN.py:127-133 of layer l and GCN.py:110 of layer l+1, applied to a pre-activation y wherever a kernel has it in registers:
 *     act  = relu(y)                                                               (GCN.py:128)
 *     next = dropout_{seed,p}( c_act * act + c_mix * mix_src[mix row] )            (res_tricks.py:7-23, GCN.py:110/133)
 * One argument of every entry that applies it: a HOST struct, passed by pointer and read during the call only (nothing retains it); the pointers
 * inside are device pointers.  `next` (and what else the entry writes) is the entry's own argument.
 * mix_src [., ld_mix] (NULL: no mix, next = dropout(act)): read at the node row; mix_index (NULL: none; int64, one entry per stored row; the entries
 * over a SUBSET of the node rows only — cb_*_store_rows_f32): mix_src is a compact matrix, read at row mix_index[r].
 * drop_p in [0, 1) (0: no dropout).  The keep-mask is cb_dropout_f32's draw for (seed, seed_dev, flat index (row0 + node row) * d + column): row0 =
 * global index of node row 0 (the dropout mask of the unsharded tensor), seed_dev as in cb_dropout_f32.
 * relu_bits [node rows][d/256][4] uint64 (NULL: not written) receives the backward mask of the store (word k, bit l = column 256*tile + 4*l + k): set
 * where the element passes gradient to the pre-activation, i.e. act > 0 AND the dropout keeps it (p = 0: the ReLU mask); bits_relu_only != 0: act > 0
 * alone (the 'Residual' connection, res_tricks.py:7-14: layer l+1's mix sends a second gradient through this ReLU under ANOTHER dropout mask — the
 * backward kernels regenerate the keep masks anyway).
 * out_act [., ld_act] (NULL: not written): the activation itself (the mix source of the next 'Residual' layer), at the row `next` is written at.
 * d must be a multiple of 256; mix_src / out_act rows 16-byte aligned with a leading dimension that is a multiple of 4 and >= d; relu_bits 8-byte
 * aligned.  An entry that has no kernel for an option returns CB_E_INVALID.  96 bytes.
 * ---------------------------------------------------------------------------------- */
typedef struct cb_trunk_store {
  const float* mix_src; int64_t ld_mix; const int64_t* mix_index;
  float c_act, c_mix, drop_p;
  uint64_t seed; const uint64_t* seed_dev; int64_t row0;
  uint64_t* relu_bits; int32_t bits_relu_only;
  float* out_act; int64_t ld_act;
} cb_trunk_store;

/* The store folded into the aggregation's store:  y = row_scale[v] * sum_j h[col[j]] + bias  (GCN.py:238-253); out_next = the store's `next`.
 * h_bf16 / acc_init ([n_rows, ld_init], 16-byte aligned rows; NULL: none) as in cb_spmm_csr_f32: bf16-stored source rows, and the fused store as
 * the LAST pass of a node-sharded aggregation on top of the running sums.
 * row_ids (int32 [n_rows], ascending; NULL: none; fp32 rows, no acc_init): the CSR's rows are a SUBSET of the node rows — row r of rowptr / row_scale /
 * out_act / out_next is node row row_ids[r]; mix_src, relu_bits ([all node rows][d/256][4]) and the dropout mask are taken at the node row.  The
 * rows-only training forward (trunk.py): a GCNConv + store (GCN.py:205-256,127-133) evaluated only on the rows the layers above read.
 * No mix_index: the mix is taken at the node row. */
int cb_spmm_csr_fused_f32(const cb_csr_view* g, const int32_t* row_ids, const void* h, int32_t h_bf16, int64_t ld_h, int64_t d,
                          const float* row_scale, const float* bias, const float* acc_init, int64_t ld_init, const cb_trunk_store* store,
                          float* out_next, int64_t ld_next, void* stream);

/* Backward of that epilogue in one pass over contiguous [rows, d]:
 *     gm = dropout_bwd(g);  gx0 = (accumulate ? gx0 : 0) + c_mix * gm  (gx0 NULL: skipped);
 *     gy = c_act * gm * relu_bit;  colsum = sum_rows gy (dbias; NULL to skip);  out = gy * row_scale[r]. */
int cb_trunk_layer_bwd_f32(const float* g, const uint64_t* relu_bits, const float* row_scale, void* out, int out_bf16, float* gx0,
                           int accumulate, int64_t rows, int64_t d, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                           int64_t row0, float c_act, float c_mix, const float* g2, uint64_t seed2, float c2, const int32_t* g2_pos, float* colsum,
                           void* ws, size_t ws_bytes, void* stream);
/* g2 (may be NULL): 'Residual' connection (res_tricks.py:7-14) — the layer's ReLU output also is the mix source of the NEXT layer, so
 *     gy = (c_act * dropout_bwd_seed(g) + c2 * dropout_bwd_seed2(g2)) * relu_bit     (g2 = gradient w.r.t. the next layer's stored output;
 * relu_bits written with bits_relu_only).  g2_pos (may be NULL; int32 [rows of the full matrix]): g2 is a COMPACT matrix of a row-sparse backward —
 * full row r sits at g2_pos[r], absent (= zero) where that is negative. */
/* (out_bf16 != 0: `out` is a bf16 [rows, d] matrix — gradient rows stored in bf16 for the bf16 aggregation variant.) */
/* cb_trunk_layer_bwd_f32 for layer 0 of the 'Initial' trunk (all rows, fp32 out, no in-place accumulator) that also FOLDS the gradients the residual mixes send
 * to X0 (InitialConnection, res_tricks.py:19-23, each under its own store's dropout GCN.py:110,133) — round 6, the elementwise form of
 * cb_spmm_csr_store_bwd_mix_f32's epilogue for the levels whose reverse aggregation does not carry the store backward:
 *   out_m = c_mix * ( dropout_bwd_seed(g) + sum_q dropout_bwd_{mix_seeds[q]}(mix_g[q][mix_pos[q][r] | r]) )      n_mix <= 2 operands (host arrays); mix_pos[q] NULL: a
 * dense [rows, d] operand, else int32 [rows] positions in a compact one (< 0: absent).  out / colsum: exactly cb_trunk_layer_bwd_f32's (bit-identical).  The
 * input stage then reads out_m beside dL/d dropout(X0): cb_gemm_tn_instage_f32.  colsum2 (may be NULL): the column sums of cs_c * dropout_bwd(mix_g[cs_src]) through
 * the mask words cs_bits (indexed by the node row) — the bias gradient (GCN.py:253) of a store whose backward cb_spmm_csr_store_bwd_f32 applied, as
 * cb_trunk_input_bwd_multi_cs_f32 returns it; ws2: cb_colsum_workspace_bytes(rows, d). */
int cb_trunk_layer_bwd_fold_f32(const float* g, const uint64_t* relu_bits, const float* row_scale, float* out, int64_t rows, int64_t d, float drop_p,
                                uint64_t seed, const uint64_t* seed_dev, int64_t row0, float c_act, float c_mix, int32_t n_mix, const float* const* mix_g,
                                const int32_t* const* mix_pos, const uint64_t* mix_seeds, float* out_m, float* colsum, void* ws, size_t ws_bytes, int32_t cs_src,
                                const uint64_t* cs_bits, float cs_c, float* colsum2, void* ws2, size_t ws2_bytes, void* stream);
/* The same over a SUBSET of the rows (row-sparse backward: the loss rows): g / out are compact [n_rows, d] matrices holding rows
 * row_index[0 .. n_rows) (ascending) of the full ones; relu_bits / row_scale are the full arrays; the dropout mask is the global row's. */
int cb_trunk_layer_bwd_rows_f32(const float* g, const int64_t* row_index, int64_t n_rows, const uint64_t* relu_bits, const float* row_scale, float* out,
                                int64_t d, float drop_p, uint64_t seed, const uint64_t* seed_dev, int64_t row0, float c_act, const float* g2, uint64_t seed2,
                                float c2, const int32_t* g2_pos, float* colsum, void* ws, size_t ws_bytes, void* stream);
/* (g2 / seed2 / c2 / g2_pos as in cb_trunk_layer_bwd_f32; g2_pos is required with g2: the two compact matrices live on different supports.) */

/* Backward into the trunk's input stage X0 = relu(Linear(dropout(x))) (GCN.py:104-107,110):
 *     out = (add + dropout_bwd(g)) * (act > 0);  colsum = sum_rows out  (bias gradient of the input Linear). */
int cb_trunk_input_bwd_f32(const float* g, const float* add, const float* act, float* out, int64_t rows, int64_t d, float drop_p,
                           uint64_t seed, const uint64_t* seed_dev, int64_t row0, float* colsum, void* ws, size_t ws_bytes,
                           void* stream);

/* The same input stage with the X0 gradient gathered in one pass (no [rows, d] accumulator is read-modify-written per layer):
 *     out = ( dropout_bwd_seed(g) + c_mix * sum_{l < n_mix} dropout_bwd_seeds_mix[l](g_mix[l]) ) * (act > 0)
 * g_mix[l] = gradient w.r.t. the output of layer l's fused store (host array of n_mix <= 7 device pointers); used with
 * cb_trunk_layer_bwd_f32(gx0 = NULL).  Autograd of GCN.py:104-110 + res_tricks.py:23 for every layer at once.
 * act_bits (may be NULL): [rows][d / 256][4] mask words of (act > 0) used instead of act (act may then be NULL).
 * g_mix_pos (may be NULL): host array of n_mix device pointers (entries may be NULL); where g_mix_pos[l] is set (int32 [rows]), g_mix[l] is a
 * COMPACT matrix that holds only some rows (the support rows of a row-sparse backward) — row r at position g_mix_pos[l][r], absent (= zero)
 * where that is negative. */
int cb_trunk_input_bwd_multi_f32(const float* g, uint64_t seed, int32_t n_mix, const float* const* g_mix, const uint64_t* seeds_mix,
                                 float c_mix, const float* act, float* out, int64_t rows, int64_t d, float drop_p,
                                 const uint64_t* seed_dev, int64_t row0, float* colsum, void* ws, size_t ws_bytes,
                                 const uint64_t* act_bits, const int32_t* const* g_mix_pos, void* stream);
/* The same, which also returns n_cs (<= 2) extra column sums (host arrays of n_cs entries): colsum2[q] = the column sums of cs_c[q] *
 * dropout_bwd_{seeds_mix[cs_src[q]]}(g_mix[cs_src[q]]) where the mask words cs_bits[q] ([rows][d / 256][4], indexed by the node row also for a compact operand)
 * have the element's bit: the bias gradients (GCN.py:253) of the layers whose store backward was applied by the reverse aggregation's own epilogue
 * (cb_spmm_csr_store_bwd_f32) — this pass reads those gradients anyway.  ws2: n_cs planes of cb_colsum_workspace_bytes(rows, d).  A dense operand's sum
 * has the partial-sum order of cb_trunk_layer_bwd_f32's (bit-identical). */
int cb_trunk_input_bwd_multi_cs_f32(const float* g, uint64_t seed, int32_t n_mix, const float* const* g_mix, const uint64_t* seeds_mix,
                                    float c_mix, const float* act, float* out, int64_t rows, int64_t d, float drop_p,
                                    const uint64_t* seed_dev, int64_t row0, float* colsum, void* ws, size_t ws_bytes,
                                    const uint64_t* act_bits, const int32_t* const* g_mix_pos, int32_t n_cs, const int32_t* cs_src,
                                    const uint64_t* const* cs_bits, const float* cs_c, float* const* colsum2, void* ws2, size_t ws2_bytes, void* stream);
/* A (reverse) aggregation whose epilogue is the BACKWARD of the trunk's store of the rows it writes — autograd of GCN.py:127-133 applied to the output of
 * the autograd of GCN.py:238 in one kernel:
 *   g = row_scale * sum_{u in row v} h[u]              -> out_g (may be NULL): dL/d(stored, dropped activation), the input stage's mix operand
 *   out_gr = bwd_rowscale[v] * c_act * dropout_bwd_seed(g) where relu_bits (READ: the forward store's mask words) has the element's bit, else 0
 * = cb_spmm_csr_f32 followed by cb_trunk_layer_bwd_f32 (gx0 = NULL, no second gradient) without that pass's read of g; values bit-identical.  The
 * pass's column sums (the bias gradient) come from cb_trunk_input_bwd_multi_cs_f32.  d % 256 == 0, fp32 rows, 16-byte aligned. */
int cb_spmm_csr_store_bwd_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale, const uint64_t* relu_bits,
                              const float* bwd_rowscale, float c_act, float drop_p, uint64_t seed, const uint64_t* seed_dev, int64_t row0,
                              float* out_g, int64_t ld_g, float* out_gr, int64_t ld_gr, void* stream);
/* The same on ALL node rows, with the mix gradients FOLDED (round 6): the first output is not the raw g but everything this store and the layers above
 * send to X0 through their residual mixes (InitialConnection, res_tricks.py:19-23: X = (1 - alpha) X_l + alpha X_0, each under its own store's dropout
 * GCN.py:110,133):
 *   out_m = c_mix * ( dropout_bwd_seed(g) + sum_q dropout_bwd_{mix_seeds[q]}(mix_g[q][mix_pos[q][v]]) )          n_mix <= 2 compact operands (host arrays);
 * mix_pos[q] (int32 [N]): position of node row v in operand q, < 0 where it holds no such row.  out_gr as above (bit-identical).  colsum (may be NULL; [d]) =
 * column sums of out_gr / bwd_rowscale: the bias gradient (GCN.py:253) of the store whose backward this is; ws2 = cb_spmm_store_bwd_mix_workspace_bytes.
 * The input stage then reads ONE [N, d] matrix beside dL/d dropout(X0): cb_gemm_tn_instage_f32. */
size_t cb_spmm_store_bwd_mix_workspace_bytes(int64_t N, int64_t n_hubs, int64_t d);
int cb_spmm_csr_store_bwd_mix_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale, const uint64_t* relu_bits,
                                  const float* bwd_rowscale, float c_act, float drop_p, uint64_t seed, const uint64_t* seed_dev, int64_t row0,
                                  float* out_m, int64_t ld_m, float* out_gr, int64_t ld_gr, int32_t n_mix, const float* const* mix_g,
                                  const int32_t* const* mix_pos, const uint64_t* mix_seeds, float c_mix, float* colsum, void* ws2, size_t ws2_bytes,
                                  void* stream);

/* bf16-storage variant of the dense transform in front of the aggregation (build extension = BASELINE config 2; the reference is fp32-only):
 * C is stored as bf16 (round-to-nearest-even) for cb_spmm_csr_f32 / cb_spmm_csr_fused_f32 with h_bf16; everything else as cb_gemm_nn_f32. */
int cb_gemm_nn_bf16out_f32(const float* A, int64_t lda, const float* B, int64_t ldb, uint16_t* C, int64_t ldc, int64_t M, int64_t N,
                           int64_t K, const float* rowscale, const float* addend, int64_t ld_add, const float* bias, int relu,
                           void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Normalisation tricks (GNN_model/norm_tricks.py) as fused reductions; all matrices contiguous [rows, d].
 * ---------------------------------------------------------------------------------- */
/* node_norm (norm_tricks.py:53-84): y = (x - c*mu_r) * std_r^-q, mu/std over the features of row r
 * (std = sqrt(biased var + eps)); 'n': c=1,q=1; 'v': c=0,q=1; 'm': c=1,q=0; 'srv'/'pr': c=0,q=0.5.
 * stats2 [rows][2] = (mu, std) is written by the forward (may be NULL) and read by the backward. */
int cb_node_norm_fwd_f32(const float* x, float* y, float* stats2, int64_t rows, int64_t d, float c, float q, float eps, void* stream);
int cb_node_norm_bwd_f32(const float* x, const float* g, const float* stats2, float* dx, int64_t rows, int64_t d, float c, float q,
                         void* stream);
/* Column statistics in one pass: colsum[c] = sum_r x[r,c]; colsum2[c] = sum_r x[r,c]^2 (w == NULL) or
 * sum_r x[r,c]*w[r,c] — the reductions behind mean_norm / pair_norm / BatchNorm1d (norm_tricks.py:25-41,106,132)
 * and their backward; fixed-order two-stage reduce (ws: cb_colstats_workspace_bytes).
 * shift [d] (may be NULL) centres them about a per-column pivot, so that a column mean that is large against the
 * column's spread does not cancel:  w == NULL: colsum = sum_r (x - shift), colsum2 = sum_r (x - shift)^2;
 * w != NULL: colsum = sum_r x, colsum2 = sum_r x * (w - shift). */
size_t cb_colstats_workspace_bytes(int64_t rows, int64_t d);
int cb_colstats_f32(const float* x, const float* w, const float* shift, int64_t rows, int64_t d, float* colsum, float* colsum2,
                    void* ws, size_t ws_bytes, void* stream);
/* y[r,c] = ((x[r,c] - shift[c]) * scale[c]) * gscale + bias[c]  (vectors may be NULL). */
int cb_col_affine_f32(const float* x, const float* shift, const float* scale, const float* bias, float gscale, float* y, int64_t rows,
                      int64_t d, void* stream);
/* dx[r,c] = a[c]*ga*g[r,c] + b[c]*gb*(xh[r,c] - xs[c]) + e[c]  (xh, xs, a, b, e may be NULL: a,b default 1, xs default 0) — the
 * backward of the column norms. */
int cb_col_bwd_combine_f32(const float* g, const float* xh, const float* xs, const float* a, const float* b, const float* e, float ga,
                           float gb, float* dx, int64_t rows, int64_t d, void* stream);

/* ------------------------------------------------------------------------------------
 * Teacher -> student hand-off: `SEMLP.replacement` (MLP_model/__init__.py:143-156), a per-node
 * Python loop of [1,N] matmuls + argsort in the reference.  For every query row q_i [D]:
 *     s_j = <q_i, t_j> over the N teacher rows;  sel = the K largest (ties: larger index);
 *     out_i = sum_k softmax(s_sel)_k * t_sel_k          (contiguous out [B, D])
 * One fp32-MFMA sweep with a running top-K in LDS (the B x N score matrix is never written) + a merge kernel.
 * out_idx [B,K] / out_w [B,K] (nullable) receive the selection and the softmax weights in ascending score order
 * (the order of `sortidx[-K:]`).  1 <= K <= 8.  ws: cb_topk_replace_workspace_bytes(B, N, K).
 * Ties follow one total order: larger score first, then larger index — what a stable ascending argsort followed by [-K:]
 * selects (torch's default argsort is not stable, so the reference itself leaves ties open).
 * NaN: a query row that holds a NaN scores NaN against every teacher row and has no winner; its out row and its K weights
 * are NaN and its K indices -1, as the reference's softmax of NaN scores propagates it.  The other rows are unaffected.
 * NaN in individual teacher rows is outside the contract: such a row never wins, and what the remaining rows yield is not
 * specified.
 * ---------------------------------------------------------------------------------- */
size_t cb_topk_replace_workspace_bytes(int64_t B, int64_t N, int64_t K);
int cb_topk_replace_f32(const float* q, int64_t ldq, const float* t, int64_t ldt, int64_t B, int64_t N, int64_t D, int32_t K,
                        float* out, int32_t* out_idx, float* out_w, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Device-side graph analysis in front of the path (per-edge Python dict / list loops in the reference).
 * Integer work, bit-exact, order-preserving (outputs list elements in input order, as np.where and the reference's append
 * loops do).  ws for the compactions: cb_compact_workspace_bytes(n elements scanned).
 * ---------------------------------------------------------------------------------- */
/* counts[v] = #{e : ids[e] == v}, v in [0, N)  — graph_analyze (utils.py:300-334): out-degree from edge_index[0], in-degree
 * from edge_index[1].  *n_bad = ids outside [0, N) (not counted). */
int cb_id_count_i64(const int64_t* ids, int64_t E, int64_t N, int32_t* counts, int32_t* n_bad, void* stream);
/* hist[b] = #{i : vals[i] == b}, b in [0, n_bins)  — the degree-value histogram from which every repeated median of
 * get_partial_sorted_idx (utils.py:910-941) is read. */
int cb_value_hist_i32(const int32_t* vals, int64_t N, int32_t n_bins, int32_t* hist, int32_t* n_bad, void* stream);
size_t cb_compact_workspace_bytes(int64_t n);
/* out_idx[0 .. *count) = ascending indices i with lo <= vals[i] <= hi; out_mask[i] = 1 for them, 0 otherwise (either output
 * may be NULL)  — np.where(arr <= median) / (arr >= median) of get_partial_sorted_idx and the *_deg_mask vectors of
 * save_graph_analyze (utils.py:694-717). */
int cb_select_range_i32(const int32_t* vals, int64_t N, int32_t lo, int32_t hi, int64_t* out_idx, uint8_t* out_mask, int64_t* count,
                        void* ws, size_t ws_bytes, void* stream);
/* craft_isolation_v2 (utils.py:731-752): keeps edge e, in order, unless src[e] != dst[e] and (node_flag[src[e]] or
 * node_flag[dst[e]]).  out_src / out_dst need room for E entries; *count = edges kept. */
int cb_craft_isolation_i64(const int64_t* src, const int64_t* dst, int64_t E, const uint8_t* node_flag, int64_t N, int64_t* out_src,
                           int64_t* out_dst, int64_t* count, void* ws, size_t ws_bytes, void* stream);
/* ensure_symmetric (utils.py:667-674) / to_undirected as load_ogbn uses it (trainer_node_classification.py:574): the edge set
 * united with its transpose, duplicates removed, sorted by (row, col).  out_row / out_col need room for 2E entries. */
size_t cb_symmetrize_workspace_bytes(int64_t E, int64_t N);
int cb_symmetrize_i64(const int64_t* src, const int64_t* dst, int64_t E, int64_t N, int64_t* out_row, int64_t* out_col, int64_t* count,
                      int32_t* n_bad, void* ws, size_t ws_bytes, void* stream);

/* out[i, :] = src[idx[i], :] (contiguous out [n_idx, d]) — packs the rows a peer asked for before the
 * all-to-all of the node-sharded halo exchange (new; the reference is single-device). */
int cb_gather_rows_f32(const float* src, int64_t ld, const int64_t* idx, int64_t n_idx, int64_t d, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Aggregation + the NEXT dense transform in one kernel (csrc/cb_agg_gemm.hip): a block aggregates 64 rows exactly as
 * cb_spmm_csr_f32 / cb_spmm_csr_fused_f32 do (same stores: the aggregated matrix still goes to memory), keeps them in LDS and
 * multiplies the tile by a 256 x 256 matrix B on the matrix cores before anything else is read:
 *     g_out[v, :] = g_rowscale[v] * (out[v, :] @ B) + g_addend[v, :]           (bit-identical to cb_gemm_nn_f32 on `out`)
 * Replaces, per layer of the residual trunk: forward  GCN.py:238-253,127-133 followed by :213,225,230-235 of the next layer
 * (cb_spmm_csr_fused_f32 + cb_gemm_nn_f32); backward autograd of :238 followed by autograd of :213,225
 * (cb_spmm_csr_f32 on the reverse CSR + cb_gemm_nn_f32 with W^T).  d must be 256; fp32 rows, 16-byte aligned.
 * image: B split once into bf16 limbs in MFMA fragment order by cb_agg_gemm_image_f32 (transpose = 1: B = W^T);
 * cb_agg_gemm_image_bytes(256, 256) bytes, 16-byte aligned, L2 resident (384 KB).
 * acc_init (may be NULL; [N, ld_init] fp32, may alias the aggregated output): the reduction of a row starts from these partial sums — the
 * LAST pass of a node-sharded aggregation (cb_spmm_csr_f32 / cb_spmm_csr_fused_f32 with acc_init + the GEMM), so that a rank's last halo
 * pass also produces the next layer's Z / this layer's dX.
 * A tile hand-over that times out is recorded in the device error word (cb_device_status); these calls return CB_E_DEVICE while it is set.
 * ---------------------------------------------------------------------------------- */
size_t cb_agg_gemm_image_bytes(int64_t K, int64_t N);
int cb_agg_gemm_image_f32(const float* W, int64_t ld, int64_t K, int64_t N, int transpose, void* image, size_t image_bytes, void* stream);
int cb_spmm_gemm_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale, const float* bias, int relu,
                     const float* acc_init, int64_t ld_init, float* out, int64_t ld_out, const void* image, const float* g_rowscale,
                     const float* g_addend, int64_t ld_add, float* g_out, int64_t ld_gout, void* stream);
/* skip_next != 0: a forward that no backward follows (evaluation / metrics passes, GCN.py:100-140 under no_grad): the stored activations have
 * no reader — the next layer's Z leaves this kernel — so the rows the persistent kernel finishes are NOT written to out_next (the hub rows
 * pass through it, its other contents are undefined afterwards; NULL is accepted when n_hubs == 0).  g_out as above.  store: cb_trunk_store, as
 * cb_spmm_csr_fused_f32 applies it on all node rows (no mix_index). */
int cb_spmm_gemm_fused_f32(const cb_csr_view* g, const float* acc_init, int64_t ld_init, const float* h, int64_t ld_h, int64_t d,
                           const float* row_scale, const float* bias, const cb_trunk_store* store, float* out_next, int64_t ld_next,
                           int32_t skip_next, const void* image, const float* g_rowscale, const float* g_addend, int64_t ld_add, float* g_out,
                           int64_t ld_gout, void* stream);
/* The output Linear as the tail of the LAST layer's aggregation (round 5): GCN.py:133-138 `layers_MLP[-1](F.dropout(x))` reads exactly the rows
 * the last trunk store has just made — logits = out_next @ W_out^T + b_out leave the aggregation kernel (C <= 64 classes; the four multiplying
 * wavefronts of a block take the four 32 x 32 blocks of a tile's 64 x 64 output), the separate head GEMM and its re-read of the [N, 256]
 * activations disappear.  Same limb products in the same order as cb_gemm_nn_f32.  head_image: cb_agg_gemm_head_image_f32 of the nn.Linear
 * weight [C, 256] (transpose = 1) — 256 x 64 with zero columns beyond C; logits [N, ld_logits >= C], 16-byte aligned.  Other arguments as
 * cb_spmm_gemm_fused_f32.  skip_next != 0: a forward that no backward follows — the last layer's activations are not written at all. */
size_t cb_agg_gemm_head_image_bytes(int64_t K, int64_t C);
int cb_agg_gemm_head_image_f32(const float* W, int64_t ld, int64_t K, int64_t C, int transpose, void* image, size_t image_bytes, void* stream);
int cb_spmm_gemm_fused_head_f32(const cb_csr_view* g, const float* acc_init, int64_t ld_init, const float* h, int64_t ld_h, int64_t d,
                                const float* row_scale, const float* bias, const cb_trunk_store* store, float* out_next, int64_t ld_next,
                                int32_t skip_next, const void* head_image, const float* head_bias, int64_t C, float* logits, int64_t ld_logits,
                                void* stream);
/* Fault injection for the failure path above (tests): one wavefront waits with a short spin bound for a hand-over that never comes;
 * cb_device_status() must then report CB_E_DEVICE. */
int cb_agg_gemm_handover_selftest(void* stream);

/* ------------------------------------------------------------------------------------
 * The forward front of the residual trunk in one kernel (csrc/cb_front.hip): GNN_model/GCN.py:104-107 (dropout of x, input Linear, ReLU),
 * :110 (dropout in front of layer 0) and :213,225,230-235 (first GCNConv's transform):
 *     X0 = relu(dropout_{seed_x}(x) @ W_in^T + bias_in)                  -> x0 [M, 256] (+ relu_bits [M][4]: mask words of X0 > 0, may be NULL)
 *     Z0 = rowscale * (dropout_{seed_x0}(X0) @ W_0) + addend             -> z0 [M, 256]
 * dropout(X0) never leaves the chip unless x0_drop is given (then it is also stored: the backward's weight gradient can read it instead of
 * regenerating the mask, cb_gemm_tn_adrop_f32).  drop_p = 0: no dropout.  Bit-identical to cb_gemm_nn_indrop_drop2_f32 + cb_gemm_nn_f32.
 * image_in / image_0: cb_front_image_f32 of W_in (nn.Linear layout [256, K], transpose = 1) and of W_0 ([256, 256], transpose = 0);
 * K (input features) in {64, 128} — cb_front_image_bytes(K) == 0 says "no forward-front kernel for this K" — and hidden width 256.
 * ---------------------------------------------------------------------------------- */
size_t cb_front_image_bytes(int64_t K);
int cb_front_image_f32(const float* W, int64_t ld, int64_t K, int transpose, void* image, size_t image_bytes, void* stream);
int cb_trunk_front_f32(const float* x, int64_t ld_x, int64_t M, int64_t K, const void* image_in, const float* bias_in, const void* image_0,
                       const float* rowscale, const float* addend, int64_t ld_add, float* x0, int64_t ld_x0, uint64_t* relu_bits, float* x0_drop,
                       int64_t ld_drop, float* z0, int64_t ld_z, float drop_p, uint64_t seed_x, uint64_t seed_x0, const uint64_t* seed_dev,
                       int64_t row0, void* stream);

/* Edge-weighted aggregation — the `edge_weight` argument of GCNConv.forward (GNN_model/GCN.py:199-202: fn.u_mul_e + fn.sum):
 *     out[v, :] = act( row_scale[v] * sum_{j in row v} w[j] * h[col[j], :] + bias[:] ),   w in CSR order ([E], fp32)
 * and the gradient of the weights, dw[j] = <h[col[j], :], g[row of j, :]>.  The reference asserts len(edge_weight) == E (:200);
 * TricksComb never passes one, so these are plain one-wavefront-per-row kernels (exact, deterministic), not the tuned stream. */
int cb_spmm_csr_weighted_f32(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int64_t E, const float* h, int64_t ld_h,
                             int64_t d, const float* row_scale, const float* bias, int relu, float* out, int64_t ld_out, void* stream);
int cb_spmm_edge_dot_f32(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t E, const float* h, int64_t ld_h, const float* g,
                         int64_t ld_g, int64_t d, float* dw, void* stream);

/* Dropout of an OPERAND while it is staged (GCN.py:104: `x = F.dropout(x)` in front of layers_MLP[0] of the residual trunk): the input
 * Linear reads the undropped features and applies the keep-mask cb_dropout_f32(x, ..., a_seed, seed_dev, offset = row0 * K) draws as it
 * splits them into limbs — no dropped copy is written, kept or re-read; the weight gradient regenerates the same mask:
 *     C = act(dropout(A) @ B + bias), C2 = dropout_{seed}(C)            cb_gemm_nn_indrop_drop2_f32   (else: cb_dropout_f32 + cb_gemm_nn_drop2_f32)
 *     C = A^T @ dropout(G)                                              cb_gemm_tn_gdrop_f32          (else: cb_dropout_f32 + cb_gemm_tn_f32)
 * Results are bit-identical to the two-kernel forms.  The *_supported queries (1 / 0) say whether the fused form exists for a shape.  * relu_bits (may be NULL; N == 256 and relu only): [M][4] mask words of (C > 0), in the layout of the aggregation's fused store — the input stage
 * of the trunk backward (cb_trunk_input_bwd_multi_f32, act_bits) then reads 32 bytes per row instead of C's 1 KiB. */
int cb_gemm_nn_indrop_supported(const float* A, int64_t lda, const float* B, int64_t ldb, const float* C, int64_t ldc, const float* C2, int64_t ldc2,
                                int64_t M, int64_t N, int64_t K);
int cb_gemm_nn_indrop_drop2_f32(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, float* C2, int64_t ldc2,
                                int64_t M, int64_t N, int64_t K, const float* bias, int relu, float a_drop_p, uint64_t a_seed, float drop_p,
                                uint64_t seed, const uint64_t* seed_dev, int64_t row0, uint64_t* relu_bits, void* stream);
/* Single-output forms of the same (no dropped copy of the OUTPUT either): the input Linear writes X0 (+ its mask words) only, and the first
 * GCNConv's transform applies the dropout in front of layer 0 (GCN.py:110) to X0 while IT stages it; its weight gradient regenerates that mask:
 *     C = act(rowscale * (dropout(A) @ B) + addend + bias)             cb_gemm_nn_indrop_f32   (cb_gemm_nn_indrop_supported with C2 = C)
 *     C = dropout(A)^T @ (rowscale * G)                                cb_gemm_tn_adrop_f32    (cb_gemm_tn_adrop_supported)
 * X0's dropped copy (10 GB at the headline size) is then never written, kept or read.  Bit-identical to the forms with the copy. */
int cb_gemm_nn_indrop_f32(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                          const float* rowscale, const float* addend, int64_t ld_add, const float* bias, int relu, float a_drop_p, uint64_t a_seed,
                          const uint64_t* seed_dev, int64_t row0, uint64_t* relu_bits, void* stream);
int cb_gemm_tn_adrop_supported(const float* A, int64_t lda, const float* G, int64_t ldg, int64_t K1, int64_t K2);
int cb_gemm_tn_adrop_f32(const float* A, int64_t lda, const float* G, int64_t ldg, const float* rowscale, float* C, int64_t M, int64_t K1, int64_t K2,
                         float a_drop_p, uint64_t a_seed, const uint64_t* seed_dev, int64_t row0, void* ws, size_t ws_bytes, void* stream);
int cb_gemm_tn_gdrop_supported(const float* A, int64_t lda, const float* G, int64_t ldg, int64_t K1, int64_t K2);
int cb_gemm_tn_gdrop_f32(const float* A, int64_t lda, const float* G, int64_t ldg, float* C, int64_t M, int64_t K1, int64_t K2, float g_drop_p,
                         uint64_t g_seed, const uint64_t* seed_dev, int64_t row0, void* ws, size_t ws_bytes, void* stream);
/* The input stage of the fused trunk's backward INSIDE the input Linear's weight gradient (round 6; autograd of GCN.py:104-110 — F.dropout(x),
 * layers_MLP[0], F.relu, F.dropout — and of the mixes res_tricks.py:23):
 *     gy = (X0 > 0) * ( dropout_bwd_{g_seed}(g) + mfold )          [M, 256], computed while it is staged as the A operand: never written, never re-read
 *     C  = gy^T @ dropout_{x_seed}(X)                               [256, K2] = layers_MLP[0].weight.grad
 *     colsum = column sums of gy                                    [256]     = layers_MLP[0].bias.grad
 * g = dL/d dropout(X0) (the dX of the first GCNConv), mfold = the folded mix gradients (cb_spmm_csr_store_bwd_mix_f32), x0_bits = [M][4] mask words of
 * (X0 > 0) (cb_gemm_nn_indrop_*'s relu_bits), X = the undropped features.  Replaces cb_trunk_input_bwd_multi_f32 + cb_gemm_tn_gdrop_f32 (2 * 4 * 256 * M bytes
 * less traffic).  64 < K2 <= 128, K2 % 4 == 0, both dropouts active, >= 256 row slabs: cb_gemm_tn_instage_supported first. */
int cb_gemm_tn_instage_supported(const float* g, const float* mfold, const float* X, int64_t ldx, int64_t M, int64_t K2);
size_t cb_gemm_tn_instage_workspace_bytes(int64_t M, int64_t K2);
int cb_gemm_tn_instage_f32(const float* g, const float* mfold, const uint64_t* x0_bits, const float* X, int64_t ldx, float* C, float* colsum, int64_t M, int64_t K2,
                           float g_drop_p, uint64_t g_seed, float x_drop_p, uint64_t x_seed, const uint64_t* seed_dev, int64_t row0, void* ws, size_t ws_bytes,
                           void* stream);

/* The sum-first GCNConv + store of the rows-only training forward in one persistent kernel (replaces GCN.py:213-256 with the sum taken first,
 * then :127-133 on a subset of the node rows: cb_spmm_csr_f32 with col_scale followed by cb_gemm_nn_store_rows_f32 — the same values bit for bit):
 *     out   = H[v] = sum_{u in row v} col_scale[u] * h[u]                  [N, 256] (stored: the backward's source-side level reads it)
 *     act   = relu(g_rowscale[m] * (H @ B)[m] + bias)                      -> out_act [N, ld_act] if given
 *     g_out = dropout_{seed, node row}(c_act * act + c_mix * mix_src[mix_index[m] | row_ids[m]])
 *     relu_bits[row_ids[m]][0..3] = the mask words of act > 0 (AND kept by the dropout unless bits_relu_only), as cb_gemm_nn_store_rows_f32
 * store: cb_trunk_store (relu_bits 16-byte aligned here: the words leave as 16-byte vectors).  row_ids (int64 [N]): the node row of each CSR row; the
 * dropout mask is drawn at (row0 + row_ids[m]).  d must be 256, fp32 rows, 16-byte aligned;
 * image: cb_agg_gemm_image_f32 of W.  A tile hand-over that times out is recorded in the device error word (cb_device_status). */
int cb_spmm_gemm_store_rows_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* col_scale, float* out, int64_t ld_out,
                                const void* image, const float* g_rowscale, const float* bias, const int64_t* row_ids, const cb_trunk_store* store,
                                float* g_out, int64_t ld_gout, void* stream);

/* One label-propagation step, elementwise passes folded into the aggregation's store (Label_propagation_model/outcome_correlation.py:137-143
 * with alpha_term and post_step = clamp(0, 1), as trainer_node_classification.py:33-63 drives it):
 *     out[v, :] = post_scale[v] * clamp(row_scale[v] * sum_{u in row v} h[u, :] + c_mix * mix[v, :], 0, 1)      (post_scale NULL: 1) */
int cb_spmm_csr_lp_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale, const float* mix, int64_t ld_mix,
                       float c_mix, const float* post_scale, float* out, int64_t ld_out, void* stream);

/* One propagation step of general_outcome_correlation (Label_propagation_model/outcome_correlation.py:128-145) for every normalised adjacency and
 * post-step of Correct & Smooth, next to cb_spmm_csr_lp_f32 (same kernels, same hub plan; lo = 0, hi = 1, fix_rows = NULL is that entry bit for bit):
 *     out[v, :] = post_scale[v] * fix_v(clamp(row_scale[v] * sum_{u in row v} h[u, :] + c_mix * mix[v, :], lo, hi))      (post_scale NULL: 1)
 * lo = -INFINITY and hi = +INFINITY: no clamp.  fix_rows (uint8 [N], one byte per row, or NULL): where the byte is non-zero the row is replaced by
 * mix[v, :] (fix_inputs, :194-199, whose fixed values ARE the mix rows).  With A_norm = diag(R) A diag(S) — DAD: R = S = D^-1/2; DA: R = D^-1, S = 1;
 * AD: R = 1, S = D^-1 (:51-55) — and the state s_t = S (.) result_t as h: row_scale = alpha R, c_mix = 1 - alpha (alpha_term) or 1, post_scale = S
 * (NULL on the last step, which returns result itself).  The CSR is by destination; the graph is symmetric (to_undirected, :41). */
int cb_spmm_csr_prop_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale, const float* mix, int64_t ld_mix,
                         float c_mix, float lo, float hi, const uint8_t* fix_rows, const float* post_scale, float* out, int64_t ld_out,
                         void* stream);

/* Row passes of Correct & Smooth (csrc/cb_cs.hip).  label_rows: uint8 [N], non-zero = label row (the layout of fix_rows above); labels: int64 [N];
 * Cp >= C: the row width of the matrices the aggregation reads (padding columns are written as 0).  Workspace of the first: cb_cs_workspace_bytes.
 *
 * cb_cs_residual_init_f32 — pre_residual_correlation (:95-110): E0 [N, Cp] = onehot(labels) - P on the label rows, 0 elsewhere;
 *   state [N, Cp] (may be NULL) = state_scale (.) E0 (state_scale NULL: 1); abs_sum[0] (device) = sum |E0| — two stages, fixed order, no atomics. */
size_t cb_cs_workspace_bytes(int64_t N, int64_t Cp);
int cb_cs_residual_init_f32(const float* P, int64_t ld_p, const int64_t* labels, const uint8_t* label_rows, int64_t N, int64_t C, int64_t Cp,
                            const float* state_scale, float* E0, float* state, float* abs_sum, void* ws, size_t ws_bytes, void* stream);
/* cb_cs_correct_snap_f32 — the "correct" combine and pre_outcome_correlation (:112-126) in one pass:
 *   mode 0 (autoscale, :170-176): scale[v] = (abs_sum[0] / n_label) / sum_j |resid[v, j]|, inf -> 1, then > 1000 -> 1; res = P + scale * resid, NaN -> P
 *   mode 1 (fixed, :200):         res = P + scale * resid                    mode 2 (only, :209): res = P (resid unused)
 *   res_result [N, ld_res] = res; y2 [N, Cp] = res with the label rows set to onehot(labels); state [N, Cp] (may be NULL) = state_scale (.) y2.
 * abs_sum is read on the device (what cb_cs_residual_init_f32 left there): no host synchronisation between the two. */
int cb_cs_correct_snap_f32(int32_t mode, const float* P, int64_t ld_p, const float* resid, int64_t ld_r, const int64_t* labels,
                           const uint8_t* label_rows, int64_t N, int64_t C, int64_t Cp, const float* abs_sum, int64_t n_label, float scale,
                           const float* state_scale, float* res_result, int64_t ld_res, float* y2, float* state, void* stream);

/* The same pack with the rows narrowed to bf16 (round-to-nearest-even) as they are written: the send buffer of the bf16 halo wire. */
int cb_gather_rows_bf16_f32(const float* src, int64_t ld, const int64_t* idx, int64_t n_idx, int64_t d, uint16_t* out, void* stream);
/* out[r, :] = pos[r] >= 0 ? src[pos[r], :] : fill for r < n_rows (contiguous [n, d] src and [n_rows, d] out, d % 4 == 0): a matrix over a
 * row subset written back to all rows in one pass — fill = 0: the gradient of a structural-embedding table (dL/dZ_l, GCN.py:230-232) when the level
 * of the row-sparse backward that produces it is compact; fill = NaN: the logits (GCN.py:138) of a rows-only training forward, evaluated on the loss
 * rows of trainer_node_classification.py:390-391 only — a reader of any other row gets NaN, not a plausible number (trunk.py). */
int cb_expand_rows_f32(const float* src, const int32_t* pos, int64_t n_rows, int64_t d, float fill, float* out, void* stream);
/* The trunk's store (cb_trunk_store) on a SUBSET of the rows, applied to the output of a dense transform instead of inside an aggregation: y / out
 * (and out_act) are compact [n_rows, .] matrices of the rows row_index[0 .. n_rows) (ascending global ids), relu_bits is the full array, the dropout
 * mask is drawn at the global row; mix_src is read at row mix_index[r] (mix_index NULL: at row_index[r], i.e. mix_src is a full array too).
 *   act = relu(y[r]) (-> out_act[r]);  out[r] = dropout((c_act * act + c_mix * mix_src[mix_index[r]]));  bits as cb_spmm_csr_fused_f32 writes them.
 * The rows-only forward of the training step (trunk.py): the last GCNConv (GCN.py:205-256) evaluated on the loss rows of trainer…:390-391. */
int cb_trunk_store_rows_f32(const float* y, const int64_t* row_index, int64_t n_rows, int64_t d, const cb_trunk_store* store, float* out, void* stream);
/* The same store as the EPILOGUE of the dense transform in front of it:
 *   act = relu(rowscale * (A @ B) + addend + bias) (-> out_act if given);  C = dropout(c_act * act + c_mix * mix_src[mix_index[m] | row_index[m]])
 * with A, C, out_act, rowscale, addend compact over the rows row_index[0 .. M) — a GCNConv evaluated sum-first on a subset of the rows (GCN.py:213-256
 * with the aggregation taken before the transform) and the trunk's ReLU / mix / dropout (:127-133) in one kernel.  N == 256; results equal
 * cb_gemm_nn_f32 followed by cb_trunk_store_rows_f32 bit for bit.  cb_gemm_nn_store_rows_supported tells whether the fused form exists for a shape. */
int cb_gemm_nn_store_rows_supported(const float* A, int64_t lda, const float* B, int64_t ldb, const float* C, int64_t ldc, int64_t M, int64_t N, int64_t K);
int cb_gemm_nn_store_rows_f32(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                              const float* rowscale, const float* addend, int64_t ld_add, const float* bias, const int64_t* row_index,
                              const cb_trunk_store* store, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------
 * Student MLPs (MLP_model/__init__.py:1-156; cb_mlp.hip).  HBM-bound row kernels and losses; the Linear layers are cb_gemm_*.
 * ---------------------------------------------------------------------------------- */

/* The [LayerNorm, GELU, Dropout] tail of one getMLP group (utils.py:898-903: `nn.LayerNorm(d), nn.GELU(), nn.Dropout(p)`) in one pass over
 * z [rows, d] contiguous (the Linear's output, bias added by the GEMM epilogue):
 *     mean / rstd per row (biased variance, rstd = 1 / sqrt(var + eps));  u = gamma * (z - mean) * rstd + beta;
 *     out = keep(seed, r * d + c) / (1 - p) * 0.5 u (1 + erf(u / sqrt 2))          (exact GELU, nn.GELU()'s default)
 * keep() is cb_dropout_f32's draw for (seed, seed_dev, flat index r * d + c): no mask is stored; p == 0 (also: eval mode) draws nothing.
 * stats (may be NULL; 8-byte aligned) receives {mean, rstd} per row for the backward.  1 <= d <= 512; d == 256 with 16-byte aligned
 * pointers is the unmasked fast path, d % 4 == 0 with aligned pointers uses 16-byte accesses, anything else scalar ones.
 * Traffic: 8 d + 8 bytes per row + 8 d bytes of parameters. */
int cb_ln_gelu_drop_fwd_f32(const float* z, int64_t rows, int64_t d, const float* gamma, const float* beta, float eps, float p,
                            uint64_t seed, const uint64_t* seed_dev, float* out, float* stats, void* stream);
/* Its backward (autograd of the three modules) in one pass: recomputes x_hat, u and the keep mask from z, stats and the seed and writes
 *     dz = rstd * (dx_hat - mean_c(dx_hat) - x_hat * mean_c(dx_hat * x_hat)),  dx_hat = gamma * keep / (1 - p) * gelu'(u) * dy;
 *     dgamma[c] = sum_r du * x_hat,  dbeta[c] = sum_r du,  dbias[c] = sum_r dz[r, c]  (the bias gradient of the Linear in front).
 * Any of the three may be NULL.  The column sums leave as one partial row per wavefront in ws (cb_ln_gelu_drop_bwd_workspace_bytes) and are
 * summed in a fixed order: no atomics, two calls give the same bits.  Traffic: 12 d + 8 bytes per row. */
size_t cb_ln_gelu_drop_bwd_workspace_bytes(int64_t rows, int64_t d);
int cb_ln_gelu_drop_bwd_f32(const float* dy, const float* z, const float* stats, int64_t rows, int64_t d, const float* gamma,
                            const float* beta, float p, uint64_t seed, const uint64_t* seed_dev, float* dz, float* dgamma,
                            float* dbeta, float* dbias, void* ws, size_t ws_bytes, void* stream);

/* `nn.MSELoss()(part1_out, lrn_targ[batch_idx])` (trainer_node_classification.py:96,108) without materialising the gathered targets:
 *     loss[0] = mean_{b, c} (pred[b, c] - target[row_index[b], c])^2;   grad[b, c] = 2 (pred - target) / (B D)   (grad may be NULL).
 * pred / grad [B, D] contiguous, target [n_target_rows, ld_t]; row_index int64 (NULL: row b).  A row index outside [0, n_target_rows) is
 * never dereferenced; the loss is then NaN.  Fixed-order reduction (ws: cb_reduce_workspace_bytes()). */
int cb_mse_rows_f32(const float* pred, int64_t B, int64_t D, const float* target, int64_t ld_t, int64_t n_target_rows,
                    const int64_t* row_index, float* loss, float* grad, void* ws, size_t ws_bytes, void* stream);

/* Input of SEMLP's part 2 (MLP_model/__init__.py:102-108): out [B, F + 2 D] = [ x | alphas[1] * replaced | alphas[0] * part1_out ] with
 * x [B, F], replaced / part1_out [B, D] contiguous and alphas a DEVICE pointer to the two learnable scales.  A block whose source pointer
 * is NULL is not written: the reference's replacement() reads alphas[0] * part1_out (:103-104), so the caller fills x and that block first,
 * hands out[:, F+D:] to cb_topk_replace_f32 as the queries, and fills the middle block with a second call.  The backward of the
 * only differentiable inputs (x, replaced and part1_out are detached in the reference), in one launch + a one-wavefront finish:
 *     dalphas[0] = <g[:, F+D:], part1_out>,  dalphas[1] = <g[:, F:F+D], replaced>      (ws: 2 * cb_reduce_workspace_bytes()). */
int cb_part2_assemble_f32(const float* x, int64_t F, const float* replaced, const float* part1_out, int64_t D, const float* alphas,
                          int64_t B, float* out, void* stream);
int cb_part2_assemble_bwd_f32(const float* g, int64_t F, const float* replaced, const float* part1_out, int64_t D, int64_t B,
                              float* dalphas, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------
 * GraphMLP's neighbour-contrastive loss (MLP_model/__init__.py:158-208; cb_ncloss.hip).  MFMA-bound Gram sweeps of the batch embeddings
 * with themselves plus walks over the sparse adjacency power; no B x B matrix in the forward, a slab of one in the backward.
 *     cos_ij = <z_i, z_j> * (rinv_i * rinv_j),  s_ij = exp(cos_ij / tau),  a = crop(adj_pow, batch_idx)      (:190-208, utils.py:1250-1276)
 *     den_i = sum_{j != i} s_ij,  num_i = sum_{j != i} a_ij s_ij,  loss = -(1 / M) sum_{num_i != 0} log(num_i / den_i),  M = #{num_i != 0}
 * The power arrives as CSR (int32 rowptr [n + 1] / col, fp32 val, columns ascending) and, for the backward, also as the CSR of its transpose.
 * The sweeps evaluate s in fp32; the sparse walks (few pairs, but long sequential sums) work in float64 and round once per output element.
 * No float atomics anywhere: every sum has a fixed order and two calls give the same bits.
 * ---------------------------------------------------------------------------------- */

/* pos [n]: the largest i with batch_idx[i] == node, else -1 (integer atomicMax: deterministic); rep [B]: pos[batch_idx[i]] == i.  Restates what
 * `n_idx[subset] = torch.arange(...)` (utils.py:1261) leaves on the CPU for a batch drawn with replacement: the last occurrence represents the
 * node, every other occurrence has an empty row and column in the cropped matrix.  An id outside [0, n) is never used as an index (rep = 0). */
int cb_ncloss_positions_i64(const int64_t* batch_idx, int64_t B, int64_t n, int32_t* pos, int32_t* rep, void* stream);

/* nrm[r] = |x_r|_2 and rinv[r] = 1 / |x_r|_2 of x [rows, D] (either may be NULL); a zero row gives rinv = inf, as `x_sum ** (-1)` (:207) does. */
int cb_ncloss_row_norms_f32(const float* x, int64_t ldx, int64_t rows, int64_t D, float* nrm, float* rinv, void* stream);

/* `cosine_sim` (:200-208) after the GEMM: s [N, N] = x @ x^T on entry, s_ij * (1 / (nrm_i * nrm_j)) on return.  N < 65536. */
int cb_cosine_scale_f32(float* s, int64_t ld, int64_t N, const float* nrm, void* stream);

/* 1 if the sweeps over z take the exact three-limb bf16-MFMA core (16-byte aligned rows, D % 4 == 0, CB_GEMM_PLAIN_F32 unset), 0 for the
 * fp32-input MFMA core: the dispatch of cb_topk_replace_f32. */
int cb_ncloss_uses_limb_core(const float* z, int64_t ldz, int64_t D);

/* Forward.  z [B, D] (ldz), tau > 0; pos / rep from cb_ncloss_positions_i64; max_splits caps the number of column slabs a row block's sweep
 * is split into (0: the rule of cb_topk_replace_f32, about four blocks per CU).  Writes rinv / num / den / w / u [B], loss [1], m_count [1]:
 *     w_i = [num_i != 0] / (M tau den_i),  u_i = [num_i != 0] / (M tau num_i)      (the backward's row weights)
 * M == 0 gives loss = NaN (the reference's mean of an empty tensor).  Four launches (row norms, sweep with the row-sum epilogue into
 * per-slab partial sums in ws, one wavefront per batch row over the power's rows, a one-block finish); no host synchronisation.
 * Traffic: the sweep reads z once per 128-row block and slab; 2 B^2 D flop.  ws: cb_ncloss_workspace_bytes(B, max_splits). */
size_t cb_ncloss_workspace_bytes(int64_t B, int32_t max_splits);
int cb_ncloss_fwd_f32(const float* z, int64_t ldz, int64_t B, int64_t D, float tau, const int32_t* rowptr, const int32_t* col,
                      const float* val, int64_t n, const int64_t* batch_idx, const int32_t* pos, const int32_t* rep, int32_t max_splits,
                      float* rinv, float* num, float* den, float* w, float* u, float* loss, int32_t* m_count, void* ws, size_t ws_bytes,
                      void* stream);

/* Backward (autograd of :190-208), with zh_i = z_i * rinv_i:
 *     dzh_i = sum_{j != i} s_ij (w_i + w_j) zh_j - sum_j a_ij s_ij u_i zh_j - sum_j a_ji s_ji u_j zh_j
 *     dz_i  = g * (dzh_i - <dzh_i, zh_i> zh_i) * rinv_i                                        (g: DEVICE pointer to the upstream scalar)
 * cb_ncloss_normalize_rows_f32 writes zh [B, D] contiguous.  cb_ncloss_bwd_slab_f32 writes P [rows, ldp] = s_ij (w_i + w_j), 0 on the
 * diagonal, for the batch rows row0 .. row0 + rows (row0 a multiple of 128) and all B columns: the caller multiplies it by zh with
 * cb_gemm_nn_f32 into rows row0.. of dzh.  cb_ncloss_bwd_finish_f32 then subtracts the two sparse terms from dzh in place (one wavefront
 * per batch row over the CSR row and the CSR row of the transpose; every row is written by its owner only) and writes dz [B, D]. */
int cb_ncloss_normalize_rows_f32(const float* z, int64_t ldz, int64_t B, int64_t D, const float* rinv, float* zhat, void* stream);
int cb_ncloss_bwd_slab_f32(const float* z, int64_t ldz, int64_t B, int64_t D, float tau, const float* rinv, const float* w, int64_t row0,
                           int64_t rows, int32_t max_splits, float* P, int64_t ldp, void* stream);
int cb_ncloss_bwd_finish_f32(const float* z, int64_t ldz, const float* zhat, int64_t B, int64_t D, float tau, const float* rinv, const float* u,
                             const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* rowptr_t, const int32_t* col_t,
                             const float* val_t, int64_t n, const int64_t* batch_idx, const int32_t* pos, const int32_t* rep, const float* g,
                             float* dzh, float* dz, void* stream);

/* ----------------------------------------------------------------------------------
 * fp32 sparse x sparse product C = A B and the exact transpose of a CSR matrix (cb_spgemm.hip): GraphMLP's adjacency power A~^r
 * (utils.py:1242-1248) without the host.  A is m x k, B is k x n_cols, both int32 CSR (rowptr / col) with fp32 values; C comes back as int32
 * CSR with ascending columns.  Contract:
 *   - C[i, j] is the sequential fp32 sum of its products A[i, k] * B[k, j] in the order of A's entries in row i (ascending k for a coalesced
 *     A); each product is rounded to fp32 on its own and the first addend is the first product.  No float atomics; two calls give the same
 *     bits and the result does not depend on the chunking.
 *   - an entry exists where at least one product exists, also where the sum is 0.0 (torch.sparse.mm + coalesce).
 *   - indices are int32, product counts and offsets int64; nnz(C) >= 2^31 is CB_E_RANGE, found from the running count of the chunks.
 * The caller walks the rows in chunks (a maximal run of consecutive rows whose products fit a budget, at least one row) so that the
 * workspace follows the budget, not the graph: about 24 B per product of the largest chunk.  Per chunk one host read of *count.
 * ---------------------------------------------------------------------------------- */

/* ent_off [nnz_a + 1] (int64): ent_off[e] = sum over A's entries e' < e of the length of B's row col_a[e']; ent_off[nnz_a] = all products.
 * The products of rows [r0, r1) of A are ent_off[rowptr_a[r1]] - ent_off[rowptr_a[r0]].  n_bad [1]: entries of A whose column lies outside
 * [0, k) or whose row of B has a negative length; they count no products. */
size_t cb_spgemm_offsets_workspace_bytes(int64_t nnz_a);
int cb_spgemm_entry_offsets_i64(const int32_t* col_a, int64_t nnz_a, const int32_t* rowptr_b, int64_t k, int64_t* ent_off, int32_t* n_bad,
                                void* ws, size_t ws_bytes, void* stream);

/* Rows [row0, row1) of A times B, first half: expands the chunk's n_products products (n_products must be the difference of ent_off
 * above; < 2^31) into ws, sorts them by (row, col) and writes the number of distinct (row, col) to *count (DEVICE int64).  The bits of
 * n_products, row1 - row0 and n_cols must fit 64 together (CB_E_RANGE otherwise: fewer rows per chunk).  ws:
 * cb_spgemm_chunk_workspace_bytes(n_products); it carries the chunk to cb_spgemm_chunk_emit_f32 and must not be touched in between. */
size_t cb_spgemm_chunk_workspace_bytes(int64_t n_products);
int cb_spgemm_chunk_count_f32(const int32_t* rowptr_a, const int32_t* col_a, const float* val_a, const int32_t* rowptr_b, const int32_t* col_b,
                              const float* val_b, const int64_t* ent_off, int64_t row0, int64_t row1, int64_t k, int64_t n_cols,
                              int64_t n_products, int64_t* count, void* ws, size_t ws_bytes, void* stream);

/* Second half, with `count` read back by the host: col_out / val_out [count] = the chunk's entries (rows ascending, columns ascending inside
 * a row) and rowptr[row0 .. row1) = nnz_base + the entries of the chunk before each row (rowptr: C's whole [m + 1] array; the caller writes
 * rowptr[m]).  nnz_base = entries of the chunks before this one; nnz_base + count >= 2^31 is CB_E_RANGE.  A chunk without products
 * (n_products == 0, count == 0) needs no ws. */
int cb_spgemm_chunk_emit_f32(const void* ws, size_t ws_bytes, int64_t row0, int64_t row1, int64_t n_cols, int64_t n_products, int64_t count,
                             int64_t nnz_base, int32_t* rowptr, int32_t* col_out, float* val_out, void* stream);

/* The transpose of an m x n CSR matrix with nnz entries: rowptr_t [n + 1], col_t / val_t [nnz], columns (the matrix's rows) ascending.  The
 * values are moved, not recomputed: val_t is a permutation of val.  One radix sort over the column bits; ws 16 B per entry + the sort's. */
size_t cb_csr_transpose_workspace_bytes(int64_t nnz);
int cb_csr_transpose_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t m, int64_t n, int64_t nnz, int32_t* rowptr_t,
                         int32_t* col_t, float* val_t, void* ws, size_t ws_bytes, void* stream);

/* The library's radix sort on its own (tests; csrc/cb_sort.h — the sort behind the CSR ingest, the symmetrisation, the product sort and the
 * transpose above, csrc/cb_pair_core.h, cb_lpx.hip and cb_heur.hip): keys_out [n] = keys_in sorted ascending by
 * bits [0, end_bit), stable — keys equal on those bits keep their input order — and the bits at and above end_bit are moved with the key and
 * never compared: a payload there rides along.  keys_in is the second buffer of the passes and is destroyed.  ws:
 * cb_sort_u64_workspace_bytes(n).  CB_E_RANGE for n < 0, n >= 2^32, end_bit <= 0 or end_bit > 64; n == 0 succeeds without pointers;
 * CB_E_WORKSPACE for a null buffer or short scratch.  No atomics: two calls give the same bits. */
size_t cb_sort_u64_workspace_bytes(int64_t n);
int cb_sort_u64(uint64_t* keys_in, uint64_t* keys_out, int64_t n, int end_bit, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------
 * The teacher's edge-wise (link-prediction) term (trainer_node_classification.py:417-438, 507-563; utils.py:754-791; cb_linkp.hip): positive and
 * negative edge samplers on the by-dst CSR (row v lists the sources u of the edges u -> v, columns ascending), the DistMult scores, the
 * binary cross-entropy with logits, the MRR and the gradient of the loss with respect to the embedding matrix.
 * The graph arrives as a cb_csr_view of which rowptr / col / n_rows / n_edges are read (square, plain column ids: col_flags == 0).
 * mask [N] uint8: the train mask.  mode 0 = train (a node is valid if mask != 0), mode 1 = test (valid if mask == 0).
 * Random draws: Philox4x32-10 (the generator of cb_dropout_f32, same fixed counter words 2 and 3), key = the 64-bit seed (+ *seed_dev when
 * seed_dev != NULL: the device seed word of a captured step), counter = the 64-bit draw number slot * CB_LINKP_MAX_TRIES + try.  With the four
 * output words r0..r3 a draw gives the integers hi64((r0 << 32 | r1) * n) and hi64((r2 << 32 | r3) * n) of [0, n).
 * No float atomics; no host synchronisation; two calls with the same inputs give the same bits.
 * ---------------------------------------------------------------------------------- */
#define CB_LINKP_MAX_TRIES 64
int cb_linkp_max_tries(void);

/* counts [N]: the number of entries of row v with a valid column if v is valid itself, else 0 (multiplicity and self loops counted as stored).
 * The caller scans it into prefix [N + 1] (int32, prefix[0] = 0, prefix[N] = n_valid); once per (graph, mask, mode), off the step. */
int cb_linkp_valid_counts_i32(const cb_csr_view* g, const uint8_t* mask, int32_t mode, int32_t* counts, void* stream);

/* out [2, P]: P draws, uniform with replacement over the n_valid valid edges (np.random.choice(n_valid, samp_size_p), :523); row 0 = source
 * (column id), row 1 = destination (CSR row).  One wavefront per draw (try 0 of its slot, first integer): binary search of prefix for the row,
 * then the row is walked 64 columns at a time.  n_valid > 0.  A prefix that does not belong to (g, mask, mode) gives (-1, -1), never a fault. */
int cb_linkp_positives_i32(const cb_csr_view* g, const uint8_t* mask, int32_t mode, const int32_t* prefix, int64_t n_valid, int64_t P,
                           uint64_t seed, const uint64_t* seed_dev, int32_t* out, void* stream);

/* out [2, Nn], Nn even: slot s < Nn / 2 writes (u, v) to column 2 s and (v, u) to column 2 s + 1 (`force_undirected=True`, :546).  mode 0: u and v
 * are train_nodes[first integer], train_nodes[second integer] (train_nodes [n_train]: the train nodes, ascending); mode 1: the two integers of
 * [0, N) themselves, rejected if both are train nodes.  Rejected in both modes: u == v, u in row v, v in row u.  A slot that finds no pair in
 * CB_LINKP_MAX_TRIES tries writes -1 to its four cells and adds 1 to *n_failed (int32, integer atomic; the caller zeroes and reads it). */
int cb_linkp_negatives_i32(const cb_csr_view* g, const uint8_t* mask, int32_t mode, const int32_t* train_nodes, int64_t n_train, int64_t Nn,
                           uint64_t seed, const uint64_t* seed_dev, int32_t* out, int32_t* n_failed, void* stream);

/* `linkp_loss_eva` (utils.py:759-774) on index pairs instead of gathered rows: emb [N, D] (ld >= D), pos [2, P], neg [2, Nn], P >= 1.
 *     scores [P + Nn]: <emb[h_e], emb[t_e]> in fp32 (one wavefront per edge; float4 loads when D % 4 == 0, ld % 4 == 0 and emb is 16-byte aligned)
 *     loss = mean_e max(s_e, 0) - s_e y_e + log1p(exp(-|s_e|)),  y = 1 for the P positives, 0 for the Nn negatives
 *     mrr  = mean_i 1 / rank_i,  rank_i = 1 + #{j in [i k, (i + 1) k): neg_j > pos_i},  k = Nn / P (k = 0: every rank is 1); ties count for the positive
 * loss and mrr are summed in float64 in one fixed order by one block and rounded once.  status [1]: the number of edges with an endpoint
 * outside [0, N) (a failed sampler slot holds -1): such an edge is never used as an index, its score is NaN and so are loss and mrr. */
int cb_linkp_loss_fwd_f32(const float* emb, int64_t ld, int64_t N, int64_t D, const int32_t* pos, int64_t P, const int32_t* neg, int64_t Nn,
                          float* scores, float* loss, float* mrr, int32_t* status, void* stream);

/* `cal_MRR` (utils.py:776-791) for callers that hold scores: the finishing kernel of cb_linkp_loss_fwd_f32 without the loss. */
int cb_linkp_mrr_f32(const float* pos_score, int64_t P, const float* neg_score, int64_t Nn, float* mrr, void* stream);

/* Backward: ds_e = g (sigmoid(s_e) - y_e) / (P + Nn) (g: DEVICE pointer to the upstream scalar); demb [N, D] (ldd >= D) =
 * sum_e ds_e (emb[t_e] into row h_e, emb[h_e] into row t_e); rows no sample touches are zero.  The 2 (P + Nn) contributions are sorted by
 * destination; one wavefront per distinct node adds its contributions in ascending contribution number (2 e for h_e, 2 e + 1 for t_e) in
 * float64 and writes the row once.  Edges with an endpoint outside [0, N) contribute nothing. */
size_t cb_linkp_bwd_workspace_bytes(int64_t P, int64_t Nn);
int cb_linkp_loss_bwd_f32(const float* emb, int64_t ld, int64_t N, int64_t D, const int32_t* pos, int64_t P, const int32_t* neg, int64_t Nn,
                          const float* scores, const float* g, float* demb, int64_t ldd, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------
 * The link-prediction baselines CN / AA (Link_prediction_baseline/heuristics.py:107-129 `CN`, `AA`; Link_prediction_model/layer.py:6-17
 * `Heuristics.get_score`; base_options.py:112 `--encoder CN | AA | PPR`) and the counts behind Hits@K / AUC
 * (Link_prediction_model/utils.py:43-59; Link_prediction_baseline/heuristics.py:51-62); cb_heur.hip.  The reference evaluates
 * `A[src].multiply(A_[dst])` with scipy on the host in batches of 100 000 pairs; on the CSR it is a sorted-row intersection.
 * A = csr_matrix((1, (ei[0], ei[1]))): A[s, k] = the multiplicity of the edge s -> k, row s = the OUT-row of s = row s of the by-src CSR
 * (rowptr_t / col_t of cb_csr_from_coo_i64; ascending columns, duplicates stored).  CN(s, d) = sum_k A[s, k] A[d, k];
 * AA(s, d) = sum_k A[s, k] A[d, k] w[k].  No special case for s == d, self loops, or (s, d) being an edge.
 * The views are read for rowptr / col / n_rows / n_edges only (square, plain column ids: col_flags == 0).
 * The float results involve no atomic; no host synchronisation; two calls with the same inputs give the same bits.
 * ---------------------------------------------------------------------------------- */
#define CB_HEUR_GROUP 16 /* lanes that share one pair in cb_heur_pair_scores_f32 (four pairs per wavefront) */

/* w [N] float64: 1 / log(in-degree), 0 where in-degree <= 1 (heuristics.py:119-120: `1 / np.log(A.sum(axis=0))`, the inf of a column sum
 * of 1 zeroed).  g_in: the by-dst view (rowptr read only): in-degree with multiplicity = rowptr[k + 1] - rowptr[k]. */
int cb_heur_aa_weights_f64(const cb_csr_view* g_in, double* w, void* stream);

/* score [P] fp32 (heuristics.py:113, 126).  g_out: the by-src view.  pairs int32 [2, P]: row 0 = s, row 1 = d.
 * w == NULL: CN, accumulated in int64, converted once (exact below 2^24).
 * w != NULL ([N] float64): the sum of the multiplicity products times w[k] in float64, rounded to fp32 once.
 * status [1] (zeroed by the call): the number of pairs with an endpoint outside [0, N).  Such a pair is never used as an index; its score
 * is NaN (one integer atomic per such pair, order-independent).  P == 0 launches nothing. */
int cb_heur_pair_scores_f32(const cb_csr_view* g_out, const double* w, const int32_t* pairs, int64_t P, float* score, int32_t* status,
                            void* stream);
/* The same with the group width chosen by the caller: group = 16 or 64 lanes per pair.  CN does not depend on it; the weighted sum is taken
 * in another order (float64, rounded once).  For measuring the choice of CB_HEUR_GROUP and for testing that results do not hinge on it. */
int cb_heur_pair_scores_width_f32(const cb_csr_view* g_out, const double* w, const int32_t* pairs, int64_t P, int32_t group, float* score,
                                  int32_t* status, void* stream);

/* gt [P], eq [P] int32: gt[i] = #{j : neg[j] > pos[i]}, eq[i] = #{j : neg[j] == pos[i]} over ALL Nn negatives (Nn < 2^31, P < 2^31):
 * Hits@K = mean(gt + eq < K) and AUC = sum_i (Nn - gt_i - eq_i + eq_i / 2) / (P Nn) derive from them and are well defined under ties
 * (Link_prediction_model/utils.py:43-59).  The negatives are sorted once (order-preserving float -> uint32 key: -0.0 == +0.0, -inf first,
 * +inf last; cb_sort.hip on 32 bits), then two binary searches per positive.  status [1] (zeroed by the call): the number of NaNs in pos
 * and neg; if it is not 0, every gt / eq is -1 (a NaN never compares as a number).  Nn == 0 gives zeros and needs no workspace. */
size_t cb_rank_counts_workspace_bytes(int64_t P, int64_t Nn);
int cb_rank_counts_f32(const float* pos, int64_t P, const float* neg, int64_t Nn, int32_t* gt, int32_t* eq, int32_t* status, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------
 * The link-prediction experiment's samplers, epoch shuffle and ranking metrics (Link_prediction_model/negative_sample.py:5-57; model.py:121-266;
 * utils.py:568-586 `cal_recall`; Link_prediction_model/utils.py:61-91); cb_lpx.hip.  Draws are those of the samplers above: Philox4x32-10 under the
 * 64-bit seed, draw number d -> words r0..r3, the integers hi64((r0 << 32 | r1) * n) and hi64((r2 << 32 | r3) * n) of [0, n).
 * No float atomics; no host synchronisation; two calls with the same inputs give the same bits.
 * ---------------------------------------------------------------------------------- */
#define CB_LPX_MAX_TRIES 64
int cb_lpx_max_tries(void);

/* `global_neg_sample` (negative_sample.py:5-19).  g: the by-dst view (rowptr / col / n_rows / n_edges read; square, col_flags == 0, N >= 2).
 * out int32 [2, S].  Slot s, try t: (u, v) = the two integers of draw s * CB_LPX_MAX_TRIES + t in [0, N); accepted iff u != v and u is not a
 * column of row v (binary search; only the directed pair u -> v is tested, as `negative_sampling` does after `add_self_loops`).  The first accepted
 * try goes to out[0, s], out[1, s]; a slot without one holds -1 in both cells and adds 1 to *n_failed (int32, integer atomic; the caller zeroes
 * and reads it). */
int cb_lpx_neg_global_i32(const cb_csr_view* g, int64_t S, uint64_t seed, int32_t* out, int32_t* n_failed, void* stream);

/* `local_neg_sample`, random_src=False (negative_sample.py:28-40).  pos_src int32 [P]: the sources of the positives; out int32 [2, P k]:
 * out[0, s] = pos_src[s / k] as it stands, out[1, s] = the first integer of draw s * CB_LPX_MAX_TRIES in [0, N).  No rejection.  N >= 2. */
int cb_lpx_neg_local_i32(const int32_t* pos_src, int64_t P, int64_t k, int64_t N, uint64_t seed, int32_t* out, void* stream);

/* perm int32 [n]: perm[j] = the low 32 bits of the j-th smallest key (r0(draw i) << 32) | i, i in [0, n), sorted over all 64 bits (cb_sort.hip).
 * The keys are distinct: a pure function of (n, seed).  n < 2^31; n == 0 launches nothing. */
size_t cb_lpx_permutation_workspace_bytes(int64_t n);
int cb_lpx_permutation_i32(int64_t n, uint64_t seed, int32_t* perm, void* workspace, size_t workspace_bytes, void* stream);

/* cb_rank_counts_f32's contract per row: pos [P], neg [P, K] with row stride ld >= K (elements); gt[i] = #{j : neg[i, j] > pos[i]},
 * eq[i] = #{j : neg[i, j] == pos[i]}, int32.  -0.0 == +0.0, the infinities compare as numbers.  A NaN in pos[i] or in row i gives
 * gt[i] = eq[i] = -1; status [1] (zeroed by the call) counts the NaNs (integer atomic, on that path only).  16 lanes per row for K <= 64, one
 * wavefront per row above; float4 loads from the row's first 16-byte boundary, scalar head and tail. */
int cb_lpx_row_ranks_f32(const float* pos, int64_t P, const float* neg, int64_t ld, int64_t K, int32_t* gt, int32_t* eq, int32_t* status,
                         void* stream);

/* The integer numerator of `cal_recall` (utils.py:576-585).  M = the positives with score > 0 and all Nn negatives, ordered by descending score,
 * a positive before a negative among equal scores, -0.0 taken as +0.0; result [1] int64 = the number of positives among the first min(k, |M|).
 * P + Nn < 2^32.  status [1] (zeroed by the call) counts the NaNs of pos and neg; the result is then -1. */
size_t cb_lpx_recall_topk_workspace_bytes(int64_t P, int64_t Nn);
int cb_lpx_recall_topk_f32(const float* pos, int64_t P, const float* neg, int64_t Nn, int64_t k, int64_t* result, int32_t* status,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------
 * The decoder of the link-prediction experiment on index pairs (Link_prediction_model/layer.py:85-106 `MLPPredictor`, :182-191 `DotPredictor`;
 * loss.py:4-30; model.py:108-119, 152-158); cb_linkpred.hip.  h [N, K] fp32 (ld >= K): the encoder's embeddings; pairs int32 [2, S]: row 0 = u,
 * row 1 = v.  Where the reference gathers h[u] and h[v] into two [S, K] matrices and multiplies them, these entries read the rows in place.
 * A pair with an endpoint outside [0, N) (a failed sampler slot holds -1) is never used as an index; status [1] (zeroed by the call) counts such
 * pairs (one integer atomic each, on that path only).  No float atomics; no host synchronisation; two calls with the same inputs give the same bits.
 * ---------------------------------------------------------------------------------- */

/* C [S, Nout] = act((h[u] * h[v]) @ B + bias), B [K, Nout]; the A operand is formed while the three-limb NN kernel stages it.  Every product
 * h[u][k] * h[v][k] is rounded to fp32 once and then split, and the K loop, the epilogue and the tile order are those of cb_gemm_nn_f32
 * (tiles of 256 x 64 for Nout <= 64 and 128 x 128 otherwise; an output element's K order does not depend on the tile): C has the bits
 * cb_gemm_nn_f32 gives on the materialised product.  drop_p > 0: C2 = dropout_p(C) with the keep-mask of cb_dropout_f32(C, ..., seed, seed_dev,
 * offset = row0 * Nout), the bits cb_gemm_nn_drop2_f32 writes — from the GEMM's own epilogue when Nout > 64 and C, C2 allow float4 stores
 * (16-byte aligned, ldc % 4 == 0, ldc2 % 4 == 0), else from cb_dropout_f32 after it, which needs ldc == ldc2 == Nout (checked before anything
 * is launched); drop_p == 0: C2 is not read.  The whole row of an unusable pair is NaN in C and in C2, in either form.
 * Exists where the three-limb NN kernel does (cb_pair_gemm_nn_supported: K % 4 == 0, Nout % 4 == 0, ld % 4 == 0, ldb % 4 == 0, h and B 16-byte
 * aligned); elsewhere the caller composes the gather, the product and cb_gemm_nn_f32. */
int cb_pair_gemm_nn_supported(const float* h, int64_t ld, const float* B, int64_t ldb, int64_t Nout, int64_t K);
int cb_pair_gemm_nn_f32(const float* h, int64_t ld, int64_t N, const int32_t* pairs, int64_t S, const float* B, int64_t ldb, float* C, int64_t ldc,
                        float* C2, int64_t ldc2, int64_t Nout, int64_t K, const float* bias, int relu, float drop_p, uint64_t seed,
                        const uint64_t* seed_dev, int64_t row0, int32_t* status, void* stream);

/* scores [S]: <h[u_e], h[v_e]> in fp32 (one wavefront per pair, fixed-shape reduction; float4 loads when D % 4 == 0, ld % 4 == 0 and h is
 * 16-byte aligned).  NaN for an unusable pair. */
int cb_pair_dot_f32(const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* pairs, int64_t S, float* scores, int32_t* status, void* stream);

/* dh [N, D] (ldd >= D) = sum_e (c_e * h[v_e] into row u_e, c_e * h[u_e] into row v_e): the gradient of either predictor with respect to h.
 * ldcoef == 0: coef [S], a scalar per pair (the dot predictor's ds); ldcoef >= D: coef [S, ldcoef], a row per pair multiplied elementwise (the
 * MLP predictor's dX).  The 2 S contributions are sorted by destination; one wavefront per distinct node adds its contributions in ascending
 * contribution number (2 e for u_e, 2 e + 1 for v_e) in float64 and writes the row once; rows no pair touches are zero.  Unusable pairs
 * contribute nothing. */
size_t cb_pair_scatter_workspace_bytes(int64_t S);
int cb_pair_scatter_f32(const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* pairs, int64_t S, const float* coef, int64_t ldcoef,
                        float* dh, int64_t ldd, void* ws, size_t ws_bytes, void* stream);

/* The pairwise losses of Link_prediction_model/loss.py over pos [P] and neg [P * k] read as [P, k] (P >= 1, k >= 1):
 *     CB_RANK_AUC           sum_ij (1 - (pos_i - neg_ij))^2
 *     CB_RANK_ADAPTIVE_AUC  sum_ij weight_i (1 - (pos_i - neg_ij))^2                                    weight [P]
 *     CB_RANK_LOG_RANK      mean_ij -log(sigmoid(pos_i - neg_ij) + 1e-15)
 *     CB_RANK_CE            mean_i -log(sigmoid(pos_i) + 1e-15) + mean_ij -log(1 - sigmoid(neg_ij) + 1e-15)
 *     CB_RANK_INFO_NCE      mean_i -log(exp(pos_i) / (exp(pos_i) + sum_j exp(neg_ij)) + 1e-15)
 * Every term is evaluated in float64 from the fp32 scores by the formula as written (sigmoid(x) = 1 / (1 + exp(-x))), summed in float64 in one
 * fixed order (thread-strided partial sums, a halving tree per block, one over the at most 256 blocks) and rounded to fp32 once.  The reference
 * evaluates in fp32, where 1 - sigmoid(s) cancels and exp(s) overflows above s = 88; this is the float64 value.
 * Backward: g is a DEVICE pointer to the upstream scalar; dpos [P] and dneg [P * k], each element a float64 sum rounded once. */
#define CB_RANK_AUC 0
#define CB_RANK_ADAPTIVE_AUC 1
#define CB_RANK_LOG_RANK 2
#define CB_RANK_CE 3
#define CB_RANK_INFO_NCE 4
size_t cb_rank_loss_workspace_bytes(void);
int cb_rank_loss_fwd_f32(int32_t kind, const float* pos, int64_t P, const float* neg, int64_t k, const float* weight, float* loss, void* ws,
                         size_t ws_bytes, void* stream);
int cb_rank_loss_bwd_f32(int32_t kind, const float* pos, int64_t P, const float* neg, int64_t k, const float* weight, const float* g, float* dpos,
                         float* dneg, void* stream);

/* ----------------------------------------------------------------------------------
 * The device pieces of the predictors that take their endpoint rows one at a time (Link_prediction_model/layer.py:108-180 `MLPCatPredictor`,
 * `MLPDotPredictor`, `MLPBilPredictor`, :193-203 `BilinearPredictor`); cb_pairpred.hip.  h [N, D] fp32 (ld >= D).  An index outside [0, N) is never
 * used as an index; status [1] (zeroed by the call) counts the rows / pairs that hold one (one integer atomic each, on that path only).  No float
 * atomics; no host synchronisation; two calls with the same inputs give the same bits.
 * ---------------------------------------------------------------------------------- */

/* C [R, Nout] = act(A @ B + bias), B [nseg * D, Nout], A[r, s * D + k] = h[idx[s * R + r], k] for s < nseg (idx int32 [nseg, R], nseg 1 or 2): the
 * gather h[idx] or the concatenation [h[idx0] | h[idx1]], formed while the three-limb NN kernel stages it and never written.  K loop, epilogue and
 * tile order are those of cb_gemm_nn_f32: C has the bits cb_gemm_nn_f32 gives on the materialised A.  drop_p, seed, seed_dev, row0, C2: the dropped
 * copy exactly as cb_pair_gemm_nn_f32 has it (the bits of cb_gemm_nn_drop2_f32; the two-kernel form for Nout <= 64 or outputs without float4
 * alignment needs ldc == ldc2 == Nout).  A row with an unusable index is NaN in C and in C2 and counts once.
 * Exists (cb_rows_gemm_nn_supported) where cb_pair_gemm_nn_f32 does for K = nseg * D, with D % 4 == 0 for nseg == 1 and D % 16 == 0 for nseg == 2
 * (no K step of 16 straddles the seam); elsewhere the caller composes the gather and cb_gemm_nn_f32. */
int cb_rows_gemm_nn_supported(const float* h, int64_t ld, int64_t D, int32_t nseg, const float* B, int64_t ldb, int64_t Nout);
int cb_rows_gemm_nn_f32(const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* idx, int32_t nseg, int64_t R, const float* B, int64_t ldb,
                        float* C, int64_t ldc, float* C2, int64_t ldc2, int64_t Nout, const float* bias, int relu, float drop_p, uint64_t seed,
                        const uint64_t* seed_dev, int64_t row0, int32_t* status, void* stream);

/* scores [S]: s_e = sum_j (sum_k W[j, k] h[u_e, k]) h[v_e, j] for pairs int32 [2, S]; Wt [D, D] (ldw >= D) is W TRANSPOSED (Wt[k][j] = W[j][k], the
 * B operand of the rows GEMM over u).  The dot against row v_e is taken in the GEMM's epilogue: no [S, D] matrix is written.  A row's columns inside
 * a tile are reduced in one fixed order and the column blocks' partials (workspace [S, column blocks] floats) are added in ascending block order by
 * a finishing pass, so a pair's score does not depend on where in the batch it sits.  NaN and one count for an unusable pair.  Exists where
 * cb_rows_gemm_nn_supported(h, ld, D, 1, Wt, ldw, D) holds. */
int cb_rows_bilinear_supported(const float* h, int64_t ld, int64_t D, const float* Wt, int64_t ldw);
size_t cb_rows_bilinear_workspace_bytes(int64_t S, int64_t D);
int cb_rows_bilinear_f32(const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* pairs, int64_t S, const float* Wt, int64_t ldw, float* scores,
                         int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* dh [N, D] (ldd >= D) = sum_e (G0[e, :] into row u_e, G1[e, :] into row v_e): the backward of both gathers.  G0 [S, ld0] and G1 [S, ld1] have
 * leading dimensions of their own (the two halves of one [2 S, D] matrix or the two column halves of one [S, 2 D] matrix pass without a copy).
 * The machinery of cb_pair_scatter_f32 with a row contributed as it stands: sorted keys, float64 sums in ascending contribution number (2 e for
 * u_e, 2 e + 1 for v_e) rounded once, untouched rows zero, unusable pairs skipped.  Workspace: cb_pair_scatter_workspace_bytes(S). */
int cb_rows_scatter_f32(int64_t N, int64_t D, const int32_t* pairs, int64_t S, const float* G0, int64_t ld0, const float* G1, int64_t ld1, float* dh,
                             int64_t ldd, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------
 * One layer of the link-prediction encoders (Link_prediction_model/layer.py:8-35: SAGEConv with mean aggregation, GraphConv with add,
 * GCNConv(normalize=False)) in one launch; cb_sage.hip.  Widths 256 -> 256, fp32 rows, 16-byte aligned, ld >= 256 and a multiple of 4:
 *     agg[v, :] = row_scale[v] * sum_{j in row v} col_scale[col[j]] * h[col[j], :]            (row_scale / col_scale may be NULL)
 *     out[v, :] = epi([agg[v, :] | self[v, :]] @ B + bias)                                    (self == NULL: out = epi(agg @ B + bias), B 256 x 256)
 *     epi       = identity | ReLU (relu) | ReLU then dropout_p with the keep-mask of cb_dropout_f32 for (seed, seed_dev, flat index (row0 + v) * 256 + column)
 * The sums are cb_spmm_csr_f32's (rows reduced in CSR order by one wavefront, hub rows by its hub kernels before the layer kernel), the product is
 * cb_gemm_nn_f32's on the materialised [agg | self] with the stacked B (K = 512, its limb products and K order): the same bits as the two calls.
 * Forward: by-dst CSR, h = self = X, row_scale = 1 / indeg (SAGE) or NULL, B = [W_n^T ; W_s^T], agg_out NULL.
 * Backward: by-src CSR, h = self = G, col_scale = 1 / indeg (SAGE) or NULL, B = [W_n ; W_s], agg_out = R = A_s^T G (the weight gradient R^T X reads it).
 * agg_out [N, ld_agg] (may be NULL when the plan has no hub rows): receives agg; with agg_hubs_only != 0 only the hub rows are written (they reach
 * the kernel's tile through memory) and the rest of the buffer is left untouched.
 * image: B split once into bf16 limbs in MFMA fragment order by cb_sage_image_f32 — W_n [256, ld_n] and W_s [256, ld_s] (NULL: 256 x 256 image) as
 * B = [W_n ; W_s] (transpose = 0) or [W_n^T ; W_s^T] (transpose = 1); cb_sage_image_bytes(has_self) bytes, 16-byte aligned.
 * cb_sage_layer_supported: 1 where the kernel exists (d_in == d_out == 256, fp32, alignment as above), else 0 — the caller then composes
 * cb_spmm_csr_f32 and cb_gemm_nn_f32; an unsupported direct call returns CB_E_INVALID.  No atomics, no device error word, deterministic.
 * ---------------------------------------------------------------------------------- */
size_t cb_sage_image_bytes(int has_self);
int cb_sage_image_f32(const float* W_n, int64_t ld_n, const float* W_s, int64_t ld_s, int transpose, void* image, size_t image_bytes, void* stream);
int cb_sage_layer_supported(int64_t d_in, int64_t d_out, int32_t h_bf16, const void* h, int64_t ld_h, const float* self, int64_t ld_self,
                            const float* agg_out, int64_t ld_agg, const float* out, int64_t ld_out);
int cb_sage_layer_f32(const cb_csr_view* g, const float* h, int64_t ld_h, const float* self, int64_t ld_self, const float* col_scale,
                      const float* row_scale, const void* image, const float* bias, int relu, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                      int64_t row0, float* agg_out, int64_t ld_agg, int32_t agg_hubs_only, float* out, int64_t ld_out, void* stream);

/* ----------------------------------------------------------------------------------
 * The adjacency WITH VALUES of the link-prediction encoders: one fp32 value w per stored edge, in the order of the view's col array (the by-dst CSR
 * for a forward, the by-src CSR for a backward; repeated edges stay separate entries).  Values are data: no entry here differentiates them
 * (cb_spmm_edge_dot_f32 above does that for the node-classification boundary).
 *   cb_spmm_csr_ew_f32   out[v] = sum_{j in row v} w_csr[j] * h[col[j]] on the tuned aggregation (cb_spmm_csr_f32's walk, hub plan, gather policy):
 *                        fp32 rows, d % 256 == 0, 16-byte aligned, ld % 4 == 0; acc += w * x edge by edge in fp32, a hub row's chunk partials merged in
 *                        chunk order.  Other widths: cb_spmm_csr_weighted_f32.
 *   cb_ewlayer_f32       cb_sage_layer_f32 with w_csr in place of col_scale / row_scale (GraphConv: self = h; GCNConv(normalize=False): self = null);
 *                        image, epilogue, agg_out and cb_sage_layer_supported as there.  Bit for bit cb_spmm_csr_ew_f32 + cb_gemm_nn_f32 on [agg | self].
 *   cb_adjnorm_rowsum_f64  deg[v] = fp32(float64 sum of row v's values, fixed order), fac[v] = fp32(1.0 / deg) (inv_sqrt = 0) or fp32(1.0 / sqrt(deg))
 *                        (inv_sqrt = 1), computed in float64 from the fp32 deg, an infinite result -> 0.  status (one int32 the caller zeroed) counts
 *                        the rows with a negative sum under inv_sqrt.
 *   cb_adjnorm_scale_f32 w_out[j] = (f[row of j] * w_csr[j]) * g[col[j]] (two fp32 roundings in this order); g null: f[row of j] * w_csr[j].  col may
 *                        carry hot-source flags.  D^-1 A: (f = 1 / deg, g = null); D^-1/2 A D^-1/2: f = g = deg^-1/2.
 * ---------------------------------------------------------------------------------- */
int cb_spmm_csr_ew_f32(const cb_csr_view* g, const float* w_csr, const float* h, int64_t ld_h, int64_t d, float* out, int64_t ld_out, void* stream);
int cb_ewlayer_f32(const cb_csr_view* g, const float* w_csr, const float* h, int64_t ld_h, const float* self, int64_t ld_self, const void* image,
                   const float* bias, int relu, float drop_p, uint64_t seed, const uint64_t* seed_dev, int64_t row0, float* agg_out, int64_t ld_agg,
                   int32_t agg_hubs_only, float* out, int64_t ld_out, void* stream);
int cb_adjnorm_rowsum_f64(const int32_t* rowptr, const float* w_csr, int64_t N, int64_t E, int32_t inv_sqrt, float* deg, float* fac, int32_t* status,
                          void* stream);
int cb_adjnorm_scale_f32(const int32_t* rowptr, const int32_t* col, const float* w_csr, int64_t N, int64_t E, const float* f, const float* g, float* w_out,
                         void* stream);

/* ----------------------------------------------------------------------------------
 * Attention over the rows of a CSR (PyG TransformerConv with heads = 1, no edge features, no beta: Link_prediction_model/layer.py:77-83);
 * cb_attn.hip.  Q, K, V, S, dO and every result are fp32 rows of D elements with a leading dimension each (column slices of one [N, 4 D]
 * matrix): D % 4 == 0, D <= 512, 16-byte aligned, ld % 4 == 0, ld >= D — cb_attn_supported(D, rows, ld) answers per operand before any
 * launch; an unsupported call returns CB_E_INVALID.  For an in-edge j = (u_j -> v) of the by-dst view, s_j = <Q[v], K[u_j]> / sqrt(D):
 *     fwd:      a_j = softmax_j(s_j) (the row's maximum subtracted; each copy of a duplicate edge is its own term),
 *               out[v] = act(sum_j a_j V[u_j] + S[v]),  lse[v] = max_j s + log sum_j exp(s_j - max_j s)   (lse may be NULL: not written)
 *               a row without in-edges: out[v] = act(S[v]), lse[v] = -inf
 *     bwd_dst:  a_j = exp(s_j - lse[v]);  delta[v] = sum_j a_j <dO[v], V[u_j]>;  dQ[v] = 1/sqrt(D) sum_j a_j (<dO[v], V[u_j]> - delta[v]) K[u_j]
 *     bwd_src:  on the by-src view, for the out-edges j = (u -> v) of u:  dK[u] = 1/sqrt(D) sum_j a_j (<dO[v], V[u]> - delta[v]) Q[v],
 *               dV[u] = sum_j a_j dO[v]        (lse and delta as bwd_dst left them; dS = dO needs no kernel)
 * No atomics, nothing of length E is written, every sum in CSR order: bit-reproducible.  Hub rows (a view with n_hubs > 0) are reduced in chunks
 * of hub_threshold edges, one wavefront per chunk, the partials — (max, sum, acc[D]) in the forward, plain sums of D (bwd_dst) and 2 D (bwd_src)
 * floats — combined in chunk order; all three entries need ws_bytes >= cb_attn_workspace_bytes(n_chunks, D) = n_chunks * (2 D + 4) floats
 * (CB_E_WORKSPACE otherwise), ws 16-byte aligned.  col_flags = 1 chooses the cache policy of the gathered rows only.
 * ---------------------------------------------------------------------------------- */
int cb_attn_supported(int64_t d, const void* rows, int64_t ld);
size_t cb_attn_workspace_bytes(int64_t n_chunks, int64_t d);
int cb_attn_fwd_f32(const cb_csr_view* g, int64_t d, const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v,
                    const float* skip, int64_t ld_s, int relu, float* out, int64_t ld_out, float* lse, void* stream);
int cb_attn_bwd_dst_f32(const cb_csr_view* g, int64_t d, const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v,
                        const float* dout, int64_t ld_do, const float* lse, float* dq, int64_t ld_dq, float* delta, void* stream);
int cb_attn_bwd_src_f32(const cb_csr_view* g_src, int64_t d, const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v,
                        const float* dout, int64_t ld_do, const float* lse, const float* delta, float* dk, int64_t ld_dk, float* dv, int64_t ld_dv,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COLDBREW_HIP_H */
