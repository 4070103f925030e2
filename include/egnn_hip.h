/*
 * egnn_hip.h -- C ABI of libegnn_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * GNN-distillation hot path of chaitjo/efficient-gnns.
 *
 * The reference has no FFI of its own: its hot path calls the PyG / torch-sparse / torch-scatter
 * Python operator API, whose native kernels live in un-vendored wheels.  Each entry
 * point below therefore cites the reference call site whose third-party kernel it replaces.  The
 * Python host side (efficient-gnns_amd/) binds these with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch's caching allocator); no entry
 *     point allocates, frees or synchronises, and none keeps state between calls: all are re-entrant.
 *     Two process-wide, write-once values exist: the GEMM pipeline choice read from the environment on
 *     first use (EGNN_GEMM_PIPE=f32 pins every product to the f32-input MFMA; default: the bf16-split
 *     pipeline, csrc/gemm_split.h) and the per-device "large dynamic LDS" opt-in of the kernels that need
 *     more than 64 KB (hipFuncSetAttribute, once per kernel and device).  No other environment variable
 *     is read by the library;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *   - dense matrices are row-major fp32 with an explicit leading dimension in ELEMENTS;
 *   - sparse structure is CSR; index arrays are int32 or int64, selected by `index_bits` (32|64).
 *     The exported structure is always int64 (torch-sparse convention); int32 is an internal
 *     narrowing the host performs when nnz and N fit;
 *   - return value: 0 on success, a negative EGNN_E* code otherwise (nothing enqueued on error,
 *     except EGNN_ELAUNCH which reports hipGetLastError() after a launch).
 */
#ifndef EGNN_HIP_H
#define EGNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGNN_OK 0
#define EGNN_EINVAL (-1)   /* bad argument (null pointer, negative size, unsupported enum) */
#define EGNN_ELAUNCH (-2)  /* the HIP runtime reported a launch error */
#define EGNN_EWORKSPACE (-3) /* caller-provided workspace too small */
#define EGNN_EALIGN (-4)   /* pointer / leading dimension not aligned as the entry point requires */

#define EGNN_ABI_VERSION 9
int egnn_abi_version(void);
const char* egnn_error_string(int code);
/* Number of distinct kernels-families compiled in; used by the loader's self check. */
int egnn_build_info(char* buf, size_t buf_bytes);

/* ------------------------------------------------------------------------------------------------
 * Neighbour aggregation: Y[i,:] = REDUCE_{e in row i} val[e] * src_scale[col[e]] * X[col[e],:]  (+ bias)
 *
 * Replaces torch_sparse::spmm (K1/K2 in SURVEY.md 2.2), reached from
 *   GCNConv.forward      /root/reference/arxiv_pyg/gnn.py:47,52   (reduce=sum, val = gcn_norm)
 *   SAGEConv.forward     /root/reference/arxiv_pyg/gnn.py:79,84   (reduce=mean, val = NULL)
 *   adj_t.matmul(mean)   /root/reference/mag_pyg/gnn.py:162
 *   loss.backward()      /root/reference/arxiv_pyg/gnn.py:192     (same kernel on the transposed CSR)
 *
 * The operands travel as ONE descriptor, egnn_spmm_t, shared by the three schedules below and the combine step.  A call
 * reads it only while it runs and never keeps the pointer (kernel arguments are copied at launch: the descriptor may live on
 * the caller's stack, also while a hipGraph is captured).  op == NULL is EGNN_EINVAL; an entry point checks only what it reads.
 *   val        [nnz]   nullable (= 1.0)
 *   src_scale  [n_src] nullable; per-source-row factor, used for the backward of mean (dX = A^T (dY / cnt)) without
 *                      materialising a per-entry value array
 *   bias       [K]     nullable; added to every written row (GCNConv `out += bias`, gnn.py:47); not with EGNN_MAX
 *   reduce             EGNN_SUM, EGNN_MEAN (sum / max(stored entries of the row, 1)), EGNN_MAX (egnn_spmm_csr_f32 and egnn_spmm_csr_max_piece_f32 only)
 * The epilogue is read by egnn_spmm_csr_blk_f32 and egnn_spmm_combine_f32 only.  The other two schedules have none: there addend,
 * stat_part or flags bit 3 set is EGNN_EINVAL (a fused add or ReLU is never silently dropped); the store hints are ignored.
 *   addend     nullable [n_rows, ld_addend] fp32: added to every stored row (Y = A X + addend): the sharded run aggregates
 *              its local and its halo columns in two calls, the second one accumulating onto the first
 *   stat_part  nullable [*, 2, K] fp32 partials of sum_r (y_r - shift) and sum_r (y_r - shift)^2 -- BatchNorm statistics in
 *              the aggregation epilogue (gnn.py:47-48), finished by egnn_bn_stats_merge_f32
 *   stat_shift nullable [K] (any vector near the column means, e.g. BatchNorm's running_mean; exactness does not depend on
 *              it, only the conditioning of the variance)
 *   flags      bit 1 (2): non-temporal Y stores; bit 2 (4): write-through (sc1) Y stores (tuning knobs, results are identical);
 *              bit 3 (8): Y = max(Y, 0) on the way out -- ReLU fused into the store (an eval-mode BatchNorm folded into the
 *              weights / bias by egnn_bn_fold_f32 + ReLU, gnn.py:47-49 under model.eval()); not together with stat_part
 * ---------------------------------------------------------------------------------------------- */
#define EGNN_SUM 0
#define EGNN_MEAN 1
#define EGNN_MAX 2

typedef struct egnn_spmm {
  int64_t n_rows; int64_t n_src; int64_t K;
  const void* rowptr; const void* col; int index_bits;      /* 32 | 64 */
  const float* val; const float* src_scale; const float* bias;
  const float* X; int64_t ldx;
  float* Y; int64_t ldy;
  int reduce;                                               /* EGNN_SUM | EGNN_MEAN | EGNN_MAX */
  const float* addend; int64_t ld_addend;                   /* epilogue: block schedule + combine only */
  float* stat_part; const float* stat_shift;
  int flags;
} egnn_spmm_t;

/* The ROW-CLASS schedule, and the only one that offers EGNN_MAX.
 *   argmax     [n_rows, K] int64, required for EGNN_MAX (index of the FIRST maximal stored entry in CSR order, -1 and 0.0
 *              for an empty row), ignored otherwise
 * Row schedule (built once per sparsity structure by the caller; integer preprocessing):
 *   short_rows [n_short]  row ids whose entry count is small; a wavefront walks 64/G of them at once (one
 *                         G-lane sub-group per row, G = lanes per 128-byte column slice), so list neighbours
 *                         with similar lengths next to each other
 *   mid_rows   [n_mid]    row ids reduced by one wavefront each
 *   long_rows  [n_long]   row ids reduced by a whole 16-wave workgroup with a fixed-order LDS combine
 * A call writes exactly the rows it lists (each at most once); with all three lists NULL every row of
 * [0, n_rows) takes the one-wavefront path.  The host normally covers all rows with one call, or with two calls
 * on two streams (short rows | mid + long rows) so the few heavy rows overlap the bulk.  The accumulation order
 * is fixed by the schedule, so results are run-to-run bit-stable for every degree distribution. */
int egnn_spmm_csr_f32(const egnn_spmm_t* op, int64_t* argmax, const int64_t* short_rows, int64_t n_short,
                      const int64_t* mid_rows, int64_t n_mid, const int64_t* long_rows, int64_t n_long, void* stream);

/* The same aggregation (EGNN_SUM / EGNN_MEAN) under a SEGMENT schedule: every row is cut into entry ranges of at most
 * ~64 entries and ALL ranges go through the sub-group-per-row kernel, so the few hub rows of a power-law graph (8 % of the
 * entries in 138 rows on the arxiv-shaped graph) get the same parallelism as the bulk instead of one workgroup each.
 *   seg       [n_seg,3] int64: (first entry, end entry, destination); destination < n_rows: that row of Y is written
 *             directly (the row's only range); destination >= n_rows: slot (destination - n_rows) of `partial`
 *   comb_rows [n_comb], comb_ptr [n_comb+1]: row r = comb_rows[i] is the sum of partial slots comb_ptr[i] .. comb_ptr[i+1]-1,
 *             added in slot order (fixed => bit-stable), then scaled (mean) and biased like a direct row
 *   partial   [partial_slots, K] fp32 workspace (16-byte aligned)
 * Requires K % 4 == 0 and 16-byte aligned X / Y / bias (else EGNN_EALIGN: use egnn_spmm_csr_f32).  Every row of
 * [0, n_rows) must be covered exactly once by the schedule (rows with no entries as an empty direct range). */
int egnn_spmm_csr_seg_f32(const egnn_spmm_t* op, const int64_t* seg, int64_t n_seg, const int64_t* comb_rows,
                          const int64_t* comb_ptr, int64_t n_comb, float* partial, int64_t partial_slots, void* stream);

/* The same aggregation (EGNN_SUM / EGNN_MEAN) under the ROW-BLOCK schedule (csrc/spmm_blk.hip), the default of the host
 * layer: ONE launch walks, per 128-byte column slice, first the hub segments and then blocks of `rows_per_blk`
 * consecutive rows (or rows [blk_ptr[b], blk_ptr[b+1]) when blk_ptr != NULL; every block at most rows_per_blk rows);
 * int32 indices (index_bits == 64 is EGNN_EALIGN); any K % 4 == 0; X addressed through a 32-bit buffer descriptor
 * (n_src * ldx * 4 < 2^31 bytes, else EGNN_EALIGN).  EGNN_EALIGN = shape not taken: the caller uses another schedule.
 *   hub_seg    [n_hub_seg,4] int32 (first entry, end entry, partial slot, 0): the entry ranges (<= seg_max entries each) of
 *              the rows with MORE than seg_max entries; their sums go to partial[slot,:] ([slots,K] fp32, 16-byte aligned)
 *              and the caller finishes those rows with egnn_spmm_combine_f32 on the SAME descriptor.
 *              Rows with at most seg_max entries are written here, completely.
 *   win        nullable [n_rows,2] int32 from egnn_spmm_blk_window_i32: entries [win[2r], win[2r+1]) of row r have their
 *              source inside row r's own block.  When given (square adjacency, X rows in node order, rows_per_blk a multiple
 *              of 128, <= 512) the block's X rows are streamed into LDS (LDS-DMA) while the out-of-block entries are
 *              gathered, and the in-block entries read LDS instead of L2 (graphs in a locality order).
 *   stat_part  here [egnn_spmm_blk_stat_rows(n_rows, rows_per_blk, win != NULL), 2, K]: one partial row per WAVE of every row
 *              block, over the rows that wave stored (egnn_bn_stats_merge_f32's n_blk = that row count)
 * CLASS WIDTHS (32 < K < 64: the 40-class output layer) without blk_ptr, win and stat_part take a form of their own: a 16-lane
 * sub-group per row (col / val read once per entry, not once per 128-byte slice), 16 rows per workgroup; rows_per_blk is not read.  Same hub_seg / partial / combine
 * contract, same summation order: bit-equal to egnn_spmm_csr_seg_f32 with cuts at seg_max. */
int egnn_spmm_csr_blk_f32(const egnn_spmm_t* op, int seg_max, int rows_per_blk, const int32_t* blk_ptr, int64_t n_blk,
                          const int32_t* win, const int32_t* hub_seg, int64_t n_hub_seg, float* partial, void* stream);
int64_t egnn_spmm_blk_stat_rows(int64_t n_rows, int rows_per_blk, int lds);
int egnn_spmm_blk_window_i32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int rows_per_blk,
                             const int32_t* blk_ptr, int64_t n_blk, int32_t* win, void* stream);
/* mean[c], var[c] (biased) of n_total rows of Y: the block partials of egnn_spmm_csr_blk_f32 plus the rows listed in
 * extra_rows (the hub rows, whose Y rows the combine step wrote), read from Y.  Fixed summation order (deterministic).
 * ws: egnn_bn_stats_merge_ws_floats(C) floats (needed when n_blk > 1024: the partials are folded in two short launches). */
size_t egnn_bn_stats_merge_ws_floats(int64_t C);
int egnn_bn_stats_merge_f32(const float* stat_part, int64_t n_blk, int64_t C, const float* Y, int64_t ldy,
                            const int64_t* extra_rows, int64_t n_extra, const float* stat_shift, int64_t n_total,
                            float* mean, float* var, float* ws, size_t ws_floats, void* stream);

/* The combine step on its own -- the hub rows of egnn_spmm_csr_blk_f32: Y[r] = (sum of partial slots comb_ptr[i] .. comb_ptr[i+1]-1
 * of row r = comb_rows[i], added in slot order) * (1 / rowcount for EGNN_MEAN) + bias (+ addend[r]).  K % 4 == 0, 16-byte
 * aligned rows.  Reads neither col, val, src_scale, X, ldx nor n_src (they may be unset); of flags only bit 3 (ReLU).
 * stat_part != NULL: row (stat_base + i) of the [*, 2, K] statistics partials receives (y - shift) and (y - shift)^2 of
 * combined row i (one partial row per hub row, folded by egnn_bn_stats_merge_f32 together with the block kernel's). */
int egnn_spmm_combine_f32(const egnn_spmm_t* op, const int64_t* comb_rows, const int64_t* comb_ptr, int64_t n_comb,
                          const float* partial, int64_t stat_base, void* stream);

/* Backward of EGNN_MAX: dX[col[argmax[i,k]], k] += val * dY[i,k].  dX must be zero-filled by the
 * caller.  Uses float atomics (the only entry point that does); max-aggregation is never exercised
 * by the reference and is provided because north_star names it. */
int egnn_spmm_csr_max_bwd_f32(int64_t n_rows, int64_t K, const void* col, int index_bits, const float* val,
                              const int64_t* argmax, const float* dY, int64_t ldy, float* dX, int64_t ldx,
                              void* stream);

/* EGNN_MAX over one PIECE of a row set -- the sharded run aggregates a shard's own columns while the halo rows travel and then
 * merges the halo columns' piece into the same (Y, argmax) state.  Descriptor as for egnn_spmm_csr_f32 with reduce == EGNN_MAX (val,
 * src_scale as there; bias, addend, stat_part or flags bit 3 set is EGNN_EINVAL: there is no epilogue); every row of [0, n_rows) takes the
 * one-wavefront path (64-entry chunks, float4 lanes where K % 4 == 0 and the rows are 16-byte aligned, else scalar lanes).
 *   entry_id   nullable [nnz] int64: the id recorded in argmax for entry e of this piece (NULL: e itself).  Must be strictly increasing
 *              within a row.  The sharded run passes the entry's position in the unsplit [own | halo] matrix, so that the merged argmax
 *              is the one a single egnn_spmm_csr_f32(EGNN_MAX) call over that matrix writes, bit for bit.
 *   merge      0: Y / argmax are written from scratch (an empty row: 0.0 and -1; with entry_id == NULL the result of egnn_spmm_csr_f32
 *              with its three row lists NULL).  1: Y / argmax hold the state earlier pieces over the same rows left.  A state with
 *              argmax < 0 is EMPTY and its Y value is not compared; otherwise the stored pair competes with this piece's candidates:
 *              the larger value wins, on equal values the smaller id.  A row that stays empty keeps 0.0 and -1.
 *   argmax     [n_rows, K] int64, required
 * No atomics: each wavefront owns its row's state.  The result does not depend on the order the pieces are applied in.
 * (op is the descriptor above, named by its struct tag.) */
int egnn_spmm_csr_max_piece_f32(const struct egnn_spmm* op, const int64_t* entry_id, int merge, int64_t* argmax, void* stream);

/* Backward of EGNN_MAX as a GATHER over the TRANSPOSED piece (deterministic; the form the sharded run uses):
 *   dX[j,k] = addend[j,k] + sum_p (argmax[t_row[p],k] == t_eid[p] ? val[t_eid[p]] * dY[t_row[p],k] : 0),  p in [t_rowptr[j], t_rowptr[j+1])
 * added in p order.  EVERY row j of dX [n_src, K] is written -- no zero-fill by the caller; rows no target picked receive the addend,
 * or an exact 0 -- no atomics, fixed summation order (run-to-run bit-stable).
 *   t_rowptr   [n_src + 1], t_row [nnz]: the transposed structure (target row of transposed entry p), index_bits wide
 *   t_eid      [nnz] int64: the forward id of transposed entry p, in the numbering argmax is expressed in
 *   val        nullable, indexed by FORWARD id (= 1.0)
 *   argmax     [n_rows, K] int64 (leading dimension K), dY [n_rows, ldy]
 *   addend     nullable [n_src, ld_addend]
 * Reads nnz * K argmax words against the n_rows * K of the scatter form above. */
int egnn_spmm_csr_max_bwd_rows_f32(int64_t n_src, int64_t n_rows, int64_t K, const void* t_rowptr, const void* t_row, int index_bits,
                                   const int64_t* t_eid, const float* val, const int64_t* argmax, const float* dY, int64_t ldy,
                                   const float* addend, int64_t ld_addend, float* dX, int64_t ldx, void* stream);

/* Gradient of an aggregation with respect to its ENTRY VALUES -- a sampled dense-dense product (SDDMM) over the CSR pattern
 * (csrc/sddmm.hip; torch-sparse `spmm` value backward):
 *   dval[e] = row_scale[r] * sum_k m(e,k) * G[r,k] * X[col[e],k],   r = row of entry e,  e in [0, nnz)
 *   G          [n_rows, ldg]  the incoming dY;  X [n_src, ldx]  the aggregation's dense operand
 *   rowptr     [n_rows + 1], col [nnz]: index_bits (32 | 64) wide, as in egnn_spmm_t; nnz = rowptr[n_rows], passed by the caller
 *   row_scale  nullable [n_rows] (= 1.0): EGNN_MEAN passes 1 / max(stored entries of the row, 1) -- mean divides by the entry count,
 *              not by the sum of the values
 *   argmax     nullable [n_rows, K] int64 (leading dimension K).  NULL: m = 1 (EGNN_SUM / EGNN_MEAN).  Otherwise m(e,k) =
 *              (argmax[r,k] == e): the subgradient of EGNN_MAX at the entry the forward picked (the first maximal one in CSR order,
 *              the tie rule of dX)
 *   dval       [nnz]: EVERY entry is written exactly once -- no zero-fill by the caller; nnz == 0 launches nothing
 * Work is cut over entries, not rows: a wavefront owns 256 consecutive entries and finds their rows from rowptr (one wave-uniform binary
 * search, then a forward walk), so a hub row is no wavefront's serial job.  A group of G lanes owns one entry (G = the power of two at or
 * above ceil(K / 4), at most 64; float4 lanes, looping when K > 256); K % 4 != 0 or rows that are not 16-byte aligned take scalar lanes.
 * No atomics, fixed summation order per entry: two calls on the same inputs are bit-equal. */
int egnn_sddmm_csr_f32(int64_t n_rows, int64_t n_src, int64_t K, const void* rowptr, const void* col, int index_bits, int64_t nnz,
                       const float* G, int64_t ldg, const float* X, int64_t ldx, const float* row_scale, const int64_t* argmax,
                       float* dval, void* stream);

/* Algorithmic (compulsory) HBM bytes of one egnn_spmm_csr_f32 call, SURVEY.md 8(d):
 * 4*n_src*K (read X) + 4*n_rows*K (write Y) + nnz*(index bytes + value bytes) + rowptr. */
int64_t egnn_spmm_algorithmic_bytes(int64_t n_rows, int64_t n_src, int64_t K, int64_t nnz, int index_bits,
                                    int has_val);

/* ------------------------------------------------------------------------------------------------
 * Graph structure (integer work is bit-exact vs torch-sparse semantics)
 * ---------------------------------------------------------------------------------------------- */
/* Edge list -> CSR sorted by (row, col), on the device (hipCUB radix sort over the bits the keys use; bit-exact).
 *   symmetric == 0: T.ToSparseTensor() (/root/reference/arxiv_pyg/gnn.py:237): duplicates are KEPT;
 *                   pass row = edge targets, col = edge sources; col_out holds E entries.
 *   symmetric != 0: SparseTensor.to_symmetric() (gnn.py:240): union of (r,c) and (c,r), duplicates merged;
 *                   col_out needs room for 2*E entries.
 * rowptr [N+1], nnz_out [1] (device scalar: the entry count, = E when symmetric == 0).  ws: egnn_csr_from_coo_ws_bytes.
 * Requires N < 3 037 000 499 (row * N + col in int64) and fewer than 2^31 keys. */
size_t egnn_csr_from_coo_ws_bytes(int64_t E, int64_t N, int symmetric);
int egnn_csr_from_coo_i64(const int64_t* row, const int64_t* col, int64_t E, int64_t N, int symmetric,
                          int64_t* rowptr, int64_t* col_out, int64_t* nnz_out, void* ws, size_t ws_bytes, void* stream);

/* CSR -> CSC: colptr [n_cols+1], row_out [nnz] (the rows of each column, ascending) and perm [nnz] = the csr2csc
 * permutation torch-sparse caches for the backward SpMM (stable sort of the entries by column; SURVEY 9.6,
 * /root/reference/arxiv_pyg/gnn.py:192): value_csc = value[perm].  ws: egnn_csr_transpose_ws_bytes(nnz, n_cols). */
size_t egnn_csr_transpose_ws_bytes(int64_t nnz, int64_t n_cols);
int egnn_csr_transpose_i64(const int64_t* rowptr, const int64_t* col, int64_t n_rows, int64_t n_cols, int64_t nnz,
                           int64_t* colptr, int64_t* row_out, int64_t* perm, void* ws, size_t ws_bytes, void* stream);

/* rowptr[i] = #entries with row < i, for i in [0, n_rows]; `row` sorted ascending.
 * Replaces torch_sparse ind2ptr inside T.ToSparseTensor()  /root/reference/arxiv_pyg/gnn.py:237. */
int egnn_rowptr_from_sorted_rows_i64(const int64_t* row, int64_t nnz, int64_t n_rows, int64_t* rowptr, void* stream);

/* int64 -> int32 narrowing of an index array; *overflow (device int32, caller-zeroed) is set to 1
 * if any element does not fit. */
int egnn_narrow_i64_to_i32(const int64_t* src, int64_t n, int32_t* dst, int32_t* overflow, void* stream);

/* gcn_norm on a value-less, row-sorted CSR (GCNConv first forward, /root/reference/arxiv_pyg/gnn.py:28-35;
 * SURVEY 9.3): A^ = D^-1/2 (A + I) D^-1/2 with fill_diag(1) replacing any stored diagonal.
 *  step 1: out_count[i] = #off-diagonal entries of row i + 1                 (caller scans -> rowptr_out)
 *  step 2: writes col_out (diagonal inserted at its sorted slot) and dinv[i] = deg^-1/2 (inf -> 0)
 *  step 3: val_out[e] = (1 * dinv[row(e)]) * dinv[col_out[e]]
 */
int egnn_gcn_norm_count_i64(const int64_t* rowptr, const int64_t* col, int64_t n, int64_t* out_count, void* stream);
int egnn_gcn_norm_fill_i64(const int64_t* rowptr, const int64_t* col, int64_t n, const int64_t* rowptr_out,
                           int64_t* col_out, float* dinv, void* stream);
int egnn_gcn_norm_values_i64(const int64_t* rowptr_out, const int64_t* col_out, int64_t n, const float* dinv,
                             float* val_out, void* stream);

/* gcn_norm on a VALUED row-sorted CSR (PyG gcn_norm, SparseTensor branch with weights): same structure as above
 * (step 1 and rowptr_out are shared, col_out comes out bit-equal), then
 *  fill:  every off-diagonal entry carries its value to its new slot (val_out), the inserted diagonal gets 1.0; a stored diagonal
 *         entry is dropped whatever its weight.  slot (nullable, [nnz]): new position of input entry e, -1 for a dropped one -- the
 *         map the backward reads the weight gradients through.
 *  (the caller forms deg = row sums of the filled values in entry order: egnn_segment_sum_f32 over rowptr_out)
 *  scale: dinv[i] = deg[i]^-1/2 (inf -> 0), val_out[e] = (w[e] * dinv[row(e)]) * dinv[col_out[e]]; w = the filled values.  Also the
 *         PyG <= 1.7 edge-index branch with edge_weight, on the target-major CSR of the edges after add_remaining_self_loops. */
int egnn_gcn_norm_fill_val_i64(const int64_t* rowptr, const int64_t* col, const float* val, int64_t n, const int64_t* rowptr_out,
                               int64_t* col_out, float* val_out, int64_t* slot, void* stream);
int egnn_gcn_norm_scale_i64(const int64_t* rowptr_out, const int64_t* col_out, int64_t n, const float* w, const float* deg,
                            float* dinv, float* val_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dense fp32 GEMM on the f32-input MFMA (v_mfma_f32_32x32x2_f32, exact fp32 == fmaf chain).
 * C[M,N] = alpha * op(A)[M,K] * op(B)[K,N] (+ bias[N]) ; op = identity or transpose.
 *   trans_a = 0: A is [M,K] row-major (lda >= K);  trans_a = 1: A is stored [K,M] (lda >= M)
 *   trans_b = 0: B is [K,N] row-major (ldb >= N);  trans_b = 1: B is stored [N,K] (ldb >= K)
 * Replaces cuBLAS SGEMM under torch.matmul / nn.Linear (K4): GCNConv `x @ W`
 * (/root/reference/arxiv_pyg/gnn.py:47), SAGEConv lin_l/lin_r (:79), projection heads (:296-306) and
 * their backward (dX = dY W^T, dW = X^T dY).
 * split_k > 1 writes split_k partial products into `ws` ([split_k, M, N] floats) and reduces them in
 * a fixed order (deterministic); ws may be NULL when split_k <= 1.
 * ---------------------------------------------------------------------------------------------- */
/* Workspace floats a call with these arguments needs (split-K partials; the row-chunk partials of the class-count-wide dW
 * form of csrc/gemm_skinny.hip).  0 = none. */
size_t egnn_gemm_ws_floats(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, int split_k);
int egnn_gemm_f32(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, float alpha,
                  const float* A, int64_t lda, const float* B, int64_t ldb,
                  const float* bias, float* C, int64_t ldc,
                  int split_k, float* ws, size_t ws_bytes, void* stream);

/* Which kernel the last egnn_gemm_f32 / _ex_ / _add_ / _rows_ call of the calling thread ran (host-only, thread-local; 0 after a
 * call that launched nothing: an empty output or an error found before the dispatch).  Written at the one place where the
 * dispatcher commits to a kernel, so a test can assert the route it means to exercise:
 *   bits 0-7   form: 1 skinny_fwd_tile (K = 256 rows through an LDS tile), 2 skinny_fwd, 3 skinny_dx, 4 skinny_dw with the narrow
 *              matrix = A, 5 skinny_dw with the narrow matrix = B, 6 DMA form, 7 general 128x64 tile, 8 general 128x128 tile
 *   bit 8      vec4: 16-byte operand loads (forms 7, 8)
 *   bit 9      wide_store: 16-byte stores through LDS (forms 6, 7, 8; for split_k > 1 it describes the partial store)
 *   bit 10     products on the bf16 split pipe (form 6 always; form 8 unless EGNN_GEMM_PIPE=f32; the 128x64 tile has no split form)
 *   bit 11     row gather fused into A (a_rows);   bit 12   row gather fused into B (b_rows)
 *   bits 16+   the split_k in effect after clamping to the number of k-steps (forms 6, 7, 8; >= 1)
 * The skinny forms (1-5) report the form alone. */
int egnn_gemm_last_route(void);

/* egnn_gemm_f32 with an epilogue option: flags bit 0 (1) = C = max(alpha op(A) op(B) + bias, 0) -- the ReLU that follows an
 * eval-mode BatchNorm whose scale / shift were folded into B and bias (egnn_bn_fold_f32). */
int egnn_gemm_ex_f32(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, float alpha, const float* A, int64_t lda,
                     const float* B, int64_t ldb, const float* bias, float* C, int64_t ldc, int split_k, float* ws,
                     size_t ws_bytes, int flags, void* stream);
/* egnn_gemm_f32 with an accumulating store: C = alpha op(A) op(B) + bias + addend (addend [M,N], ld_addend >= N, nullable; may be C
 * itself only if nothing else reads it).  SAGEConv's lin_l(agg) + lin_r(x) (/root/reference/arxiv_pyg/gnn.py:79-84 via PyG SAGEConv.forward,
 * SURVEY 9.5) and the two-path input gradient of its backward become one store each instead of a GEMM + an element-wise pass. */
int egnn_gemm_add_f32(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, float alpha, const float* A, int64_t lda,
                      const float* B, int64_t ldb, const float* bias, const float* addend, int64_t ld_addend, float* C, int64_t ldc,
                      int split_k, float* ws, size_t ws_bytes, void* stream);
/* The same GEMM with a row gather fused into one operand's load, for the `feat[train_idx]` gathers in front of the
 * projection heads (/root/reference/arxiv_pyg/gnn.py:150-156: `out_feat[train_idx]`, `teacher_out_feat[train_idx]`,
 * the latter 273 MB read + written per step in the reference):
 *   a_rows [M] (requires trans_a == 0): row m of op(A) is row a_rows[m] of the matrix at A        (y = x[idx] W^T)
 *   b_rows [K] (requires trans_b == 0): row k of B      is row b_rows[k] of the matrix at B        (dW = dY^T x[idx])
 * At most one of them; both NULL = egnn_gemm_f32.  Ids must be valid row numbers (not checked on the device). */
int egnn_gemm_rows_f32(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, float alpha,
                       const float* A, int64_t lda, const int64_t* a_rows, const float* B, int64_t ldb, const int64_t* b_rows,
                       const float* bias, float* C, int64_t ldc,
                       int split_k, float* ws, size_t ws_bytes, void* stream);

/* C [M, N] = alpha A^T B[b_rows] for a CONSTANT B (dW = dY^T x[idx] of a Linear over a constant input: the teacher projection head
 * of /root/reference/arxiv_pyg/gnn.py:296-306, whose input -- the teacher's [N, 750] features -- never changes): B's gathered rows
 * are cut ONCE into tile-packed bf16 planes with the gathered row index as the reduction dimension (egnn_gemm_tn_planes_pack_f32;
 * egnn_gemm_tn_planes_bytes of 1 KB-aligned device memory, 6 bytes per element); every later product reads A [K, M] (lda >= M,
 * 16-byte aligned rows, M % 256 == 0) down LDS columns against those planes -- no gather and no operand cut in the loop.  Same
 * six-product fp32 arithmetic as egnn_gemm_f32 on the bf16 pipe; fixed-order split over k (workspace egnn_gemm_tn_planes_ws_floats).
 * EGNN_EALIGN: shape / alignment not taken, or EGNN_GEMM_PIPE=f32 (callers then use egnn_gemm_rows_f32). */
size_t egnn_gemm_tn_planes_bytes(int64_t N, int64_t K);
int egnn_gemm_tn_planes_pack_f32(const float* B, int64_t ldb, const int64_t* b_rows, int64_t N, int64_t K, void* planes,
                                 size_t planes_bytes, void* stream);
size_t egnn_gemm_tn_planes_ws_floats(int64_t M, int64_t N, int64_t K);
int egnn_gemm_tn_planes_f32(int64_t M, int64_t N, int64_t K, float alpha, const float* A, int64_t lda, const void* planes, float* C,
                            int64_t ldc, float* ws, size_t ws_floats, void* stream);

/* The forward of the same Linear, C [M, N] = alpha A[a_rows] B^T + bias (B stored [N, K] as nn.Linear keeps its weight; N % 128 == 0):
 * the CONSTANT A's gathered rows are cut once into planes (row blocks of 128 gathered rows x k-steps of 16: the gather is baked in),
 * B is cut per call into the workspace (egnn_gemm_rows_planes_ws_bytes); both operand tiles then travel global -> LDS as lane-linear
 * DMA copies with no VALU work in the loop.  Same arithmetic and return codes as above. */
size_t egnn_gemm_rows_planes_bytes(int64_t M, int64_t K);
int egnn_gemm_rows_planes_pack_f32(const float* A, int64_t lda, const int64_t* a_rows, int64_t M, int64_t K, void* planes,
                                   size_t planes_bytes, void* stream);
size_t egnn_gemm_rows_planes_ws_bytes(int64_t N, int64_t K);
int egnn_gemm_rows_planes_f32(int64_t M, int64_t N, int64_t K, float alpha, const void* planes_a, const float* B, int64_t ldb,
                              const float* bias, float* C, int64_t ldc, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused losses (K5-K7).  Every loss entry point comes as fwd (scalars out) + bwd (input grads out);
 * upstream gradients are passed as DEVICE scalars so that no host sync is needed.
 * ---------------------------------------------------------------------------------------------- */

/* Row-wise cross entropy + logit-KD, /root/reference/arxiv_pyg/criterion.py:8-21 (and the
 * `loss_cls = F.cross_entropy(logits, labels)` first line of every criterion, :26,41,60,98,132).
 * Row i of the loss reads row r = rows ? rows[i] : i of logits / teacher and labels[r]: with a row list the
 * `out[train_idx]`, `y[train_idx]`, `teacher_logits[train_idx]` gathers of train() (gnn.py:107-116) are fused into the
 * operand loads (logits / teacher / labels are then the FULL [N,*] arrays).  A label outside [0, C) is ignored the
 * way F.cross_entropy ignores ignore_index (no loss, no gradient, not counted in the mean); it is never an address.
 *   out3[0] = mean over valid-label rows of CE(logits_r, labels_r)
 *   out3[1] = sum_{i,c} p_t (log p_t - log q) / (n*C)   (F.kl_div default reduction='mean'), q = softmax(logits/T),
 *             p_t = softmax(teacher/T); 0 when teacher == NULL
 *   out3[2] = number of valid-label rows (the backward's CE denominator)
 * partials: workspace of egnn_ce_kd_ws_floats(n) floats. */
size_t egnn_ce_kd_ws_floats(int64_t n);
int egnn_ce_kd_fwd_f32(const float* logits, int64_t ld_logits, const float* teacher, int64_t ld_teacher,
                       const int64_t* labels, const int64_t* rows, int64_t n, int64_t C, float T,
                       float* out3, float* partials, void* stream);
/* dlogits[r,c] = g_cls * (softmax(logits_r)_c - [c == label_r]) / out3[2]  +  g_kd * (q_rc - p_t,rc) / (T * n * C)
 * g_cls / g_kd: device scalars (nullable = 0); out3: the forward's output.  With a row list, dlogits is the full
 * [n_total_rows, C] block: it is cleared first and only the listed rows are written (the scatter of the
 * `out[train_idx]` backward). */
int egnn_ce_kd_bwd_f32(const float* logits, int64_t ld_logits, const float* teacher, int64_t ld_teacher,
                       const int64_t* labels, const int64_t* rows, int64_t n_total_rows, int64_t n, int64_t C, float T,
                       const float* out3, const float* g_cls, const float* g_kd, float* dlogits, int64_t ld_dlogits,
                       void* stream);

/* Gather + L2 row normalisation:  out[i,:] = x[idx[i],:] / max(||x[idx[i],:]||_2, eps), inv_norm[i] = 1/max(..).
 * idx nullable (identity).  F.normalize in criterion.py:29-30,71-72,139-140 fused with the
 * `feat[sampled_inds]` gather (:64-65,136-137). */
int egnn_gather_normalize_rows_f32(const float* x, int64_t ldx, const int64_t* idx, int64_t n, int64_t D, float eps,
                                   float* out, int64_t ldo, float* inv_norm, void* stream);
/* Backward of the above: dx[idx[i],:] (+)= inv_norm[i] * (dout[i,:] - xhat[i,:] * <dout[i,:], xhat[i,:]>)
 * (zero where the eps clamp was active).  `accumulate` != 0 adds into dx (rows of idx are unique). */
int egnn_normalize_rows_bwd_f32(const float* xhat, int64_t ldh, const float* dout, int64_t ldd, const float* inv_norm,
                                const int64_t* idx, int64_t n, int64_t D, float eps,
                                float* dx, int64_t ldx, int accumulate, void* stream);

/* G-CRD / InfoNCE, /root/reference/arxiv_pyg/criterion.py:139-145:
 *   Z = fhat that^T / tau  ([S,S]);  loss = mean_i( logsumexp_j Z_ij - Z_ii ).
 * fwd: Z tiles are produced on the fp32 MFMA, the row log-sum-exp is accumulated online per lane and
 *      merged in a fixed order; the scores are saved in `Z` ([S,S], ld = S) for the backward when Z != NULL.
 *      lse [S] and the scalar loss are outputs.  ws: egnn_nce_ws_floats(S) floats.
 *      unit_rows != 0 asserts ||fhat_i|| = ||that_j|| = 1 (what criterion.py:139-140 guarantees): logits are then
 *      bounded by 1/tau and that bound replaces the running row maximum (one exp per element, half the state);
 *      with unit_rows == 0 (or tau < 0.025) the general online-max form runs.
 *      What `Z` holds: the logits Z_ij in the general form; E_ij = exp(Z_ij - 1.0001/tau) in the unit-rows form
 *      (egnn_nce_saves_exp(tau, unit_rows) tells which) -- the forward needs E for the row sums anyway, and with
 *      w_i = exp(1.0001/tau - lse_i) the backward becomes two exp-free GEMMs on E.
 * bwd: dfhat = g/(S tau) (P - I) that ; dthat = g/(S tau) (P - I)^T fhat, P = exp(Z - lse) = diag(w) E; g device
 *      scalar.  Requires the `Z` written by fwd and the SAME tau / unit_rows.
 *      ws (nullable): egnn_nce_bwd_ws_floats(S, S, P) floats.  With it the two GEMMs (reduction length S, only
 *      S*P outputs) split their reduction over enough workgroups to fill the chip and sum the partials in a fixed
 *      order; without it they fall back to smaller row tiles. */
size_t egnn_nce_ws_floats(int64_t S);
size_t egnn_nce_bwd_ws_floats(int64_t Sr, int64_t Sc, int64_t P);
int egnn_nce_saves_exp(float tau, int unit_rows);
int egnn_nce_fwd_f32(const float* fhat, const float* that, int64_t S, int64_t P, int64_t ld, float tau, int unit_rows,
                     float* Z, float* lse, float* loss, float* ws, size_t ws_floats, void* stream);
int egnn_nce_bwd_f32(const float* fhat, const float* that, int64_t S, int64_t P, int64_t ld, float tau, int unit_rows,
                     const float* Z, const float* lse, const float* g,
                     float* dfhat, float* dthat, float* ws, size_t ws_floats, void* stream);

/* Row-block form of the two entry points above, for node-range sharding: this rank owns Sr of the
 * S_total sampled rows, `that` holds ALL Sc = S_total teacher rows (all-gathered over RCCL), and the positive of
 * local row i is column i + diag_off.  loss = inv_count * sum_i (lse_i - Z_i,i+off)  (pass 1/S_total and all-reduce);
 * dfhat [Sr,P] is complete, dthat [Sc,P] is this rank's contribution (all-reduce it); scale = 1 / (S_total * tau).
 * Z is [Sr,Sc] (ld = Sc); fwd ws: egnn_nce_ws_floats(Sr); bwd ws (nullable): egnn_nce_bwd_ws_floats(Sr, Sc, P). */
int egnn_nce_block_fwd_f32(const float* fhat, int64_t ld_f, const float* that, int64_t ld_t, int64_t Sr, int64_t Sc,
                           int64_t diag_off, int64_t P, float tau, float inv_count, int unit_rows, float* Z, float* lse,
                           float* loss, float* ws, size_t ws_floats, void* stream);
int egnn_nce_block_bwd_f32(const float* fhat, int64_t ld_f, const float* that, int64_t ld_t, int64_t Sr, int64_t Sc,
                           int64_t diag_off, int64_t P, float tau, float scale, int unit_rows, const float* Z,
                           const float* lse, const float* g, float* dfhat, int64_t ld_df, float* dthat, int64_t ld_dt,
                           float* ws, size_t ws_floats, void* stream);

/* GSP all-pairs similarity loss, /root/reference/arxiv_pyg/criterion.py:69-88:
 *   loss = mean_ij (k(xs_i,xs_j) - k(xt_i,xt_j))^2 ; kernel: EGNN_K_COSINE / _POLY (rows must be unit vectors,
 *   criterion.py:71-72,76-77) or EGNN_K_L2 / _RBF (raw rows; ||a-b||^2 via ||a||^2+||b||^2-2<a,b>, diagonal exact 0;
 *   the reference's [S,S,D] difference tensor is never formed).
 * Writes Ws, Wt ([S,S], ld = S) such that, for an upstream gradient g,
 *   dxs = g * (Ws xs - rowsum(Ws) o xs),  dxt = g * (Wt xt - rowsum(Wt) o xt)   (rowsum term for L2/RBF only),
 * i.e. one egnn_gemm_f32 + egnn_rowsum_f32 + egnn_scale_rowcorr_f32 per side.  ws: egnn_gsp_ws_floats(S). */
#define EGNN_K_COSINE 0
#define EGNN_K_POLY 1
#define EGNN_K_L2 2
#define EGNN_K_RBF 3
size_t egnn_gsp_ws_floats(int64_t S);
int egnn_gsp_fwd_f32(const float* xs, int64_t ld_s, int64_t Ps, const float* xt, int64_t ld_t, int64_t Pt, int64_t S,
                     int kernel, float* Ws, float* Wt, float* loss, float* ws, size_t ws_floats, void* stream);
/* out[i] = sum_j W[i,j] (fixed order) */
int egnn_rowsum_f32(const float* W, int64_t ld, int64_t n, int64_t m, float* out, void* stream);
/* out[i,:] = g * (WX[i,:] - r[i] * X[i,:]);  r nullable (no correction), g nullable device scalar (= 1) */
int egnn_scale_rowcorr_f32(const float* WX, int64_t ldw, const float* X, int64_t ldx, const float* r, const float* g,
                           int64_t n, int64_t P, float* out, int64_t ldo, void* stream);

/* PPI multi-label logit KD, /root/reference/ppi_pyg/criterion.py:11-13: out2[0] = mean BCEWithLogits(logits, labels),
 * out2[1] = mean BCEWithLogits(logits, sigmoid(teacher)) over all `total` = n*C elements (contiguous arrays). */
size_t egnn_bce_pair_ws_floats(void);
int egnn_bce_pair_fwd_f32(const float* logits, const float* labels, const float* teacher, int64_t total, float* out2,
                          float* ws, void* stream);
int egnn_bce_pair_bwd_f32(const float* logits, const float* labels, const float* teacher, int64_t total,
                          const float* g_cls, const float* g_kd, float* dlogits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LSP building blocks, /root/reference/arxiv_pyg/criterion.py:95-126 (K5/K6 in SURVEY.md 2.2)
 * ---------------------------------------------------------------------------------------------- */
/* Per-edge similarity of rows a = F[idx_a[e]], b = F[idx_b[e]] (never materialising feat[src] / feat[dst]):
 *   EGNN_K_COSINE  <a,b> / sqrt(max(|a|^2 |b|^2, 1e-16))   (F.cosine_similarity, criterion.py:103)
 *   EGNN_K_POLY    cosine^2 (:106)      EGNN_K_L2  ||a-b||_2 (:109)      EGNN_K_RBF  exp(-||a-b||^2 / 2) (:112)
 * aux3 [E,3] keeps (dot,|a|^2,|b|^2) or (||a-b||^2,0,0) for the backward. */
int egnn_edge_sim_f32(const float* F, int64_t ld, int64_t D, const int64_t* idx_a, const int64_t* idx_b, int64_t E,
                      int kernel, float* sim, float* aux3, void* stream);
/* Backward coefficients: with g = dL/dsim,  dL/dF[a] += alpha*b + beta_a*a  and  dL/dF[b] += alpha*a + beta_b*b per edge;
 * the caller turns them into two egnn_spmm_csr_f32 calls (values = alpha) plus a per-row scale (segment sums of beta). */
int egnn_edge_sim_coef_f32(const float* g, const float* sim, const float* aux3, int64_t E, int kernel,
                           float* alpha, float* beta_a, float* beta_b, void* stream);
/* torch_geometric.utils.softmax over CSR segments: p = exp(x - max_seg) / (sum_seg + 1e-16); x, p in segment
 * order (seg_ptr [n_seg+1]).  bwd: gx = p * (gp - sum_seg p*gp).  No atomics, fixed order. */
int egnn_segment_softmax_fwd_f32(const int64_t* seg_ptr, const float* x, int64_t n_seg, float* p, void* stream);
int egnn_segment_softmax_bwd_f32(const int64_t* seg_ptr, const float* p, const float* gp, int64_t n_seg, float* gx, void* stream);
int egnn_segment_sum_f32(const int64_t* seg_ptr, const float* x, int64_t n_seg, float* out, void* stream);

/* Tail of lpw_criterion (/root/reference/arxiv_pyg/criterion.py:103-122) in one pass per direction: both segment softmaxes of
 * the student / teacher similarity vectors (same PyG form as above), the element-wise criterion and its mean over the E edges:
 *   criterion 0 (kld): F.kl_div(log p_s, p_t, reduction='mean') = mean_e p_t (log p_t - log p_s), 0 where p_t == 0   (:118)
 *   criterion 1 (mse): F.mse_loss(p_s, p_t)                                                                          (:120)
 * p_s, p_t [E] are written for the backward; loss [1]; ws: egnn_lsp_loss_ws_floats() floats.  Fixed summation order.
 * bwd: g [1] = dL/dloss on the device; gsim_s [E] = dL/dsim_s; gsim_t [E] nullable (= dL/dsim_t when the teacher side needs one). */
size_t egnn_lsp_loss_ws_floats(void);
int egnn_lsp_loss_fwd_f32(const int64_t* seg_ptr, const float* sim_s, const float* sim_t, int64_t n_seg, int64_t E,
                          int criterion, float* p_s, float* p_t, float* loss, float* ws, void* stream);
int egnn_lsp_loss_bwd_f32(const int64_t* seg_ptr, const float* p_s, const float* p_t, int64_t n_seg, int64_t E,
                          int criterion, const float* g, float* gsim_s, float* gsim_t, void* stream);

/* out[c] = sum_r x[r, c] of a row-major [n, C] matrix (leading dimension ld): the bias gradients of GCNConv / nn.Linear
 * (arxiv_pyg/gnn.py:28-33 modules' `bias`), fixed row stripes + fixed-order finalize.  ws: egnn_colsum_ws_floats(C) floats. */
size_t egnn_colsum_ws_floats(int64_t C);
int egnn_colsum_f32(const float* x, int64_t ld, int64_t n, int64_t C, float* out, float* ws, void* stream);

/* GAT attention coefficients (the teacher that the PPI / MAG train loops run inside the student step,
 * /root/reference/ppi_pyg/gnn.py:86-117,208-209; PyG <=1.7 GATConv.message + utils.softmax):
 *   s[e,h]   = leaky_relu(alpha_src[col[e],h] + alpha_dst[row(e),h], negative_slope)          (u_add_v SDDMM)
 *   att[h,e] = exp(s - max over the row's entries) / (sum exp(..) + 1e-16)                     (edge softmax per target)
 * rowptr / col: CSR by target, int64; alpha_src [n_src,H], alpha_dst [n_rows,H] row-major; att is HEAD-major [H,nnz]
 * so that head h's values are a contiguous per-entry array for egnn_spmm_csr_*_f32 (u_mul_e_sum).  Backward:
 * egnn_gat_layer_bwd_f32 below. */
int egnn_gat_attention_fwd_f32(const int64_t* rowptr, const int64_t* col, const float* alpha_src, const float* alpha_dst,
                               int64_t n_rows, int64_t nnz, int H, float negative_slope, float* att, void* stream);

/* One GAT layer's attention + aggregation in training, for both layer kinds; csrc/gat.hip, deterministic (fixed summation orders,
 * no atomics).  The operands travel as ONE descriptor, egnn_gat_layer_t, read only while the call runs (it may live on the
 * caller's stack).
 *   - PyG <=1.7 GATConv (the PPI GAT student and teacher, /root/reference/ppi_pyg/gnn.py:50-83 StudentNet, :23-47 TeacherNet trained
 *     by ppi_pyg/train_teacher.py): el / er are its alpha_src / alpha_dst, attn_l / attn_r its att_l / att_r; keep, src_scale
 *     and dst_scale are NULL (read r = q = 1 below).  Its forward is egnn_gat_attention_fwd_f32 + one valued aggregation per head.
 *   - the arxiv GAT teacher's layer (the reference's own GATConv over DGL message passing, /root/reference/arxiv_dgl/models.py:95-236;
 *     trained by arxiv_dgl/gat.py:116-148 with --use-norm --no-attn-dst --edge-drop=0.3, arxiv_dgl/scripts/gat-teachers.sh): every
 *     field in use; forward and backward through the two entry points below.
 * Square message graph of n nodes, CSR by target (rowptr / col) and, for the backward, its transposed structure (colptr [n+1],
 * t_col / perm [nnz]: entry p of source column j is CSR entry perm[p] of target row t_col[p]; SparseTensor._transpose_meta; not
 * read by the forward).
 *   xl [n, ld_xl >= H*C]  the projected features, UNSCALED, read in place (any C: 16-, 8- or 4-byte aligned head blocks)
 *   el [n,H]              <r_j xl[j,h,:], attn_l[h,:]> (from the scaled source features, models.py:179-196)
 *   er [n,H] nullable     <xl[i,h,:], attn_r[h,:]> (from the unscaled ones, :199-200); NULL together with attn_r (--no-attn-dst)
 *   keep [nnz] bytes, nullable      the entries edge_drop keeps (models.py:207-212); the softmax runs over the kept entries
 *   mult [H,nnz] nullable           the attention-dropout multiplier (mask / (1 - p))
 *   src_scale r [n], dst_scale q [n], nullable   out-degree^-1/2 and in-degree^1/2 of use_symmetric_norm (:179-184,220-225)
 * Forward, one launch for all heads:
 *   s_e = leaky_relu(el[col e,h] + er[i,h]);  att[h,e] = softmax of s over the kept entries of row i, exactly 0 at dropped
 *   entries (a row without a kept entry: all zeros);  out[i,h,:] = q_i sum_e att[h,e] mult[h,e] r_{col e} xl[col e,h,:]
 *   att [H,nnz] head-major; out [n, ld_out >= H*C].
 * Backward, three launches for all heads (target side: one wavefront per target row; source side: one wavefront per source row
 * over the transposed structure; a fixed-order finalize of d_attn).  go = d out: [n, ld_go >= H*C] (mean_heads == 0), or, with
 * mean_heads != 0, [n, ld_go >= C] = the gradient of the average over the heads, read by every head and scaled by 1/H.
 * With go' = q_i go_i and s_e recomputed from el / er as the forward formed it:
 *   g_e = mult_e r_{col e} <go'_i, xl[col e]>;  d_raw[h,e] = att_e (g_e - sum_row att g) * (s_e > 0 ? 1 : negative_slope)
 *   d_er[i,h] = sum_row d_raw (NULL with er);  d_el[j,h] = sum_{col e = j} d_raw
 *   dxl[j,h,:] = r_j (sum_{col e = j} att_e mult_e go'_{row e} + d_el[j,h] attn_l[h,:]) + d_er[j,h] attn_r[h,:]
 *   d_attn [2,H*C] nullable: d_attn[0] = sum_j r_j xl_j d_el[j] (= d attn_l), d_attn[1] = sum_j xl_j d_er[j] (= d attn_r), as
 *   per-block partials in ws + the finalize; needs H*C <= 2048 and ws of egnn_gat_layer_bwd_ws_floats(n, H, C) floats.
 *   dxl [n, ld_dxl >= H*C];  d_raw [H,nnz]: scratch of the call. */
typedef struct egnn_gat_layer {
  const int64_t* rowptr; const int64_t* col;
  const int64_t* colptr; const int64_t* t_col; const int64_t* perm;
  int64_t n; int64_t nnz; int H; int C;
  const float* xl; int64_t ld_xl;
  const float* el; const float* er;
  const float* attn_l; const float* attn_r;
  const uint8_t* keep; const float* mult; const float* src_scale; const float* dst_scale;
  float negative_slope;
} egnn_gat_layer_t;
int egnn_gat_layer_fwd_f32(const egnn_gat_layer_t* layer, float* att, float* out, int64_t ld_out, void* stream);
size_t egnn_gat_layer_bwd_ws_floats(int64_t n, int H, int C);
int egnn_gat_layer_bwd_f32(const egnn_gat_layer_t* layer, const float* att, const float* go, int64_t ld_go, int mean_heads, float* d_raw,
                           float* d_er, float* dxl, int64_t ld_dxl, float* d_attn, float* ws, size_t ws_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused BatchNorm1d (+ ReLU + dropout) over node rows -- SURVEY.md 8(f) rank 1; replaces the ATen BatchNorm /
 * threshold / fused_dropout chain at /root/reference/arxiv_pyg/gnn.py:48-50,80-82,296-306.
 * Shapes: x [n,C] fp32, C % 4 == 0, C <= 1024, ld % 4 == 0, 16-byte aligned (else EGNN_EALIGN: the host uses
 * the torch operators for such shapes).
 *   egnn_bn_stats_f32     mean[c], biased var[c] over the n rows (training statistics)
 *
 * Every other entry point of this family takes its BatchNorm operands as one descriptor, egnn_bn_act_t.  The call reads
 * it only while it runs and never keeps the pointer (kernel arguments are copied at launch: the descriptor may live on the
 * caller's stack, also while a hipGraph is captured).  bn == NULL is EGNN_EINVAL.
 *   y = drop_p(relu?(gamma * (x - mean) * rsqrt(var + eps) + beta)); gamma / beta nullable (1 / 0); the dropout mask is a
 *   counter-based hash of (seed + *seed_dev, row*C + c): keep if u >= p, kept values scaled 1/(1-p); seed_dev: nullable
 *   device scalar added to `seed` -- a per-step value that lives on the device, so that a captured hipGraph of the step
 *   draws a fresh mask on every replay.
 *   pick == NULL: every row of x is an output row.  pick != NULL: only the OUTPUT ROWS pick (n_pick unique ids into the n rows
 *   of x) are formed / carry a gradient -- the projection heads feeding the sampled criteria (/root/reference/arxiv_pyg/
 *   gnn.py:296-306 -> criterion.py:62-65,134-137: the statistics span all train rows, the criterion keeps max_samples of the
 *   output rows).  y / dy then have n_pick rows, y[i] = act(bn(x[pick[i]])); dx always has all n rows (the mean / variance
 *   terms reach every row).  The apply half takes n_pick == 0 (a shard without picked rows; pick still non-NULL, not read);
 *   the other calls need n_pick > 0. */
typedef struct egnn_bn_act {
  const float* x; int64_t ld; int64_t n; int64_t C;   /* x [n, C]: the rows the statistics span */
  const float* mean; const float* var; float eps;
  const float* gamma; const float* beta;
  int relu; float p; uint64_t seed; const uint64_t* seed_dev;
  const int64_t* pick; int64_t n_pick;                 /* NULL / 0: every row; else the unique output rows */
} egnn_bn_act_t;

/*   egnn_bn_act_fwd_f32         y [out rows, C]
 *   egnn_bn_act_bwd_f32         recomputes xhat / ReLU sign / mask from x and seed; dgamma = sum d*xhat, dbeta = sum d [C] over the
 *                               output rows; dx [n,C]; batch_stats != 0: mean/var are this batch's statistics (training backward,
 *                               the -(sum d + xhat sum d xhat)/n terms apply); 0: running statistics (eval-mode graph).
 *                               dx_colsum [C] nullable: the column sums of dx -- the gradient of a bias added in front of the
 *                               BatchNorm (GCNConv / nn.Linear bias, gnn.py:47-48,296-306), formed while dx is written instead of by
 *                               a second pass over it (ATen: gy.sum(0))
 *   egnn_bn_act_bwd_reduce_f32 / _apply_f32   the two halves of egnn_bn_act_bwd_f32, for batch statistics that span several
 *                               GPUs (node-range shards, SURVEY.md 8e: SyncBN semantics): reduce writes this shard's dbeta = sum d and
 *                               dgamma = sum d*xhat; the caller all-reduces them over RCCL and passes the totals plus inv_count =
 *                               1 / (rows of ALL shards) to apply (inv_count = 0: running statistics; the all-rank sums already
 *                               divided by the row total go with inv_count = 1).  With pick and dx_colsum, apply needs local_dbeta
 *                               (this tensor's own sum d: the picked rows' own term is local); otherwise local_dbeta is not read.
 * ws: egnn_bn_ws_floats(C) floats (apply: only with dx_colsum). */
size_t egnn_bn_ws_floats(int64_t C);
int egnn_bn_stats_f32(const float* x, int64_t ld, int64_t n, int64_t C, float* mean, float* var, float* ws, size_t ws_floats,
                      void* stream);
int egnn_bn_act_fwd_f32(const egnn_bn_act_t* bn, float* y, int64_t ldy, void* stream);
int egnn_bn_act_bwd_f32(const egnn_bn_act_t* bn, const float* dy, int64_t ld_dy, int batch_stats, float* dgamma, float* dbeta,
                        float* dx, int64_t ld_dx, float* dx_colsum, float* ws, size_t ws_floats, void* stream);
int egnn_bn_act_bwd_reduce_f32(const egnn_bn_act_t* bn, const float* dy, int64_t ld_dy, float* dgamma, float* dbeta, float* ws,
                               size_t ws_floats, void* stream);
int egnn_bn_act_bwd_apply_f32(const egnn_bn_act_t* bn, const float* dy, int64_t ld_dy, const float* sum_dbeta, const float* sum_dgamma,
                              float inv_count, const float* local_dbeta, float* dx, int64_t ld_dx, float* dx_colsum, float* ws,
                              size_t ws_floats, void* stream);

/* Merge the per-shard statistics of a sharded batch: stats [world, 2C+1] = (mean[C] | biased var[C] | rows) per shard
 * (all-gathered over RCCL), combined in shard order with the pairwise update of Chan et al. (identical on every rank);
 * shards with 0 rows are skipped.  Outputs mean [C], biased var [C], total [1] (rows of all shards). */
int egnn_bn_merge_shards_f32(const float* stats, int world, int64_t C, float* mean, float* var, float* total, void* stream);

/* h = act(bn(x)) [M, C] followed by the narrow Linear  h W  (W [C, Ks] for w_kmajor = 0, [Ks, C] rows for 1; Ks <= 64): the last
 * hidden layer of the students (/root/reference/arxiv_pyg/gnn.py:47-52).  bn->pick must be NULL; M = bn->n, C = bn->C.
 * Forward in one pass over x: h is stored AND multiplied by W while its 16-byte pieces are in registers: xw = h W [M, Ks].  h is
 * bit-identical to egnn_bn_act_fwd_f32.  EGNN_EALIGN when the shape is not taken (C != 256, M * ld >= 2^31): the caller then makes
 * the two calls. */
int egnn_bn_act_linear_fwd_f32(const egnn_bn_act_t* bn, const float* W, int64_t ldw, int w_kmajor, int64_t Ks, float* h, int64_t ldh,
                               float* xw, int64_t ld_xw, void* stream);
/* Backward in one pass over the [M, C] tensors (loss.backward()), in two halves so that node-range shards can all-reduce the column
 * sums between them (SyncBN semantics); C % 64 == 0:
 *   reduce: dh = alpha G W^T (+ addend, nullable dense [M, C]) (+ add_rows[add_inv[row]] where add_inv[row] >= 0: the row-compact input
 *           gradient of the projection head, gnn.py:150; add_inv int32 [M], -1 = no row); d = dh * gate(x) is left in dx (dh is never
 *           stored) and THIS shard's (sum d, sum d xhat) in dbeta / dgamma.  ws: egnn_skinny_dx_bn_ws_floats(M, C) floats.
 *   apply:  turns the stored d into dx = gamma rstd (d - (sum_dbeta + xhat sum_dgamma) inv_count) in place (dx_colsum nullable:
 *           column sums of dx, ws of egnn_bn_ws_floats(C) floats then).  On one GPU: the local sums and inv_count = 1 / M. */
size_t egnn_skinny_dx_bn_ws_floats(int64_t M, int64_t C);
int egnn_skinny_dx_bn_bwd_reduce_f32(const float* G, int64_t ldg, const float* W, int64_t ldw, int w_kmajor, int64_t Ks, float alpha,
                                     const float* addend, int64_t ld_addend, const float* add_rows, int64_t ld_add_rows,
                                     const int32_t* add_inv, const egnn_bn_act_t* bn, float* dgamma, float* dbeta, float* dx,
                                     int64_t ld_dx, float* ws, size_t ws_floats, void* stream);
int egnn_bn_bwd_apply_stored_f32(const egnn_bn_act_t* bn, const float* sum_dbeta, const float* sum_dgamma, float inv_count, float* dx,
                                 int64_t ld_dx, float* dx_colsum, float* ws, size_t ws_floats, void* stream);

/* nn.BatchNorm1d's training-step state update in one launch (torch/nn/modules/batchnorm.py: num_batches_tracked += 1,
 * running = (1 - m) running + m stat with the unbiased variance n/(n-1) var):  mean / var [C] = this batch's statistics,
 * momentum < 0 = cumulative average (momentum=None); num_batches_tracked: nullable device int64. */
int egnn_bn_running_update_f32(const float* mean, const float* var, int64_t C, int64_t n, float momentum, float* running_mean,
                               float* running_var, int64_t* num_batches_tracked, void* stream);
/* The same update with the row count read from device memory (total_rows [1], float): the all-rank row total of a node-range
 * sharded run (SyncBN) never visits the host. */
int egnn_bn_running_update_dev_f32(const float* mean, const float* var, int64_t C, const float* total_rows, float momentum,
                                   float* running_mean, float* running_var, int64_t* num_batches_tracked, void* stream);

/* Eval-mode BatchNorm1d folded into the layer in front of it (model.eval(): y = (x W + b - running_mean) * gamma /
 * sqrt(running_var + eps) + beta, gnn.py:47-49,198-201):  W_out[i,c] = W[i,c] * s_c,  bias_out[c] = (bias[c] - mean[c]) * s_c
 * + beta[c],  s_c = gamma[c] / sqrt(var[c] + eps).  W [rows, C] row-major (GCNConv layout [in, out]); bias / gamma / beta
 * nullable (0 / 1 / 0).  The aggregation is linear, so the fold also holds with A^ between W and the BatchNorm. */
int egnn_bn_fold_f32(const float* W, int64_t ldw, int64_t rows, int64_t C, const float* bias, const float* mean, const float* var,
                     const float* gamma, const float* beta, float eps, float* W_out, int64_t ld_out, float* bias_out, void* stream);

/* test() of /root/reference/arxiv_pyg/gnn.py:198-218 in one pass: acc3[k] = |{i : split_id[i] == k, argmax_c logits[i,c] == y[i]}|
 * / |{i : split_id[i] == k}| for the splits k = 0, 1, 2 (train / valid / test; any other id = not evaluated), as the ogb
 * Evaluator forms it (integer hit count over split size, in double).  argmax = first maximal column (torch.argmax).
 * ws: egnn_split_accuracy_ws_ints() int32. */
size_t egnn_split_accuracy_ws_ints(void);
int egnn_split_accuracy_f32(const float* logits, int64_t ld, int64_t n, int64_t C, const int64_t* y, const int8_t* split_id,
                            double* acc3, int32_t* ws, size_t ws_ints, void* stream);
/* The same pass returning the raw counts: out6 = (hits_train, hits_valid, hits_test, n_train, n_valid, n_test) as doubles -- what
 * one node-range shard contributes to the all-rank accuracies of test() (summed over ranks by an all-reduce). */
int egnn_split_counts_f32(const float* logits, int64_t ld, int64_t n, int64_t C, const int64_t* y, const int8_t* split_id,
                          double* out6, int32_t* ws, size_t ws_ints, void* stream);

/* dst[idx[r], :] += src[r, :], r < n, for UNIQUE ids: the row-compact gradient of x[idx] joins the dense gradient of x
 * (the backward of gnn.py:150 `feat[train_idx]` next to the conv's gradient) without a zero-filled [N,C] temporary. */
int egnn_rows_add_f32(float* dst, int64_t ld_dst, const int64_t* idx, const float* src, int64_t ld_src, int64_t n, int64_t C,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row gathers whose ids may REPEAT (csrc/rows_sum.hip): the backward of x[idx] as torch defines it -- every entry's gradient row is
 * added into its row -- without float atomics, in a fixed order.  A plan is built once per index tensor; the sum runs per step.
 *
 * egnn_rows_plan_build_i64   idx int64 [S].  An entry in [-n_rows, 0) is wrapped (+ n_rows), as torch does; an entry outside
 *     [-n_rows, n_rows) gets no key (the all-ones key, which sorts last) and is counted.  keys_sorted uint64 [S] (8-byte aligned):
 *     key = (row << shift) | position with shift = number of bits of S - 1 (at least 1), radix-sorted (hipCUB) over the bits in
 *     use: a row's positions form one run, ascending.  counters int32 [4], written by the call (the caller zeroes nothing):
 *       [0] entries out of range, [1] keyed entries that are not the head of their run (0: the ids are unique),
 *       [2] entries that were negative and wrapped, [3] the longest run.
 *     S and n_rows < 2^31 - 1 (else EGNN_EINVAL).  S == 0 enqueues nothing and writes nothing (all pointers may be NULL).
 *     ws: egnn_rows_plan_ws_bytes(S, n_rows) bytes, 16-byte aligned (one key array and the sort's temporary storage; sized by
 *     hipCUB from the current device, see egnn_adam_rows_step_sum_ws_bytes); missing or short: EGNN_EWORKSPACE, misaligned:
 *     EGNN_EALIGN.  Every check happens before the first launch.
 *
 * egnn_rows_add_runs_f32     dst[r, :] = (accumulate ? dst[r, :] : 0) + sum of src[p, :] over the positions p of row r's run,
 *     r < n_rows; dst [n_rows, ld_dst], src [S, ld_src], C columns, shift as above (anything else: EGNN_EINVAL).  A row that no key
 *     names keeps its value when accumulate == 1 and is ZEROED when accumulate == 0 (dst may be uninitialised: no memset needed).
 *     ORDER OF THE ADDITIONS, a function of (idx, C) only -- never of the launch geometry, so two calls are bit-equal: with
 *     p1 < p2 < ... < pk the positions of row r and K = EGNN_ROWS_SUM_CHUNK, the run is cut from its head into chunks of K
 *     positions (the last one may be shorter); chunk j gives  P_j = ((src[p_(jK+1)] + src[p_(jK+2)]) + ...)  in ascending
 *     position, the row gets  T = ((P_0 + P_1) + ...)  in ascending chunk order, and  dst[r] = accumulate ? dst[r] + T : T.
 *     k <= K: T = P_0.  With unique ids the result therefore equals egnn_rows_add_f32 into the same dst (accumulate == 1) and
 *     index_copy_ into zeros (accumulate == 0) bit for bit.  No float atomics.
 *     One lane group per chunk (min(64, pow2ceil(C / 4)) lanes, 16 bytes per lane) when C % 4 == 0, both pitches % 4 == 0 and
 *     both matrices are 16-byte aligned; a scalar path in the same entry point otherwise (any C, any pitch).  The chunks of a run
 *     longer than K are summed by different lane groups and meet in ws: egnn_rows_add_runs_ws_bytes(S, C) bytes, 16-byte aligned
 *     (0 for S <= K: ws may be NULL); missing or short: EGNN_EWORKSPACE, misaligned: EGNN_EALIGN; all checks before any launch.
 *     S == 0: EGNN_OK; with accumulate == 0 and a non-NULL dst the n_rows rows are zeroed.
 *     A position or row that does not fit S / n_rows (keys built for other operands) is skipped, never used as an address.
 *
 * EGNN_ROWS_SUM_CHUNK = 128.  A lane group is at most one wave and streams a chunk's rows one after the other (four in flight), so
 * the chunk length is the longest serial chain of row reads in the kernel: 128 KiB per wave at C = 256.  Edge endpoints name a hub
 * thousands of times (ogbn-arxiv: a maximum degree of about 13 000) next to a median of a few; uncut, that one wave would still be reading when the
 * other resident waves (up to 256 CUs x 32) have long finished.  At 128 the hub is spread over ~100 waves, every
 * run of the common degrees stays in one piece, the partial rows are at most 1/64 of the bytes of src, and the serial second pass
 * adds ~100 rows for the largest hub.  Chosen by this count, not tuned by measurement.
 * ---------------------------------------------------------------------------------------------- */
#define EGNN_ROWS_SUM_CHUNK 128
size_t egnn_rows_plan_ws_bytes(int64_t S, int64_t n_rows);
int egnn_rows_plan_build_i64(const int64_t* idx, int64_t S, int64_t n_rows, uint64_t* keys_sorted, int32_t* counters, void* ws,
                             size_t ws_bytes, void* stream);
size_t egnn_rows_add_runs_ws_bytes(int64_t S, int64_t C);
int egnn_rows_add_runs_f32(float* dst, int64_t ld_dst, int64_t n_rows, const uint64_t* keys_sorted, int64_t S, int shift,
                           const float* src, int64_t ld_src, int64_t C, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Aggregation by an UNSORTED index (csrc/scatter.hip): out[r, :] = reduce of src[p, :] over the positions p with index[p] == r --
 * torch_scatter.scatter along dim 0, the aggregation step of a user-defined message-passing layer (nn.MessagePassing) -- and its
 * backward.  No float atomics, no integer atomics.
 *
 * egnn_scatter_runs_f32   walks the sorted (row, position) keys of egnn_rows_plan_build_i64 (keys_sorted, S, shift as there).
 *     src [S, ld_src], out [n_rows, ld_out], C columns; reduce: 0 sum, 1 mean, 2 max, 3 min (anything else: EGNN_EINVAL).  EVERY row
 *     of out is written (out may be uninitialised: no memset needed).
 *     count int32 [n_rows] (nullable; required for mean, else EGNN_EINVAL): the length of row r's run.
 *     arg int64 [n_rows, C] contiguous (nullable; max / min only, else EGNN_EINVAL).
 *     sum:  bit-equal to egnn_rows_add_runs_f32(accumulate = 0) on the same keys -- the same code runs -- so the order of the
 *           additions is the one documented there, a function of (index, C) only.
 *     mean: that sum divided by (float)count[r], one correctly rounded division per element; a row that no key names is 0.
 *     max / min: exact.  arg[r, c] is the SMALLEST position p attaining the extreme of column c (ties are decided by edge order); a
 *           row that no key names gets the value 0 and arg = S (torch_scatter's convention).  A run longer than
 *           EGNN_ROWS_SUM_CHUNK is cut like the run-sum's, its chunks are folded by different lane groups into (value, position)
 *           pairs in ws, and a second launch merges the pairs in ascending chunk order; a pair is replaced only by a strictly
 *           better value, and where a chunk starts is read off the keys, so the result does not depend on the launch geometry.
 *           NaN inputs: unspecified (a NaN never compares better, so what a column holding one returns depends on its position).
 *     Lane groups as in the run-sum: 16 bytes per lane when C % 4 == 0, both pitches % 4 == 0 and out and src are 16-byte aligned;
 *     a scalar path in the same entry point otherwise (any C, any pitch).
 *     ws: egnn_scatter_runs_ws_bytes(S, C, reduce) bytes, 16-byte aligned (0 for S <= EGNN_ROWS_SUM_CHUNK: ws may be NULL); missing
 *     or short: EGNN_EWORKSPACE, misaligned ws / keys / count / arg: EGNN_EALIGN.  Every check happens before the first launch.
 *     S == 0: EGNN_OK; with a non-NULL out the n_rows rows and counts are zeroed and arg is filled with S = 0.
 *     A position or row that does not fit S / n_rows (keys built for other operands) is skipped, never used as an address.
 *
 * egnn_scatter_bwd_f32    the backward in gather form: ONE pass over dsrc [S, ld_dsrc]; every element is written with a plain store (no
 *     zero-fill needed, no atomics).  index int64 [S] holds row ids already wrapped; r = index[p] outside [0, n_rows) writes a zero
 *     row and reads nothing.  g [n_rows, ld_g].
 *       sum:  dsrc[p, c] = g[r, c];   mean: g[r, c] / (float)count[r];   max / min: arg[r, c] == p ? g[r, c] : 0
 *     with count / arg as the forward wrote them (required for mean / max, min; else EGNN_EINVAL).  S == 0: EGNN_OK.
 *
 * egnn_rows_wrap_i64      wrapped[p] = idx[p] (+ n_rows when negative), or -1 when idx[p] is outside [-n_rows, n_rows): the row ids of
 *     a plan whose range check is left to the device (no host read), in the form egnn_scatter_bwd_f32 takes.  S == 0: EGNN_OK.
 * ---------------------------------------------------------------------------------------------- */
int egnn_rows_wrap_i64(const int64_t* idx, int64_t S, int64_t n_rows, int64_t* wrapped, void* stream);
size_t egnn_scatter_runs_ws_bytes(int64_t S, int64_t C, int reduce);
int egnn_scatter_runs_f32(float* out, int64_t ld_out, int64_t n_rows, int32_t* count, int64_t* arg, const uint64_t* keys_sorted,
                          int64_t S, int shift, const float* src, int64_t ld_src, int64_t C, int reduce, void* ws, size_t ws_bytes,
                          void* stream);
int egnn_scatter_bwd_f32(float* dsrc, int64_t ld_dsrc, int64_t S, const int64_t* index, int64_t n_rows, const float* g, int64_t ld_g,
                         int64_t C, int reduce, const int32_t* count, const int64_t* arg, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Softmax over the groups of an UNSORTED index (csrc/scatter_softmax.hip): torch_scatter.scatter_softmax / scatter_log_softmax along
 * dim 0 and torch_geometric.utils.softmax on multi-head scores [E, H] -- the step between the lift and the aggregation of an attention
 * conv -- and its backward.  No float atomics, no integer atomics; first derivatives only.
 *
 * Operands of both calls: keys_sorted, S, shift as egnn_rows_plan_build_i64 produced them; rows int64 [S], the row ids already
 * wrapped, -1 (anything outside [0, n_rows)) for a dropped id -- the form egnn_scatter_bwd_f32 takes; C >= 1 columns (the flattened
 * trailing shape: usually the head count); form: 0 softmax, 1 log-softmax (anything else: EGNN_EINVAL).
 *
 * egnn_scatter_softmax_fwd_f32   src [S, ld_src], out [S, ld_out].  With r = rows[p] and the max and the sum over the positions q of
 *     row r's run,  M[r, c] = max_q src[q, c],  Z[r, c] = sum_q exp(src[q, c] - M[r, c]):
 *       form 0:  out[p, c] = exp(src[p, c] - M[r, c]) / (Z[r, c] + eps)        one true division per element
 *       form 1:  out[p, c] = (src[p, c] - M[r, c]) - log(Z[r, c] + eps)
 *     (PyG passes eps = 1e-16, torch_scatter 0).  A run walk leaves M and Z in row_max / row_den, float [n_rows, C] contiguous, which
 *     the caller provides and need not initialise: EVERY row is written, a row that no key names gets 0 in both.  A gather over
 *     [S, C] then writes EVERY element of out with a plain store; a position with rows[p] outside [0, n_rows) gets 0 in both forms.
 *     ORDER OF THE ADDITIONS, per column, a function of (index, C) only: a run is cut from its head into chunks of
 *     K = EGNN_ROWS_SUM_CHUNK positions exactly as egnn_rows_add_runs_f32 cuts it (read off the keys, never off the launch
 *     geometry).  Chunk j yields m_j (its exact maximum) and z_j = sum of e_o = exp(src - m_j) over its offsets o = 0 .. K - 1 in
 *     this order: for l = 0 .. 15,  s_l = ((e_l + e_(l+16)) + e_(l+32)) + ... + e_(l+112)  (offsets past the chunk's end left out, an
 *     empty s_l is 0), then
 *       z_j = (((s_0 + s_8) + (s_4 + s_12)) + ((s_2 + s_10) + (s_6 + s_14))) + (((s_1 + s_9) + (s_5 + s_13)) + ((s_3 + s_11) + (s_7 + s_15))).
 *     A run of one chunk: M = m_0, Z = z_0.  A longer run parks its pairs in ws and a second launch merges them in ascending chunk
 *     order:  M = max_j m_j,  Z = ((z_0 exp(m_0 - M) + z_1 exp(m_1 - M)) + ...).  The bits of out are therefore a function of
 *     (index, C, values, eps, form) only -- not of a pitch, an alignment or the addressing path (16 bytes per lane when C % 4 == 0,
 *     all pitches % 4 == 0 and all float operands are 16-byte aligned; a scalar path in the same entry point otherwise) -- two calls
 *     are bit-equal, and column c of a [S, C] call equals the [S, 1] call on that column bit for bit.
 *     Lanes run along positions: one 16-lane group per chunk, lane l reading the chunk's offsets l, l + 16, ... (csrc/scatter_softmax.hip).
 *     UNSPECIFIED: NaN, +inf, and a run whose values are all -inf.
 *
 * egnn_scatter_softmax_bwd_f32   out as the forward wrote it, g the gradient of out, dsrc [S, ld_dsrc].  One more run walk, with the
 *     same cut and the same order of additions, leaves row_dot float [n_rows, C] contiguous (every row written, 0 for a row that
 *     no key names), and a gather writes EVERY element of dsrc (0 for a dropped position):
 *       form 0:  row_dot[r, c] = sum_q out[q, c] * g[q, c]  (products formed in registers),  dsrc[p, c] = out[p, c] * (g[p, c] - row_dot[r, c])
 *       form 1:  row_dot[r, c] = sum_q g[q, c],                                              dsrc[p, c] = g[p, c] - exp(out[p, c]) * row_dot[r, c]
 *
 * Both: S and n_rows < 2^31 - 1, C >= 1, every pitch >= C, shift = the number of bits of S - 1 (at least 1), form 0 | 1, no NULL
 *     operand (else EGNN_EINVAL).  ws: egnn_scatter_softmax_ws_bytes(S, C) bytes, 16-byte aligned (0 for S <= EGNN_ROWS_SUM_CHUNK: ws
 *     may be NULL); missing or short: EGNN_EWORKSPACE; misaligned ws / keys / rows / float operands: EGNN_EALIGN.  Every check happens
 *     before the first launch.  S == 0: EGNN_OK; the per-row buffers are zero-filled when they are non-NULL (everything else may be NULL).
 *     A key whose position or row does not fit S / n_rows (keys built for other operands) is skipped, never used as an address.
 * ---------------------------------------------------------------------------------------------- */
size_t egnn_scatter_softmax_ws_bytes(int64_t S, int64_t C);
int egnn_scatter_softmax_fwd_f32(float* out, int64_t ld_out, float* row_max, float* row_den, int64_t n_rows, const uint64_t* keys_sorted,
                                 int64_t S, int shift, const int64_t* rows, const float* src, int64_t ld_src, int64_t C, float eps, int form,
                                 void* ws, size_t ws_bytes, void* stream);
int egnn_scatter_softmax_bwd_f32(float* dsrc, int64_t ld_dsrc, float* row_dot, int64_t n_rows, const uint64_t* keys_sorted, int64_t S,
                                 int shift, const int64_t* rows, const float* out, int64_t ld_out, const float* g, int64_t ld_g, int64_t C,
                                 int form, void* ws, size_t ws_bytes, void* stream);

/* FitNet (/root/reference/arxiv_pyg/criterion.py:24-36, ppi_pyg/criterion.py:21-33): loss[0] = mean over n * D of
 * (F.normalize(f) - F.normalize(t))^2, F.normalize(x) = x / max(||x||_2, eps); one wave per row, fixed-order sums.
 * bwd: df / dt (nullable) = g[0] * dloss/df, dloss/dt.  ws: egnn_feature_loss_ws_floats(n) floats. */
size_t egnn_feature_loss_ws_floats(int64_t n);
int egnn_fitnet_fwd_f32(const float* f, int64_t ldf, const float* t, int64_t ldt, int64_t n, int64_t D, float eps, float* loss,
                        float* ws, size_t ws_floats, void* stream);
int egnn_fitnet_bwd_f32(const float* f, int64_t ldf, const float* t, int64_t ldt, int64_t n, int64_t D, float eps, const float* g,
                        float* df, int64_t lddf, float* dt, int64_t lddt, void* stream);

/* Attention transfer (criterion.py:39-54): e_s[i] = sum_d f[i,d]^2 over Df columns, e_t likewise over Dt; both length-n vectors are
 * L2-normalised ACROSS the n nodes (the reference's F.normalize on a 1-D tensor) and loss[0] = mean_i (e_s[i]/|e_s| - e_t[i]/|e_t|)^2.
 * The forward leaves e_s, e_t and its scalars in ws (same size as above); the backward reads them: keep ws until then. */
int egnn_at_fwd_f32(const float* f, int64_t ldf, int64_t Df, const float* t, int64_t ldt, int64_t Dt, int64_t n, float eps, float* loss,
                    float* ws, size_t ws_floats, void* stream);
int egnn_at_bwd_f32(const float* f, int64_t ldf, int64_t Df, const float* t, int64_t ldt, int64_t Dt, int64_t n, float eps, const float* ws,
                    const float* g, float* df, int64_t lddf, float* dt, int64_t lddt, void* stream);

/* Attention transfer on node-range shards: the same loss cut where the ranks' sums meet.  Each rank holds n of the n_global rows; the
 * host sums two device arrays over the ranks in between (nothing passes through host memory):
 *   energy  : es[i] = sum_d f^2, et[i] = sum_d t^2 for the rank's rows; sumsq = {sum es^2, sum et^2} of the rank          -> all-reduce sumsq
 *   partial : ns = max(sqrt(sumsq_global[0]), eps), nt likewise; d_i = es[i]/ns - et[i]/nt;
 *             sums = {sum d^2, sum d es, sum d et} of the rank; scal = {ns, nt, raw |e_s|, raw |e_t|} (4 floats)        -> all-reduce sums
 *   bwd_rows: df / dt (nullable) of the rank's rows for loss = sums_global[0] / n_global, upstream gradient g[0].
 * ws (energy, partial): egnn_feature_loss_ws_floats(n) floats, free again after the call.  Fixed-order sums, no atomics. */
int egnn_at_energy_f32(const float* f, int64_t ldf, int64_t Df, const float* t, int64_t ldt, int64_t Dt, int64_t n, float* es, float* et,
                       float* sumsq, float* ws, size_t ws_floats, void* stream);
int egnn_at_partial_f32(const float* es, const float* et, int64_t n, const float* sumsq_global, float eps, float* scal, float* sums,
                        float* ws, size_t ws_floats, void* stream);
int egnn_at_bwd_rows_f32(const float* f, int64_t ldf, int64_t Df, const float* t, int64_t ldt, int64_t Dt, int64_t n, int64_t n_global,
                         const float* es, const float* et, const float* scal, const float* sums_global, float eps, const float* g,
                         float* df, int64_t lddf, float* dt, int64_t lddt, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GraphSAINT random-walk mini-batches formed on the device (csrc/saint.hip).
 *
 * Replaces torch_geometric.data.GraphSAINTRandomWalkSampler, /root/reference/mag_pyg/gnn.py:361-366, i.e.
 * torch_sparse::random_walk + SparseTensor.saint_subgraph + the attribute gathers of its collate step (CPU C++ inside
 * DataLoader workers there, iterated by train() at :187-190), and the per-relation structure RGCNConv needs per batch (:25-68).
 * Integer work, no atomics, every output written with plain stores; node ids and row counts must be below 2^31.
 *
 * egnn_saint_random_walk_i64   B walks of L >= 1 steps over the CSR (rowptr [N+1], col [nnz]).  Step rule of
 *     torch_sparse::random_walk: from node n with d = rowptr[n+1] - rowptr[n] entries stay at n when d == 0, else go to
 *     col[rowptr[n] + min(int64(u * d), d - 1)], the product formed in fp32.  walks [B, L+1] (nullable) receives the nodes;
 *     flag [N] (uint8, zeroed by the caller) gets 1 at every visited node.
 *     Draws: INJECTED when start [B] (int64, ids outside [0, N) are clamped into it) and rand [B, L] (fp32 in [0, 1)) are given;
 *     OWN when both are NULL (one without the other is EGNN_EINVAL): with key = seed + *seed_dev (seed_dev nullable: 0) and
 *     h(key, c) the two-round 32-bit counter hash of the dropout kernels (csrc/bn_common.h hash32 / uniform01), walk b uses the
 *     counters c = b * (L + 1) + j:  j = 0: start = (h * N) >> 32 (64-bit product of the 32-bit hash; no float involved);
 *     j = 1 .. L: u of step j = (h >> 8) * 2^-24.
 * egnn_saint_select_i64        relabel [N+1] = exclusive scan of flag (relabel[N] = number of flagged nodes = n_sub) and
 *     node_idx[relabel[i]] = i for every flagged i: the ascending list walks.view(-1).unique().  node_idx holds node_cap >= n_sub
 *     ids (B * (L + 1) always suffices).  ws: egnn_saint_scan_ws_bytes(N) bytes.
 * egnn_saint_induced_count_i64 / _fill_i64   the sub-matrix of a parent CSR (rowptr, col [, val]) on flagged rows and columns.
 *     Output row r = g * n_map + i, g < groups, i < n_map, stands for parent row g * group_stride + row_map[i]; rows with
 *     i >= *n_map_dev (nullable: all n_map rows) are empty, so the caller may size n_map by an upper bound before n_sub is known
 *     on the host.  groups = 1: SparseTensor.saint_subgraph(node_idx); groups = T over a parent of T * N rows sorted by
 *     (edge type, destination, source): the per-relation CSRs of the batch.  N = number of columns = length of flag / relabel.
 *     count: counts [groups * n_map] = flagged entries per output row, out_ptr [groups * n_map + 1] = their exclusive scan
 *            (ws: egnn_saint_scan_ws_bytes(groups * n_map) bytes);
 *     fill:  for the kept entries of output row r, IN THE PARENT'S ORDER, at out_ptr[r] ...: out_row (nullable) = i,
 *            out_col = relabel[col], out_val (nullable) = val[entry] (val nullable: the entry's position in the parent).
 *            Positions >= out_cap are not written.  flag must be the one the counts were taken with.
 *     A wave compacts egnn_saint_induced_geometry(0) entries per pass (ballot + popcount prefix); rows with more than
 *     egnn_saint_induced_geometry(2) entries are compacted by one workgroup, egnn_saint_induced_geometry(1) entries per pass;
 *     both carry the row's running offset from pass to pass.
 * egnn_saint_gather_i64        o_*[i] = *[node_idx[i]], i < n_sub, for node_type / local_idx / y (int64) and train_mask (uint8),
 *     each nullable; o_edge_attr[e] = edge_attr[edge_idx[e]], e < e_sub (edge_attr nullable).
 * ---------------------------------------------------------------------------------------------- */
int64_t egnn_saint_induced_geometry(int which);
int egnn_saint_random_walk_i64(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, int64_t B, int64_t L,
                               const int64_t* start, const float* rand, uint64_t seed, const uint64_t* seed_dev, int64_t* walks,
                               uint8_t* flag, void* stream);
size_t egnn_saint_scan_ws_bytes(int64_t items);
int egnn_saint_select_i64(const uint8_t* flag, int64_t N, int64_t* relabel, int64_t* node_idx, int64_t node_cap, void* ws,
                          size_t ws_bytes, void* stream);
int egnn_saint_induced_count_i64(const int64_t* rowptr, const int64_t* col, const int64_t* row_map, int64_t n_map,
                                 const int64_t* n_map_dev, int64_t groups, int64_t group_stride, int64_t N, const uint8_t* flag,
                                 int64_t* counts, int64_t* out_ptr, void* ws, size_t ws_bytes, void* stream);
int egnn_saint_induced_fill_i64(const int64_t* rowptr, const int64_t* col, const int64_t* val, const int64_t* row_map, int64_t n_map,
                                const int64_t* n_map_dev, int64_t groups, int64_t group_stride, int64_t N, const uint8_t* flag,
                                const int64_t* relabel, const int64_t* out_ptr, int64_t out_cap, int64_t* out_row, int64_t* out_col,
                                int64_t* out_val, void* stream);
int egnn_saint_gather_i64(const int64_t* node_idx, int64_t n_sub, const int64_t* node_type, const int64_t* local_idx, const int64_t* y,
                          const uint8_t* train_mask, int64_t* o_node_type, int64_t* o_local_idx, int64_t* o_y, uint8_t* o_train_mask,
                          const int64_t* edge_idx, int64_t e_sub, const int64_t* edge_attr, int64_t* o_edge_attr, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SIGN student (/root/reference/arxiv_dgl/sign.py:105-162): Linear -> PReLU -> dropout with a learnable scalar slope, replicated
 * over the R + 1 hops and concatenated; csrc/sign.hip.  Each entry point is ONE launch for all hops (the backward adds a
 * fixed-order finalize launch); deterministic, no float atomics.
 * "Segment" h = the columns [h*Cs, (h+1)*Cs) of a row-major [B, H*Cs] matrix with leading dimension ld >= H*Cs; H <= 16
 * (more: EGNN_EINVAL, no launch).  The operands travel as ONE descriptor, egnn_sign_seg_t, read only while the call runs (it
 * may live on the caller's stack).  seed, slope, src and ld_src are HOST arrays of H entries: the entry point copies them into
 * the kernel arguments (no device allocation, no host-to-device copy besides the kernel arguments), so the pointers in `slope`
 * are read by the kernel on every launch -- slopes are parameters, nothing is baked in.
 *   dropout: the convention of the fused BatchNorm above; the uniform of element (r, c) of segment h is a counter hash of
 *   (seed[h] + *seed_dev, r * Cs + (c - h*Cs)), keep where u >= p, kept values scaled 1 / (1 - p); seed_dev nullable (0).
 *   p == 0: no mask (seed may be NULL).  Masks are recomputed by the backward, never stored.
 * 16-byte vector path when Cs % 4 == 0, every ld % 4 == 0 and every matrix pointer is 16-byte aligned; a scalar path in the
 * same entry point otherwise (any Cs, any ld).
 *   egnn_sign_gather_drop_f32   out[i, h*Cs + c] = drop_h(src[h][batch[i], c]), i < B: the `[x[batch] for x in feats]` gather,
 *                               `input_drop` and the operand of the first Linear of every hop (sign.py:236,308 and :151) in one
 *                               pass; src[h] [n_src, ld_src[h] >= Cs]; batch int64 [B] with ids in [0, n_src); no backward (the hop
 *                               features are constants).  Reads src, ld_src, n_src, batch; slope is not read.
 *   egnn_prelu_drop_fwd_f32     y = drop(prelu(z, *slope[h])), prelu(z, a) = z > 0 ? z : a*z: `self.dropout(self.prelu(x))` of
 *                               sign.py:132 for all hops of one level, and :155 over the concatenation.  p == 0: eval mode.
 *   egnn_prelu_drop_bwd_f32     from z, dy and the same seeds, one pass:  dz = dy * m * (z > 0 ? 1 : a_h);
 *                               da [H]: da[h] = sum over segment h of dy * m * (z > 0 ? 0 : z)  (the PReLU weight gradient);
 *                               dbias [H*Cs]: dbias[c] = sum_r dz[r, c]  (the bias gradient of the nn.Linear that formed z,
 *                               sign.py:130 -- ATen: a second pass, dz.sum(0)).  B >= 1.
 *                               ws: egnn_prelu_drop_ws_floats(B, Cs, H) floats (else EGNN_EWORKSPACE).
 * ---------------------------------------------------------------------------------------------- */
typedef struct egnn_sign_seg {
  int64_t B; int64_t Cs; int H;                          /* B rows, H segments of Cs columns */
  float p; const uint64_t* seed; const uint64_t* seed_dev;   /* seed: host [H]; seed_dev: device scalar, nullable */
  const float* const* slope;                             /* prelu: host [H] of device pointers to the scalar slopes */
  const float* const* src; const int64_t* ld_src; int64_t n_src;   /* gather: host [H] source matrices [n_src, ld_src[h]] */
  const int64_t* batch;                                  /* gather: device int64 [B] row ids */
} egnn_sign_seg_t;
int egnn_sign_gather_drop_f32(const egnn_sign_seg_t* seg, float* out, int64_t ld_out, void* stream);
int egnn_prelu_drop_fwd_f32(const egnn_sign_seg_t* seg, const float* z, int64_t ld_z, float* y, int64_t ld_y, void* stream);
size_t egnn_prelu_drop_ws_floats(int64_t B, int64_t Cs, int H);
int egnn_prelu_drop_bwd_f32(const egnn_sign_seg_t* seg, const float* z, int64_t ld_z, const float* dy, int64_t ld_dy, float* dz,
                            int64_t ld_dz, float* da, float* dbias, float* ws, size_t ws_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Structure-preservation metrics, arxiv_pyg/correlation.py (csrc/similarity.hip)
 * ---------------------------------------------------------------------------------------------- */
/* All-pairs Pearson moments behind the global structural correlation (Mantel), correlation.py:178-181, 205-208, 212: for the N unit
 * rows of xs [N,Ps] and xt [N,Pt] (the caller normalises, as for GSP cosine) and every unordered pair i < j, with
 * a = <xs_i, xs_j>, b = <xt_i, xt_j>:
 *   out6 = (n, sum a, sum b, sum a^2, sum b^2, sum ab)   in float64, n = N (N-1) / 2.
 * The reference correlates the cosine DISTANCES 1 - a, 1 - b; Pearson r is invariant under a -> 1 - a on both sides, so the
 * similarities are accumulated.  Neither N x N matrix is formed: only the T (T+1) / 2 upper 128 x 128 tiles are computed, each lane
 * sums its accumulator entries in fp32 ABOUT THE TILE'S MEAN (the tile's raw moments are restored in float64, so a narrow band of
 * cosines far from 0 costs no digits), everything after that is float64 in a fixed order (per-tile partials in ws, one finalising
 * launch, no atomics: two calls are bit-equal).  N < 2 or ld < P: EGNN_EINVAL; ws (8-byte aligned) shorter than
 * egnn_pair_moments_ws_bytes(N): EGNN_EWORKSPACE. */
size_t egnn_pair_moments_ws_bytes(int64_t N);
int egnn_pair_moments_f32(const float* xs, int64_t ld_s, int64_t Ps, const float* xt, int64_t ld_t, int64_t Pt, int64_t N,
                          double* out6, void* ws, size_t ws_bytes, void* stream);
/* The same six float64 moments of two length-n vectors (the per-edge cosines of the local structural correlation,
 * correlation.py:182, 209, 213); fixed order, two launches.  ws: egnn_pearson_moments_ws_bytes(n) bytes. */
size_t egnn_pearson_moments_ws_bytes(int64_t n);
int egnn_pearson_moments_f32(const float* a, const float* b, int64_t n, double* out6, void* ws, size_t ws_bytes, void* stream);

/* Kernel (RBF) CKA, correlation.py:41-53 (rbf, kernel_HSIC) and :70-75 (kernel_CKA), without an N x N object.
 * Device distance, one definition for every pass: d_ij = max(n_i + n_j - 2 g_ij, +0) in fp32, g_ij from the fp32 MFMA, n_i = |x_i|^2.
 *
 * Median bandwidth (correlation.py:45-46): out2 = (median of d_ij over the N (N-1) / 2 pairs i < j, that pair count), float64; the
 * mean of the two middle order statistics when the count is even.  Every pair is kept, coincident rows (d = 0) included; the
 * reference's KX[KX != 0] over the symmetric matrix is the same number whenever no two rows coincide.  Exact: a radix select over the
 * 31 value bits in three histogram passes that recompute the Gram tiles; 64-bit integer counts (order-independent), the bin and the
 * residual rank are chosen on the device between the passes.  N < 2 or ld < P: EGNN_EINVAL; ws (8-byte aligned) shorter than
 * egnn_sqdist_median_ws_bytes(N): EGNN_EWORKSPACE; out2 8-byte aligned. */
size_t egnn_sqdist_median_ws_bytes(int64_t N);
int egnn_sqdist_median_f32(const float* x, int64_t ld, int64_t P, int64_t N, double* out2, void* ws, size_t ws_bytes, void* stream);
/* The three sums of kernel_CKA (correlation.py:52-53, 70-75) for K_ij = exp(-d_ij / (2 sigma2_dev[0])) over xs [N,Ps] and
 * L_ij = exp(-d_ij / (2 sigma2_dev[1])) over xt [N,Pt], K_ii = L_ii = 1 exactly:
 *   out3 = (sum Kc Lc, sum Kc^2, sum Lc^2) over all N^2 entries, Kc_ij = K_ij - rowmean_i - rowmean_j + mean   (= centering(K), :30-37),
 * CKA = out3[0] / sqrt(out3[1] out3[2]).  sigma2_dev: two float64 SQUARED bandwidths in device memory (the medians above can feed it
 * without a host read); one that is not > 0 makes out3 NaN.  Row sums over the full matrix in float64 (workspace O(N), fixed order),
 * entries centred before the products, per-tile partials and one finalising launch: no atomics, two calls are bit-equal.
 * Errors as for egnn_pair_moments_f32; ws: egnn_rbf_cka_ws_bytes(N) bytes; sigma2_dev and out3 8-byte aligned. */
size_t egnn_rbf_cka_ws_bytes(int64_t N);
int egnn_rbf_cka_f32(const float* xs, int64_t ld_s, int64_t Ps, const float* xt, int64_t ld_t, int64_t Pt, int64_t N,
                     const double* sigma2_dev, double* out3, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MAG embedding tables (the reference's mag_pyg/gnn.py:100-108,117-127,424): the one-launch group_input gather and a row-lazy Adam
 * that gives dense torch.optim.Adam's parameters while touching only the rows of the batch; csrc/adam_rows.hip.
 *
 * egnn_group_input_f32   h[i, :] = tables[node_type[i]][local_idx[i], :], i < n, in ONE launch (no mask, no nonzero, no host read).
 *     tables / table_rows are HOST arrays of n_types <= 8 entries (device pointers of contiguous [table_rows[k], D] fp32 matrices and
 *     their row counts), copied into the kernel arguments.  A NULL table writes zeros for its type (the mask form of :117-127 leaves
 *     such rows zero too); a type outside [0, n_types) or an index outside its table writes zeros and adds 1 to *oob (device int32
 *     the caller zeroes and reads when it reads anything else).  D % 4 == 0; h and every table 16-byte aligned, ldh % 4 == 0
 *     (else EGNN_EALIGN).
 *
 * Row-lazy Adam.  Per table: p, m, v [n_rows, ld] and last [n_rows] int32, the step each row is current for; -1 = the row never had
 * a gradient (m = v = 0: dense Adam does not move it).  One step of one element, in torch.optim.Adam's single-tensor order:
 *     m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;  p -= step_size[tau] (m / (sqrtf(v) / bc2_sqrt[tau] + eps))
 * A row outside the batch of step tau takes that step with g = 0 -- later, in registers, when it is next read or stepped (the same
 * device function: deferring a zero-gradient step changes no bit).  step_size[tau % MAX_LAG] = lr_tau / (1 - beta1^tau) and
 * bc2_sqrt[tau % MAX_LAG] = sqrt(1 - beta2^tau) are formed by the host in double, as are 1 - beta1 and 1 - beta2: the rings hold the
 * last EGNN_ADAM_MAX_LAG steps, so no row may lag further behind than that: the caller flushes in time and states in `flushed` the
 * last step every touched row was brought up to; step - flushed > EGNN_ADAM_MAX_LAG is EGNN_EINVAL (nothing enqueued).
 * The descriptor is read only while a call runs (it is copied into the kernel arguments).
 *   egnn_adam_rows_catchup_f32  for every batch row i < n with node_type[i] == type_id (all i when node_type == NULL), table row
 *       r = local_idx[i]: replay tau = last[r] + 1 .. step with g = 0, then last[r] = step.  Rows with last[r] == -1 or == step cost
 *       one 4-byte read.  A table row named more than once is served once (claimed by compare-and-swap on last[r]); ids outside
 *       [0, n_rows) are skipped.
 *   egnn_adam_rows_flush_f32    the same over all n_rows.
 *   egnn_adam_rows_step_f32     step >= 1; claims r with a compare-and-swap step - 1 -> step on last[r] (-1 -> step for a row's first
 *       gradient) and applies the step above with g = g[i, :] ([n, ldg], 16-byte aligned, ldg % 4 == 0).  The row must be current for
 *       step - 1 (catch-up first).  A batch row that loses the claim -- a table row named twice in one batch, a row that is not
 *       current, an id outside the table -- adds 1 to *dup_count and writes nothing; the other rows are unaffected.
 * D % 4 == 0, ld % 4 == 0 and p, m, v 16-byte aligned (else EGNN_EALIGN).  No float atomics: results are bit-stable.
 * ---------------------------------------------------------------------------------------------- */
#define EGNN_ADAM_MAX_LAG 64
typedef struct egnn_adam_rows {
  float* p; float* m; float* v;                          /* [n_rows, ld] fp32, one ld */
  int32_t* last;                                         /* [n_rows] step the row is current for; -1 = never had a gradient */
  int64_t n_rows; int64_t D; int64_t ld;
  float beta1; float beta2; float eps;
  float one_minus_beta1; float one_minus_beta2;          /* formed on the host in double, like the rings */
  int32_t step;                                          /* t of the step being applied (step) / the step to reach (catch-up, flush) */
  int32_t flushed;                                       /* the last step every touched row is known to have reached (0: none yet) */
  float step_size[EGNN_ADAM_MAX_LAG];                    /* ring, index tau % MAX_LAG: lr_tau / (1 - beta1^tau) */
  float bc2_sqrt[EGNN_ADAM_MAX_LAG];                     /* ring: sqrt(1 - beta2^tau) */
  int32_t* dup_count;                                    /* device counter of batch rows whose step was not applied */
} egnn_adam_rows_t;
int egnn_group_input_f32(const float* const* tables, const int64_t* table_rows, int n_types, const int64_t* node_type,
                         const int64_t* local_idx, int64_t n, int64_t D, float* h, int64_t ldh, int32_t* oob, void* stream);
int egnn_adam_rows_catchup_f32(const egnn_adam_rows_t* a, int type_id, const int64_t* node_type, const int64_t* local_idx, int64_t n,
                               void* stream);
int egnn_adam_rows_flush_f32(const egnn_adam_rows_t* a, void* stream);
int egnn_adam_rows_step_f32(const egnn_adam_rows_t* a, int type_id, const int64_t* node_type, const int64_t* local_idx, int64_t n,
                            const float* g, int64_t ldg, void* stream);
/* egnn_adam_rows_step_sum_f32  the step over a list that may name a table row SEVERAL times (the batches of one accumulated step, or
 *     of several data-parallel ranks).  Entry i is selected when node_type[i] == type_id (every entry when node_type == NULL); a
 *     selected entry with local_idx[i] outside [0, n_rows) is not applied and adds 1 to *dup_count.  For a table row r named by the
 *     selected entries i1 < i2 < ... < ik the gradient is  G_r = scale * (((g[i1] + g[i2]) + ...) + g[ik])  -- plain fp32 adds in
 *     ascending entry order, one multiply -- and r takes exactly ONE step `step` with G_r, claimed like egnn_adam_rows_step_f32 (a row
 *     that is not current for step - 1 is not stepped and adds 1 to *dup_count).  With no row named twice and scale == 1.0f the
 *     result equals egnn_adam_rows_step_f32's bit for bit.  The entries get 64-bit keys (row, entry), radix-sorted over the bits they
 *     use; the lane group at the head of a row's run adds the run in registers.  No float atomics, no dense gradient: the result
 *     does not depend on the launch geometry.  n and n_rows < 2^31 - 1.  ws: egnn_adam_rows_step_sum_ws_bytes(n, n_rows) bytes,
 *     16-byte aligned (two key arrays of 8 n bytes and the sort's temporary storage: O(n), independent of n_rows x D); else
 *     EGNN_EWORKSPACE.  Checks as egnn_adam_rows_step_f32, all before any launch; n == 0 enqueues nothing (ws may be NULL).
 *     The sort's temporary size is asked of hipCUB, which reads the current device's configuration: in a process without a
 *     device egnn_adam_rows_step_sum_ws_bytes counts the two key arrays only, and the step returns EGNN_ELAUNCH (before any
 *     launch) if that query fails.  Size the workspace in the process, and on the device, that runs the step. */
size_t egnn_adam_rows_step_sum_ws_bytes(int64_t n, int64_t n_rows);
int egnn_adam_rows_step_sum_f32(const egnn_adam_rows_t* a, int type_id, const int64_t* node_type, const int64_t* local_idx, int64_t n,
                                const float* g, int64_t ldg, float scale, void* ws, size_t ws_bytes, void* stream);

/* DIAGNOSTIC (measurement only; bench.py's roofline.gather_ceiling_GBs): replays the gather stream of one aggregation call and
 * nothing else -- for every stored entry e, the 128-byte slice s of row col[e] of X [n_src, K] is read by an 8-lane sub-group,
 * slice s by the workgroups with blockIdx % (K / 32) == s (the aggregation kernel's slice <-> XCD binding,
 * efficient-gnns_amd/csrc/spmm_blk.hip).  nnz * K * 4 bytes of lines per call; `sink` [1] is never written for finite data.
 * K % 32 == 0, X 16-byte aligned, int32 column ids; loads_in_flight = independent 16-byte gathers per lane (4, 8 or 16).
 * No counterpart in the reference. */
int egnn_probe_gather_lines_f32(const float* X, int64_t ldx, int64_t n_src, int64_t K, const int32_t* col, int64_t nnz,
                                int blocks_per_slice, int loads_in_flight, float* sink, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gather, add the edge's own row, activate and aggregate in one walk (csrc/gather_edge_scatter.hip): the message relu(x_j + edge_attr)
 * of the convs that read edge features (PyG's GINEConv [ext]; the reference's mol_pyg is a README only) without an [S, C] tensor.  No
 * float atomics, no integer atomics; first derivatives only.
 *
 * egnn_gather_edge_scatter_runs_f32   replaces ops.scatter(relu(ops.take_rows(x, src) + e), dst): a gather that writes [S, C], an add,
 *     a relu that writes [S, C] again and the run-sum that reads it.  For every row r < n_rows, over the positions p of r's run in
 *     keys_sorted (keys_sorted, S, shift, from, x, n_x, from_count, count, reduce, ws: as egnn_gather_scatter_runs_f32 below):
 *         out[r, c] = reduce_p  m[p, c],     v[p, c] = x[from[p], c] / (float)from_count[from[p]]   (the division only when from_count != NULL)
 *         mode 0 (ADD):       m = v + e[p, c]                     (e == NULL: m = v)
 *         mode 1 (ADD_RELU):  m = max(v + e[p, c], 0)             (the sum rounded to fp32 first; a sum that is not > 0 gives +0)
 *         mode 2 (GATE):      m = own[r, c] + e[p, c] > 0 ? v : 0
 *     GATE is the backward of ADD_RELU for the gathered-from side: walked over the SOURCE side's keys with from = the target rows
 *     (-1 for a dropped id), x = the gradient of out, from_count = the forward's count for mean and own = the forward's x, whose row r
 *     every position of r's run read.  The backward of ADD is ADD with e == NULL.
 *     e float [S, ld_e], ld_e >= C: the row of position p; own float [n_rows, ld_own], ld_own >= C (read in GATE only).  A from entry
 *     outside [0, n_x) reads nothing and stands for a row of zeros (m = e[p], max(e[p], 0), 0): what the materialised messages hold
 *     for a target id a deferred plan dropped.  EVERY row of out [n_rows, ld_out] is written, a row that no key names gets 0; count
 *     and mean's division as egnn_gather_scatter_runs_f32.
 *     ORDER OF THE ADDITIONS: egnn_rows_add_runs_f32's over m -- the first message of a chunk of EGNN_ROWS_SUM_CHUNK positions is taken
 *     as it is, the others are added in ascending position, a long run's chunks are parked in ws and merged in ascending chunk order.
 *     The result is bit-equal to egnn_scatter_runs_f32 over the materialised messages, whatever the pitches and alignments.
 *     16 bytes per lane when C % 4 == 0, every pitch % 4 == 0 and out, x, e and own are 16-byte aligned; a scalar path with the same
 *     arithmetic otherwise.  Four keys, then four ids and four rows of e, then four rows of x are in flight per lane.
 *     Occupancy as egnn_gather_scatter_runs_f32 (8 waves per SIMD) except on the 16-byte path for mode 0 / 1 WITH from_count, which
 *     holds four rows of e, four rows of x and four divisors: 7 waves (no scratch anywhere; profiles/gather_edge_scatter_resources.txt).
 *     ws: egnn_gather_edge_scatter_ws_bytes(S, C) bytes (= egnn_rows_add_runs_ws_bytes), 16-byte aligned; missing or short:
 *     EGNN_EWORKSPACE; misaligned pointers: EGNN_EALIGN; mode outside 0 .. 2, mode 1 / 2 without e, mode 2 without own, sizes and
 *     pitches as egnn_gather_scatter_runs_f32: EGNN_EINVAL.  Every check happens before the first launch.  S == 0: EGNN_OK; with a
 *     non-NULL out the n_rows rows and counts are zeroed.
 *
 * egnn_edge_gate_f32   replaces the relu and scatter backward passes over [S, C]: the gradient of the edge rows,
 *         de[p, c] = gate ? g[b_rows[p], c] / (float)b_count[b_rows[p]] : 0,    gate = mode == 0 || x[a_rows[p], c] + e[p, c] > 0
 *     for p < S (the division only when b_count != NULL), mode 0 or 1.  a_rows / b_rows int64 [S]: the rows of x [n_x, ld_x] and of the
 *     gradient g [n_g, ld_g] that position p names; a b_rows entry outside [0, n_g) gives de[p, :] = 0 and reads nothing, an a_rows
 *     entry outside [0, n_x) stands for a row of zeros.  mode 0 reads neither a_rows, x nor e.  Elementwise: no reduction, every
 *     element of de [S, ld_de] is written with a plain store, one lane group per position.  S < 2^31 - 1, C >= 1, pitches >= C: else
 *     EGNN_EINVAL; misaligned pointers: EGNN_EALIGN.  S == 0: EGNN_OK.
 * ---------------------------------------------------------------------------------------------- */
size_t egnn_gather_edge_scatter_ws_bytes(int64_t S, int64_t C);
int egnn_gather_edge_scatter_runs_f32(float* out, int64_t ld_out, int64_t n_rows, int32_t* count, const uint64_t* keys_sorted, int64_t S,
                                      int shift, const int64_t* from, const float* x, int64_t ld_x, int64_t n_x, const int32_t* from_count,
                                      const float* e, int64_t ld_e, const float* own, int64_t ld_own, int mode, int64_t C, int reduce,
                                      void* ws, size_t ws_bytes, void* stream);
int egnn_edge_gate_f32(float* de, int64_t ld_de, int64_t S, int64_t C, const int64_t* a_rows, const float* x, int64_t ld_x, int64_t n_x,
                       const float* e, int64_t ld_e, const int64_t* b_rows, const float* g, int64_t ld_g, int64_t n_g,
                       const int32_t* b_count, int mode, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gather, weight and aggregate in one walk (csrc/gather_scatter.hip): the lift, the per-edge weight and the aggregation of a
 * message-passing layer without the [S, C] message tensor, and the per-edge dot that is the weights' gradient.  No float atomics, no
 * integer atomics; first derivatives only.
 *
 * egnn_gather_scatter_runs_f32   for every row r < n_rows, over the positions p of r's run in keys_sorted (keys_sorted, S, shift as
 *     egnn_rows_plan_build_i64 made them) and with D = C / H columns per head:
 *         out[r, c] = reduce_p  m[p, c],     m[p, c] = (x[from[p], c] / (float)from_count[from[p]]) * w[p, c / D]
 *     each step rounded to fp32 (the division only when from_count != NULL, the multiply only when w != NULL: weight 1).
 *     from int64 [S]: addresses into x [n_x, ld_x]; an entry outside [0, n_x) reads nothing and stands for a row of zeros (it still
 *     takes its weight, as a materialised message would).  w float [S, ld_w], H >= 1 columns, C % H == 0; w == NULL needs H == 1 (or S == 0).
 *     reduce: 0 sum, 1 mean (anything else: EGNN_EINVAL).  count int32 [n_rows] (nullable; required for mean): the length of row
 *     r's run, written as egnn_scatter_runs_f32 writes it; mean divides the sum by (float)count[r], one correctly rounded division
 *     per element.  EVERY row of out [n_rows, ld_out] is written, a row that no key names gets 0 (no memset needed).
 *     ORDER OF THE ADDITIONS: egnn_rows_add_runs_f32's, over m instead of src -- the same cut into chunks of EGNN_ROWS_SUM_CHUNK
 *     positions read off the keys, P_j = ((m[p_(jK+1)] + m[p_(jK+2)]) + ...) in ascending position, a long run's chunks parked in
 *     ws and merged in ascending chunk order.  The result is therefore bit-equal to egnn_scatter_runs_f32 over the materialised
 *     messages m, for sum and mean, whatever the pitches and alignments.
 *     The backward of x is this entry point over the SOURCE side's keys: from = the target rows (-1 for a dropped id), x = the
 *     gradient of out, from_count = the forward's count for mean, out = dx [n_src, C].
 *     16 bytes per lane when D % 4 == 0, ld_out and ld_x % 4 == 0 and out and x are 16-byte aligned; a scalar path with the same
 *     arithmetic otherwise.  Four keys, then four ids and weights, then four rows are in flight per lane.
 *     ws: egnn_gather_scatter_ws_bytes(S, C) bytes (= egnn_rows_add_runs_ws_bytes), 16-byte aligned (0 for S <= EGNN_ROWS_SUM_CHUNK);
 *     missing or short: EGNN_EWORKSPACE; misaligned ws / keys / from / other operands: EGNN_EALIGN; S and n_rows < 2^31 - 1, C >= 1,
 *     pitches >= C (ld_w >= H), shift = the number of bits of S - 1: else EGNN_EINVAL.  Every check happens before the first launch.
 *     S == 0: EGNN_OK; with a non-NULL out the n_rows rows and counts are zeroed.  A key whose position or row does not fit
 *     S / n_rows is skipped, never used as an address.
 *
 * egnn_edge_dot_f32   dw[p, h] = sum over the D = C / H columns c of head h of A[a_rows[p], c] * B[b_rows[p], c], p < S (a COO SDDMM
 *     with two gathers), divided by (float)a_count[a_rows[p]] when a_count != NULL.  a_rows / b_rows int64 [S]; an entry outside
 *     [0, n_a) / [0, n_b) gives dw[p, :] = 0 and reads nothing.  dw [S, ld_dw], ld_dw >= H; every element is written with a plain store.
 *     ORDER OF THE ADDITIONS, a function of (C, H) only: one group of G = min(64, pow2ceil(ceil(D / 4))) lanes per (p, h); lane l
 *     starts from 0.f and adds the products (each rounded to fp32) of the head's columns 4 (l + G t) + i, t = 0, 1, ..., i = 0 .. 3,
 *     below D, in ascending column order; the G lane sums meet in a butterfly over xor offsets G / 2 .. 1 (egnn_group_sum).  Pitches
 *     and alignments only decide whether the same columns are loaded 16 bytes at a time: the bits do not depend on them, two calls
 *     are bit-equal, and head h of an H-head call equals the one-head call on that head's column block.
 *     S < 2^31 - 1, C >= 1, H >= 1, C % H == 0, pitches >= C: else EGNN_EINVAL; misaligned pointers: EGNN_EALIGN.  S == 0: EGNN_OK.
 * ---------------------------------------------------------------------------------------------- */
size_t egnn_gather_scatter_ws_bytes(int64_t S, int64_t C);
int egnn_gather_scatter_runs_f32(float* out, int64_t ld_out, int64_t n_rows, int32_t* count, const uint64_t* keys_sorted, int64_t S,
                                 int shift, const int64_t* from, const float* x, int64_t ld_x, int64_t n_x, const int32_t* from_count,
                                 const float* w, int64_t ld_w, int64_t H, int64_t C, int reduce, void* ws, size_t ws_bytes, void* stream);
int egnn_edge_dot_f32(float* dw, int64_t ld_dw, int64_t S, int64_t H, int64_t C, const int64_t* a_rows, const float* A, int64_t ld_a,
                      int64_t n_a, const int64_t* b_rows, const float* B, int64_t ld_b, int64_t n_b, const int32_t* a_count,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGNN_HIP_H */
