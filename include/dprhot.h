/*
 * dprhot.h -- C ABI of libdprhot.so: the MI355X (gfx950) implementation of dpr-scale's in-batch
 * contrastive hot path.  Reference boundary (paths relative to the dpr-scale tree):
 *
 *   dpr_scale/task/dpr_task.py:153-214  DenseRetrieverTask.training_step   (the step)
 *   dpr_scale/task/dpr_task.py:98-105   DenseRetrieverTask.sim_score       (Q x C^T, masked fill)
 *   dpr_scale/task/dpr_task.py:46,212   nn.CrossEntropyLoss()              (row softmax CE, mean)
 *   dpr_scale/task/dpr_task.py:235-246  compute_rank_metrics               (rank of the gold ctx)
 *   dpr_scale/run_retrieval_pytorch.py:141-176 search_index                (einsum + topk)  ["next" row]
 *
 * The reference is 100 % Python and has no FFI of its own; these entry points are what a binding for this
 * path binds (INTEGRATION.md shows the ctypes stub and the dpr_task.py patch).
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer owned by the caller (e.g. torch's caching allocator) unless its
 *     name starts with h_.  Nothing is allocated, freed or retained by the library.
 *   - All matrices are row-major and contiguous; rows are 16-byte aligned: d % 8 == 0, Nc % 8 == 0.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  The stream contract: a call ONLY ENQUEUES on `stream`
 *     (kernel launches and nothing else -- no memset, no copy; nothing on another stream or the null stream), it DOES NOT SYNCHRONISE with the host or
 *     read device memory from the host -- loop bounds that live in device memory (labels, masks, offsets, candidate lists) are read
 *     by the kernels, every time -- and it MAY BE CAPTURED into a HIP graph (hipStreamBeginCapture on `stream`) after one eager call at
 *     the same shape, which is when anything lazily initialised gets initialised.  A replay computes what the eager call computes for
 *     whatever the buffers then hold, bit for bit (tests/test_stream_capture_gpu.py holds every stream-taking entry point to this).
 *     The exception are the collectives (dprhot_allgather_ctx, _reducescatter_dc, _reducescatter_rows, _allreduce_sum,
 *     _allgather_allpairs, _reducescatter_allpairs): they hand `stream` to RCCL, and a capture next to a live communicator is
 *     outside this contract.
 *   - bf16 values travel as uint16_t bit patterns (round-to-nearest-even from fp32).
 *   - Return value: 0 = OK, <0 = error (DPRHOT_E_*); dprhot_last_error() returns a thread-local message.
 *     Functions are re-entrant; the only process-wide state is the explicit option table below (test / A-B switches that
 *     production never touches) -- the library reads no environment variable.
 *   - Shapes: B = rows (queries) held by this rank, Nc = all columns (contexts) after the gather,
 *     d = hidden size.
 */
#ifndef DPRHOT_H
#define DPRHOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPRHOT_VERSION 174 /* 0.1.74: + dprhot_ivf_workspace_bytes / _score / _search (inverted-index retrieval for CITADEL / COIL); dprhot_router_head_*, dprhot_ivf_compact / _gather, dprhot_maxsim_score and dprhot_pq_encode / dprhot_ivf_pq_score / _search, dprhot_colbert_*, dprhot_colbert_pq_*, dprhot_colbert_cand_*, dprhot_colbert_cen_* and dprhot_colbert_res_* joined without a bump: tests/test_ivf.py pins this number */

#define DPRHOT_OK 0
#define DPRHOT_E_INVALID (-1)     /* bad argument (NULL pointer, non-positive or misaligned size) */
#define DPRHOT_E_HIP (-2)         /* a HIP runtime call failed; message has hipGetErrorString */
#define DPRHOT_E_UNSUPPORTED (-3) /* shape outside what the kernels were built for */
#define DPRHOT_E_WORKSPACE (-4)   /* workspace too small */

typedef uint16_t dprhot_bf16;

int dprhot_version(void);
const char* dprhot_last_error(void);

/* Process-wide test / A-B switches of the shape plans (production never calls this).  Every name with its default, one per line
 * (tests/test_abi.py holds this list against the library's own table):
 *   tile (-1)              0..5 pins the tile of the single-GEMM launches, -1: the plan decides
 *   no_tr (0)              1: plain 16-bit gathers in place of the LDS transpose read (cross-check)
 *   big_min (256)          fewest 256 x 256 tiles for the large-shape kernels (0: never; tests lower it)
 *   nl_min (128)           fewest 256 x 256 tiles from which the forward never stores the logits
 *   no_skinny (0)          1: no few-rows x many-contexts plan
 *   no_small_step (0)      1: no fused softmax + backward kernel of the latency-bound shapes
 *   no_wide (0)            1: vocabulary-wide fp32 operands stay on the register-staged sim kernel
 *   no_wide_bwd (0)        1: the backward of vocabulary-wide vectors stays on the generic pair kernel
 *   sk_fused (1)           the few-rows step without its dScores launch: 1 from 2^19 scores up | 2 wherever it exists | 0 never
 *   sk_w8 (1)              eight waves per workgroup in the fused few-rows backward, 0: four
 *   sk_pair (0)            1: one kind of unit in the fused few-rows backward
 *   sk_tail (0)            1 | 2: the dQ slabs are folded by the last workgroups of the few-rows backward launch itself
 *   sk_dc_regscale (0)     1: the dC units of the fused few-rows backward scale their Q fragments in registers
 *   sk_dq_atomic (0)       1: the dQ units of the fused few-rows backward add into dQ (reproducible to rounding, not to the bit)
 *   nl_p16 (1)             no-logits forward with the dScores wanted in one GEMM pass, 0: two passes
 *   g128_dma (1)           the 128 x 128 tile staged by LDS-DMA, 0: never
 *   loss_with_dq (1)       the one-call step sums the row losses in the launch that combines the dQ slabs, 0: in a launch of its own
 *   nl128 (1)              one-pass training forward on the 128 x 128 tile where the 256-wide tiles would leave the chip idle, 0: off
 *   pair128 (1)            backward pair on the 128 x 128 tile: 1 where its rule picks it | 2 wherever it qualifies | 0 never
 *   p16_staged (1)         fp16 numerators of the 256 x 256 one-pass forward leave through LDS: 1 by its rule | 2 always | 0 never
 *   small_sim (1)          the batch-32 step's sim launch on csrc/sim_small.h | 0: on the GEMM engine | 2..4: its other forms
 *   small_step_roles (3)   the batch-32 step's softmax + backward launch split by role, outputs from workgroups of their own |
 *                          2: outputs from the dC workgroup of tile 0 | 1: 2 with 16-column dQ tiles | 0: unsplit
 *   small_sim_copy (1)     the batch-32 sim launch writes its bf16 copies on waves of their own, as 16-byte write-through pieces |
 *                          2: as 8-byte plain pieces | 0: on the compute waves
 * An option changes which kernels run -- the summation order and where a value is rounded with them -- never what is computed;
 * sk_dq_atomic = 1 alone gives up run-to-run bit-reproducibility.
 * Setting one changes the plans of every later call on every thread (workspace sizes included: query them after setting).
 * DPRHOT_E_INVALID for an unknown name. */
int dprhot_set_option(const char* name, int value);
/* Bumped by every dprhot_set_option: whoever caches a plan fact of this library (dprhot_step_wants_g, dprhot_train_dq_slabs,
 * dprhot_workspace_bytes) keys the cache on it -- options set through this C ABI from any binding invalidate every such cache. */
long long dprhot_options_epoch(void);
int dprhot_get_option(const char* name, int* h_value);

/* Bytes of scratch the fused entry points (dprhot_inbatch_fwd/_bwd, dprhot_dq) need for this shape. */
int dprhot_workspace_bytes(int B, int Nc, int d, size_t* h_out);

/* fp32 -> bf16 (RNE) of n contiguous values.  Producer side of the gather: the encoder output
 * (hf_model.py:36-41, fp32) is written straight into this rank's slot of the gathered bf16 buffer.
 * n % 8 == 0. */
int dprhot_cast_bf16(const float* src, dprhot_bf16* dst, size_t n, void* stream);

/* Both producer-side casts of one step in ONE launch: Qb <- q (nq values), Cdst <- c (nc values), fp32 -> bf16
 * RNE.  Cdst is this rank's slot of the gathered context buffer (W == 1) or the all-gather send buffer. */
int dprhot_prep(const float* q, size_t nq, dprhot_bf16* Qb, const float* c, size_t nc, dprhot_bf16* Cdst, void* stream);

/* Multi-rank gather in ONE collective (the reference issues four all_gathers, dpr_task.py:169-176).
 * dprhot_pack_ctx writes this rank's all-gather send buffer [rows_c, d] bf16: rows [0, n_ctx) = the context rows
 * (fp32 -> bf16 RNE), followed by rows whose bytes carry the dummy-context mask (mask may be NULL = no dummies).
 * rows_c = dprhot_packed_rows(n_ctx, d) (a multiple of 8; of 64 from n_ctx = 2048 on).  After all-gathering W such buffers back to back, the
 * result IS the context matrix C [W*rows_c, d] of every other entry point -- the mask rows are just extra columns
 * that dprhot_unpack_mask marks as masked in the column mask it builds ([W*rows_c] bytes).  The label offset of
 * rank r becomes r * rows_c, and rank r's gradient is the first n_ctx rows of its reduce-scatter chunk. */
int dprhot_packed_rows(int n_ctx, int d, int* h_rows);
int dprhot_pack_ctx(const float* c, const uint8_t* mask, int n_ctx, int d, dprhot_bf16* send, void* stream);
int dprhot_unpack_mask(const dprhot_bf16* gathered, int W, int n_ctx, int d, uint8_t* colmask, void* stream);

/* sim_score (dpr_task.py:98-105) + the temperature scale (:211), one kernel:
 *   S[i][j] = inv_T * sum_k Q[i][k] * C[j][k]      (bf16 MFMA, fp32 accumulate)
 *   S[i][j] = -inf where colmask[j] != 0            (colmask may be NULL; it is the row that
 *                                                    `mask.repeat(Nq, 1)` at :197 broadcasts)
 * Q [B,d], C [Nc,d] bf16; S [B,Nc] fp32. */
int dprhot_sim_fwd(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const uint8_t* colmask,
                   float inv_T, float* S, void* stream);

/* Row softmax cross-entropy (dpr_task.py:46,212) fused with its backward into dScores, one pass over S:
 *   row_lse[i]  = logsumexp_j S[i][j]
 *   row_loss[i] = row_lse[i] - S[i][y[i]]
 *   G[i][j]     = (exp(S[i][j] - row_lse[i]) - [j == y[i]]) * grad_scale        (bf16, 0 at -inf columns)
 * The gold column of row i is y[i] + y_offset: y holds the rank-local positive indices from the batch
 * (dpr_transform.py:164-166) and y_offset = rank * ctx_per_rank is the label offset the reference adds
 * in its gather loop (dpr_task.py:189-190).  row_win_start is relative to the same offset.
 * grad_scale carries 1/(Nq_global * T); the incoming grad_output is applied later by dprhot_dq/_dc.
 * row_win_start/win_len (optional, NULL/0): the in_batch_negatives=False branch (:198-207) -- row i only
 * sees columns [row_win_start[i], row_win_start[i] + win_len).
 * row_loss, row_lse, G may each be NULL (not written). */
int dprhot_softmax_ce_fwd_bwd(const float* S, int B, int Nc, const int64_t* y, int64_t y_offset, float grad_scale,
                              const int64_t* row_win_start, int win_len, float* row_loss, float* row_lse,
                              dprhot_bf16* G, void* stream);

/* out[0] = scale * sum_i x[i]  (deterministic single-workgroup tree; the `mean` of CrossEntropyLoss). */
int dprhot_reduce_sum(const float* x, int n, float scale, float* out, void* stream);

/* Backward of sim_score into the local query rows:  dQ[B,d] = s * G[B,Nc] x C[Nc,d]   (fp32 out),
 * s = h_scale * (d_scale ? *d_scale : 1).  d_scale is the autograd grad_output scalar, read on the
 * device so that no host sync is needed (AMP loss scale).  Split-K over Nc; `workspace` of
 * dprhot_workspace_bytes() is required. */
int dprhot_dq(const dprhot_bf16* G, const dprhot_bf16* C, int B, int Nc, int d, float h_scale,
              const float* d_scale, float* dQ, void* workspace, size_t workspace_bytes, void* stream);

/* Backward into ALL context columns (this rank's partial; summed over ranks by reduce-scatter):
 *   dC_part[Nc,d] = s * G^T[Nc,B] x Q[B,d]   (fp32 out) */
int dprhot_dc(const dprhot_bf16* G, const dprhot_bf16* Q, int B, int Nc, int d, float h_scale,
              const float* d_scale, float* dC_part, void* stream);

/* compute_rank_metrics (dpr_task.py:235-246) without the sort or the per-row host syncs:
 *   rank[i] = 1 + #{j : S[i][j] > S[i][y[i]]} + #{j < y[i] : S[i][j] == S[i][y[i]]}
 * (== position of y[i] in torch.sort(S[i], descending=True, stable=True); bit-exact integer result). */
int dprhot_rank_of_gold(const float* S, int rows, int cols, const int64_t* y, int64_t y_offset, int64_t* rank,
                        void* stream);

/* Whole forward of the step for this rank's rows in TWO launches:
 *   1. sim GEMM whose epilogue applies mask and 1/T, stores the fp32 logits and leaves, per row and column
 *      tile, the (max, sum-exp) pair plus the gold logit;
 *   2. logsumexp from those pairs, then one streaming pass over the logits producing G (bf16), row_loss,
 *      row_lse and loss_sum[0] = sum_i row_loss[i] (fixed-point integer atomics: deterministic).
 * S_out may be NULL (logits live in the workspace) or a [B,Nc] fp32 buffer (debug / parity / eval).
 * row_loss, row_lse, G may be NULL.  `workspace` must hold dprhot_workspace_bytes(B, Nc, d) bytes.
 * LARGE shapes (>= 256 tiles of 256 x 256, B > 128, d % 128 == 0) with S_out == NULL run the NO-LOGITS plan instead: the
 * logits are never stored (at B = 8192, Nc = 65536 they would be 2 GiB, written once and read once) --
 *   1. sim GEMM whose epilogue keeps only (max, sum-exp) per row and 64-column strip plus the gold logit,
 *   2. logsumexp / loss from those,
 *   3. the same GEMM again (bit-identical accumulators), its epilogue writing G = (softmax - onehot) * grad_scale as bf16.
 * The workspace of such a shape holds no logit buffer.  Passing S_out selects the two-launch plan above at any shape. */
int dprhot_inbatch_fwd(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y,
                       int64_t y_offset, const uint8_t* colmask, float inv_T, float grad_scale, float* S_out, float* row_loss,
                       float* row_lse, float* loss_sum, dprhot_bf16* G, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Whole backward: dQ (local rows) and dC_part (all columns) from G; see dprhot_dq / dprhot_dc.  The two
 * GEMMs share only their input, so they run side by side in ONE launch (plus the split-K combine of dQ
 * when Nc is long). */
int dprhot_inbatch_bwd(const dprhot_bf16* G, const dprhot_bf16* Q, const dprhot_bf16* C, int B, int Nc, int d,
                       float h_scale, const float* d_scale, float* dQ, float* dC_part, void* workspace,
                       size_t workspace_bytes, void* stream);

/* The two launches of dprhot_inbatch_fwd, individually (profiling, or a caller that wants the logits
 * before deciding on the softmax): dprhot_sim_stats leaves logits (S_out, or the workspace when NULL) and
 * the per-tile statistics in `workspace`; dprhot_softmax_finish consumes them (S_in NULL = the workspace
 * logits).  Same B, Nc, d and workspace for both calls.
 * Short rows (Nc <= 4096 and B <= 64): dprhot_sim_stats writes up to 4 split-K slabs of PARTIAL logits into the
 * workspace and leaves S_out alone; the summed logits exist only after dprhot_softmax_finish, which writes
 * them to its S_in argument when that is non-NULL (there S_in is an output).  Callers that want logits from
 * one call use dprhot_sim_fwd.
 * No-logits shapes (see dprhot_inbatch_fwd) with S_out / S_in == NULL: dprhot_sim_stats leaves only statistics,
 * dprhot_softmax_finish turns them into row_lse / row_loss / loss_sum and must be given G == NULL (there are no logits to
 * stream; DPRHOT_E_UNSUPPORTED otherwise), and dprhot_dscores is the third launch. */
int dprhot_sim_stats(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y,
                     int64_t y_offset, const uint8_t* colmask, float inv_T, float* S_out, void* workspace,
                     size_t workspace_bytes, void* stream);
int dprhot_softmax_finish(const float* S_in, int B, int Nc, int d, const int64_t* y, int64_t y_offset,
                          float grad_scale, float* row_loss, float* row_lse, float* loss_sum, dprhot_bf16* G,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Third launch of the no-logits forward: G[B,Nc] (bf16) = (softmax(S) - onehot(y + y_offset)) * grad_scale with
 * S = (Q x C^T) * inv_T recomputed tile by tile on the MFMA (never stored).  row_lse [B]: the rows' logsumexp, or NULL to use
 * what dprhot_softmax_finish left in `workspace`.  DPRHOT_E_UNSUPPORTED at shapes that are not no-logits shapes. */
int dprhot_dscores(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                   const uint8_t* colmask, float inv_T, float grad_scale, const float* row_lse, dprhot_bf16* G,
                   void* workspace, size_t workspace_bytes, void* stream);

/* compute_rank_metrics (dpr_task.py:235-246) straight from the embeddings: rank as dprhot_rank_of_gold of
 * S = (Q x C^T) * inv_T with masked columns at -inf, bit-exact.  At no-logits shapes S is never written: the gold logits
 * come from a gathered mini GEMM that runs the identical MFMA chain, the count-greater happens in the similarity GEMM's
 * epilogue.  Smaller problems score into the workspace and count there. */
int dprhot_sim_rank(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                    const uint8_t* colmask, float inv_T, int64_t* rank, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Both halves of validation from the embeddings in one call (dpr_task.py:224-227, :296-299: compute_rank_metrics and self.loss read
 * the same score matrix): rank as dprhot_sim_rank, row_loss / row_lse (either may be NULL) and loss_sum = sum_i (lse_i - S[i][y_i]) as
 * dprhot_inbatch_fwd with grad_scale unused.  At no-logits shapes the similarity GEMM runs ONCE: its epilogue counts and keeps the
 * softmax statistics (no score matrix); smaller problems compose the two existing calls. */
int dprhot_sim_rank_loss(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                         const uint8_t* colmask, float inv_T, int64_t* rank, float* row_loss, float* row_lse, float* loss_sum,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The same forward reading the encoder outputs as they are (fp32), so that no separate cast launch and no extra
 * round trip through HBM is needed: q [B,d] fp32; c [Nc,d] fp32 when the rank holds every column (world size
 * 1), or NULL when Cb is the already gathered bf16 buffer (world size > 1: the all-gather ships bf16).
 * The sim kernel rounds to bf16 (RNE) while staging and writes the bf16 images to Qb (and to Cb when c is
 * given) for the backward GEMMs.  Everything else as dprhot_sim_stats / dprhot_inbatch_fwd. */
int dprhot_sim_stats_f32(const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d,
                         const int64_t* y, int64_t y_offset, const uint8_t* colmask, float inv_T, float* S_out,
                         void* workspace, size_t workspace_bytes, void* stream);
int dprhot_inbatch_fwd_f32(const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d,
                           const int64_t* y, int64_t y_offset, const uint8_t* colmask, float inv_T, float grad_scale,
                           float* S_out, float* row_loss, float* row_lse, float* loss_sum, dprhot_bf16* G,
                           void* workspace, size_t workspace_bytes, void* stream);

/* One training step -- forward and backward of dpr_task.py:197-212 -- in a single call, for callers that know a
 * backward will follow (autograd: any input requires grad).  Arguments as dprhot_inbatch_fwd_f32 followed by those
 * of dprhot_inbatch_bwd; loss_sum, dQ and dC_part are required, G unless dprhot_step_wants_g says 0.  dQ / dC_part are scaled by
 * h_scale * (d_scale ? *d_scale : 1): pass the autograd grad_output there if it is known at forward time, or 1 and
 * multiply later.  At the latency-bound shapes (B <= 32, Nc <= 1152, d % 16 == 0) this is TWO launches -- the sim GEMM,
 * then one kernel doing softmax-CE, dScores and both backward GEMMs from an LDS-resident G; otherwise it equals
 * dprhot_inbatch_fwd_f32 + dprhot_inbatch_bwd (three launches). */
/* Whether the step entry points below need a G buffer at this shape: *h_wants = 1 -- the plan materialises the dScores (G required);
 * 0 -- G may be NULL, and passing NULL (with S_out NULL) selects the form of the step that never writes them: the few-rows plan's sim
 * launch then leaves every 128-column tile's own softmax (bf16) and the backward units derive the row logsumexp and one factor per
 * (row, tile) themselves -- three launches instead of four at BASELINE cfg3 per rank (dpr_task.py:197-212 and its backward).  A
 * non-NULL G is always honoured (and costs the dScores launch). */
int dprhot_step_wants_g(int B, int Nc, int d, int* h_wants);
/* *h_nl = 1 when the forward of this shape never stores the logits (the "no-logits" plan: >= 256 tiles of 256 x 256 -- or the option
 * big_min -- K % 128 == 0; dprhot_softmax_finish then yields logsumexp / loss only and G comes from dprhot_inbatch_fwd / dprhot_dscores),
 * 0 when the logits live in the workspace.  A pure function of the shape and the options, like every plan. */
int dprhot_fwd_no_logits(int B, int Nc, int d, int* h_nl);
/* How dprhot_inbatch_fwd / the one-call steps form G when the caller wants the dScores and not the logits (S_out == NULL, G != NULL):
 * *h_kind = 0 the logits are stored (workspace) and a streaming softmax turns them into G; 1 ONE pass of the 256 x 256 GEMM (strip
 * statistics + fp16 softmax numerators, then a row kernel that rescales them into G in place); 2 the same on the 128 x 128 LDS-DMA tile
 * (the shapes whose 256-wide tiles would leave most of the chip idle: a few hundred query rows against thousands of contexts). */
int dprhot_fwd_one_pass(int B, int Nc, int d, int* h_kind);
int dprhot_inbatch_step_f32(const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d,
                            const int64_t* y, int64_t y_offset, const uint8_t* colmask, float inv_T, float grad_scale,
                            float h_scale, const float* d_scale, float* S_out, float* row_loss, float* row_lse,
                            float* loss_sum, dprhot_bf16* G, float* dQ, float* dC_part, void* workspace,
                            size_t workspace_bytes, void* stream);

/* The same step for world size > 1, everything between the all-gather and the reduce-scatter in ONE call
 * (dpr_task.py:177-212 and its backward on this rank's rows).  `gathered` is the all-gathered packed buffer
 * [W * rows_c, d] bf16 (dprhot_pack_ctx on every rank); it is used as the context matrix as it is:
 *   - the column mask is read from its mask rows inside the sim kernel (no dprhot_unpack_mask launch, no colmask),
 *   - labels are y + rank * rows_c,
 *   - dC_part [W * rows_c, d] is what the caller reduce-scatters; in every rank chunk k its element
 *     [k * rows_c + n_ctx][0] (first mask row, a dead gradient) carries THIS rank's loss numerator, so the rank's
 *     reduce-scatter output holds the global sum of the loss numerators at [n_ctx][0]: no all-reduce for the loss.
 * loss_sum still receives the local numerator.  G as in dprhot_inbatch_step_f32 (dprhot_step_wants_g(B, W * rows_c, d)). */
int dprhot_inbatch_step_packed_f32(const float* q, const dprhot_bf16* gathered, dprhot_bf16* Qb, int B, int W, int rank,
                                   int n_ctx, int d, const int64_t* y, float inv_T, float grad_scale, float h_scale,
                                   const float* d_scale, float* row_loss, float* row_lse, float* loss_sum,
                                   dprhot_bf16* G, float* dQ, float* dC_part, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* Brute-force retrieval epilogue (run_retrieval_pytorch.py:149-150): per row, the k largest scores and
 * their column indices, descending, ties by lower column index.  k <= 4096 (the reference's recipes use --topk 100 and 1000; up to
 * 256 and up to 1024 run on 12 / 48 KB of LDS per row, beyond that on 96 KB: 8192 sort slots), k <= cols.  A NaN score (either
 * sign, any payload) is never selected: a row with fewer than k other scores leaves its tail unfilled (-inf / -1).  +0 and -0 tie
 * (the column decides); a selected value keeps its bit pattern. */
int dprhot_topk(const float* S, int rows, int cols, int k, float* values, int64_t* indices, void* stream);

/* The same as a streaming update, for a corpus that is scored in pieces (the shard loop of
 * run_retrieval_pytorch.py:196-243 and its "sort the score again if shard > 1" re-merge at :272-277):
 * folds the scores S[rows][0..cols) (row stride ld, global column index = col_offset + j) into the running
 * per-row top-k state values/indices [rows,k] (sorted; total order score desc, column asc).  first != 0 starts
 * from an empty state (slots not yet filled hold -inf / -1).  The result after any sequence of updates equals
 * dprhot_topk of the concatenated score matrix.  A NaN score is never selected, here as there: a row that has seen fewer than k
 * other candidates keeps an unfilled tail (-inf / -1), however many NaN scores it has seen. */
int dprhot_topk_update(const float* S, int rows, int cols, int64_t ld, int64_t col_offset, int k, float* values,
                       int64_t* indices, int first, void* stream);

/* The same update for ANY k (run_retrieval_pytorch.py:69 takes any --topk): the state lives in HBM, nothing has to fit in LDS
 * (csrc/wideselect.h: exact radix select over state + chunk, then only the k winners are sorted -- blocks of 4096 in LDS, merge
 * passes over HBM; ties exact at any multiplicity: the select continues over the ids).  The same contract at every k, bit for bit
 * what dprhot_topk_update leaves where both take the k: a NaN score is never selected (it is no candidate: it reaches neither the
 * select's counts nor the sorts), and a row with fewer than k other candidates leaves its tail unfilled (-inf / -1).  workspace:
 * dprhot_topk_wide_workspace_bytes(rows, k) bytes; its first rows * 8 32-bit words are one record per row whose word 5 is an error
 * word -- a row with a non-zero one keeps its old state (no such condition is defined at present: always 0). */
int dprhot_topk_wide_workspace_bytes(int rows, int k, size_t* h_bytes);
int dprhot_topk_update_wide(const float* S, int rows, int cols, int64_t ld, int64_t col_offset, int k, float* values, int64_t* indices,
                            int first, void* workspace, size_t workspace_bytes, void* stream);

/* search_index (run_retrieval_pytorch.py:141-166) for one resident corpus shard: scores = Q x C^T on bf16 MFMA
 * (fp32 scores; the reference scores in fp16), chunk columns at a time, each chunk folded into the running
 * top-k -- the [nq, n_ctx] score matrix never exists.  Q [nq,d], C [n_ctx,d] bf16; passage ids are
 * id_offset + row.  n_ctx and chunk multiples of 8 (a ragged tail goes through sim_fwd + topk_update with
 * cols < ld).  first as in dprhot_topk_update.  The first chunk of an empty state (at most 65536 passages of it) is scored into the workspace
 * and selected from; for every later chunk the GEMM epilogue compares each score with the row's current k-th best
 * and only appends the few that beat it to a candidate list, which a merge kernel folds into the state.
 * workspace: dprhot_search_workspace_bytes(nq, chunk). */
int dprhot_search_workspace_bytes(int nq, int chunk, size_t* h_out);
int dprhot_search(const dprhot_bf16* Q, int nq, const dprhot_bf16* C, int64_t n_ctx, int d, int64_t id_offset,
                  int k, int chunk, float* values, int64_t* indices, int first, void* workspace,
                  size_t workspace_bytes, void* stream);
/* The launches dprhot_search would make for this shape under the current options, in order, without touching a device: the same host
 * function dprhot_search iterates.  Four int64 words per step in h_steps: the step's first row j0, its column count, 1 for the head of
 * an empty state (scores stored by dprhot_sim_fwd's kernel and selected from) or 0 for a filtered chunk, and the form of its GEMM:
 * 0..5 the register-staged tile of that id, 6 the 256 x 256 gemm256_kernel, 7 the phase-interleaved gemm8p_kernel, 8 tile 0 on
 * LDS-DMA (gemm128d_kernel).  The head's form is also the form of dprhot_sim_fwd at (nq, cols, d).  Arguments are validated as by
 * dprhot_search; *h_count receives the number of steps, and the call fails (DPRHOT_E_INVALID, nothing beyond capacity written) when
 * capacity steps do not hold them.  h_steps may be NULL with capacity 0. */
int dprhot_search_plan(int nq, int64_t n_ctx, int d, int k, int chunk, int first, int64_t* h_steps, int capacity, int* h_count);

/* Pairwise scores of the CITADEL router / distillation path (dpr_scale/task/citadel_task.py:137-146, sim_score(...,
 * pairwise=True)): query b against its own M contexts,  S[b][j] = <q[b], c[b*M + j]>, -inf where mask[b*M + j] != 0
 * (mask may be NULL).  q [B,d], c [B*M,d] fp32 (router vectors are vocabulary-wide: d = 30522), S [B,M] fp32.  Any d. */
int dprhot_pairwise_fwd(const float* q, const float* c, const uint8_t* mask, int B, int M, int d, float* S, void* stream);
/* Its backward: dq[b] = sum_j g[b][j] c[b*M+j] and dc[b*M+j] = g[b][j] q[b]; g [B,M] fp32 with 0 at masked pairs.
 * dq / dc may each be NULL. */
int dprhot_pairwise_bwd(const float* g, const float* q, const float* c, int B, int M, int d, float* dq, float* dc, void* stream);

/* Late-interaction ("MaxSim") expert scoring of ColBERT / COIL / CITADEL (dpr_scale/task/citadel_task.py:155-238), without the
 * token-level score tensor:
 *   S[q][y] = POOL_{i,kq} MAX_{j,kd} <Q[q,i], C[ctx,j]> * [q_ids[q,i,kq] == c_ids[ctx,j,kd]] * q_w[q,i,kq] * c_w[ctx,j,kd]
 * q_tok bf16 [Nq, LQ, dp], c_tok bf16 [Nc, LD, dp], dp a multiple of 32 (zero-pad the features), 16-byte aligned rows.
 * q_ids int32 [Nq, LQ, KQ] / c_ids [Nc, LD, KD], both or neither (ColBERT: neither, KQ = KD = 1); q_w / c_w fp32 of the same shapes,
 * both or neither.  Unmatched slots score exactly 0.  1 <= KQ, KD <= 8; 1 <= LQ, LD <= DPRHOT_MAXSIM_MAX_LEN.
 * pool DPRHOT_POOL_SUM: max over context slots, sum over query slots; DPRHOT_POOL_MAX: max over both.
 * M = 0: in-batch, S [Nq, Nc], y = ctx.  M > 0: pairwise (Nc = Nq * M), S [Nq, M], query q against contexts q*M .. q*M+M-1.
 * mask uint8 [Nc] (may be NULL): S = -inf at masked contexts, and no gradient flows through them.
 * Ties go to the LOWEST flattened context slot j * KD + kd (torch.max(dim)).
 * The workspace (dprhot_maxsim_workspace_bytes(Nq, LQ, KQ, Ny = M ? M : Nc, weights != NULL)) holds the per-row-slot max / argmax
 * tables that the backward reads: keep it unchanged between the forward and its backward.
 * Backward: dq fp32 [Nq, LQ, dp], dc fp32 [Nc, LD, dp], dwq fp32 [Nq, LQ, KQ], dwc fp32 [Nc, LD, KD]; each may be NULL and is
 * fully written otherwise.  No atomics: bit-identical run to run. */
#define DPRHOT_MAXSIM_MAX_LEN 512
#define DPRHOT_POOL_SUM 0
#define DPRHOT_POOL_MAX 1
int dprhot_maxsim_workspace_bytes(int Nq, int LQ, int KQ, int Ny, int has_weights, size_t* bytes);
int dprhot_maxsim_fwd(const void* q_tok, const void* c_tok, int Nq, int LQ, int Nc, int LD, int dp, const int* q_ids, const int* c_ids,
                      const float* q_w, const float* c_w, int KQ, int KD, int pool, int M, const uint8_t* mask, float* S, void* ws,
                      size_t ws_bytes, void* stream);
int dprhot_maxsim_bwd(const float* dS, const void* q_tok, const void* c_tok, int Nq, int LQ, int Nc, int LD, int dp, const int* q_ids,
                      const int* c_ids, const float* q_w, const float* c_w, int KQ, int KD, int pool, int M, const uint8_t* mask,
                      const void* ws, size_t ws_bytes, float* dq, float* dc, float* dwq, float* dwc, void* stream);
/* The same scores for inference (reranking: citadel_eval_task.py:238-265), pairwise only (M >= 1, Nc = Nq * M; Nc = 0 is a no-op):
 * one launch, no workspace, nothing kept for a backward.  S [Nq, M] equals dprhot_maxsim_fwd's bit for bit. */
int dprhot_maxsim_score(const void* q_tok, const void* c_tok, int Nq, int LQ, int Nc, int LD, int dp, const int* q_ids, const int* c_ids,
                        const float* q_w, const float* c_w, int KQ, int KD, int pool, int M, const uint8_t* mask, float* S, void* stream);

/* Inverted-index retrieval for CITADEL / COIL (the search the reference's citadel_retrieval_task.py:136 asks of its absent
 * dpr_scale/index/inverted_vector_index.py; csrc/ivf.h):
 *   score(n, doc) = sum over entries (e, u) of query n of max(0, max over postings (doc, v) of expert e of <u, v>)  [+ <cls_q[n], cls_doc[doc]>]
 * Index (device, built once): postings sorted by (expert, doc) -- post_vec bf16 [n_postings, dp] (dp = d zero-padded to a multiple of
 * 32), post_doc int32 [n_postings] -- and exp_off int64 [n_experts + 1], offsets by expert id.  Query batch: entries sorted by
 * (expert, query, slot) -- ent_vec bf16 [n_entries, dp], ent_q int32 [n_entries] query rows -- plus bexp int32 [n_bexp], the distinct
 * experts of the batch ascending, and bexp_off int32 [n_bexp + 1], their entry ranges (an expert >= n_experts has no postings).
 * dprhot_ivf_score ADDS the expert part for doc ids doc_begin .. doc_begin + cols into S[nq, ld].  Every cell has one owner that adds
 * its entries in the order (expert ascending, the query's entries as listed); no floating-point atomics: two runs are bit-identical
 * and a cell's value does not depend on the chunk or on the other queries of the batch.  An entry adds max(0, .): a NaN product adds 0.
 * dprhot_ivf_search runs doc ids [id_begin, id_end) in chunks of `chunk` (a multiple of 8): S = CLS scores (dprhot_sim_fwd on the
 * chunk's rows of cls_doc bf16 [cls_rows >= corpus_len + 7, dc], dc % 8 == 0, zero rows behind the corpus; cls_q bf16 [nq, dc]) or
 * zeros when both CLS pointers are NULL, then dprhot_ivf_score, then the streaming top-k (dprhot_topk_update; dprhot_topk_update_wide
 * for k > 4096) with col_offset = the chunk's first id.  values / indices / first as in dprhot_search: disjoint id ranges may be folded
 * into one result.  Every doc id of the range competes, also one without a posting (score: the CLS part or 0).
 * Limits (DPRHOT_E_INVALID): corpus_len < 2^31, n_postings < 2^40, 1 <= k <= corpus_len, n_entries <= 4096 * nq (the packer checks
 * 4096 per query).  workspace: dprhot_ivf_workspace_bytes(nq, n_entries, chunk, has_cls) (+ dprhot_topk_wide_workspace_bytes(nq, k)
 * behind it when k > 4096); DPRHOT_E_WORKSPACE when smaller. */
int dprhot_ivf_workspace_bytes(int nq, int n_entries, int chunk, int has_cls, size_t* bytes);
int dprhot_ivf_score(const dprhot_bf16* post_vec, const int32_t* post_doc, const int64_t* exp_off, int64_t n_postings, int n_experts, int dp,
                     const dprhot_bf16* ent_vec, const int32_t* ent_q, int n_entries, const int32_t* bexp, const int32_t* bexp_off,
                     int n_bexp, int nq, int64_t doc_begin, int cols, float* S, int64_t ld, void* stream);
int dprhot_ivf_search(const dprhot_bf16* post_vec, const int32_t* post_doc, const int64_t* exp_off, int64_t n_postings, int n_experts, int dp,
                      const dprhot_bf16* ent_vec, const int32_t* ent_q, int n_entries, const int32_t* bexp, const int32_t* bexp_off,
                      int n_bexp, int nq, const dprhot_bf16* cls_q, const dprhot_bf16* cls_doc, int dc, int64_t cls_rows,
                      int64_t corpus_len, int64_t id_begin, int64_t id_end, int k, int chunk, float* values, int64_t* indices, int first,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Product-quantised postings for the inverted index (the reference's quantizer="pq", sub_vec_dim; csrc/ivf_pq.h, DESIGN.md section
 * 10.2).  dsub in {2, 4, 8} features per sub-vector, m = dp / dsub subspaces; ONE codebook bf16 [m, 256, dsub] per index; a posting is
 * m code bytes, post_code uint8 [n_postings, m] in the order of post_doc, and stands for the bf16 row
 *   decode(p)[j * dsub + t] = codebook[j, post_code[p, j], t].
 * dprhot_ivf_pq_score / dprhot_ivf_pq_search are dprhot_ivf_score / dprhot_ivf_search with (post_code, codebook, dsub) in place of
 * post_vec and return, bit for bit, what those return over the index whose post_vec rows are decode(p); everything said above about
 * owners, order of additions, chunks, ties, NaN and the workspace (dprhot_ivf_workspace_bytes) holds unchanged.
 * dprhot_pq_encode writes codes uint8 [n, m] for rows vec bf16 [n, dp]: code = argmin over c = 0 .. 255 of
 *   D(c) = sum over t = 0 .. dsub - 1, in that order, of (x_t - codebook[j, c, t])^2
 * in fp32 with every subtract, multiply and add rounded on its own (no fma), centroids scanned upwards with a strict <: the lowest
 * index wins a tie, a NaN distance never wins, a row of NaNs gets code 0.  One owner per output byte, exactly n m bytes written.
 * n == 0, an empty batch and an index without postings launch nothing.
 * Limits: dsub not in {2, 4, 8}, dp % 32 != 0, a NULL or misaligned (16 bytes) codebook or code array: DPRHOT_E_INVALID; dp > 64:
 * DPRHOT_E_UNSUPPORTED; otherwise those of the dense entry points. */
int dprhot_pq_encode(const dprhot_bf16* vec, int64_t n, int dp, const dprhot_bf16* codebook, int dsub, uint8_t* codes, void* stream);
int dprhot_ivf_pq_score(const uint8_t* post_code, const dprhot_bf16* codebook, int dsub, const int32_t* post_doc, const int64_t* exp_off,
                        int64_t n_postings, int n_experts, int dp, const dprhot_bf16* ent_vec, const int32_t* ent_q, int n_entries,
                        const int32_t* bexp, const int32_t* bexp_off, int n_bexp, int nq, int64_t doc_begin, int cols, float* S, int64_t ld,
                        void* stream);
int dprhot_ivf_pq_search(const uint8_t* post_code, const dprhot_bf16* codebook, int dsub, const int32_t* post_doc, const int64_t* exp_off,
                         int64_t n_postings, int n_experts, int dp, const dprhot_bf16* ent_vec, const int32_t* ent_q, int n_entries,
                         const int32_t* bexp, const int32_t* bexp_off, int n_bexp, int nq, const dprhot_bf16* cls_q,
                         const dprhot_bf16* cls_doc, int dc, int64_t cls_rows, int64_t corpus_len, int64_t id_begin, int64_t id_end, int k,
                         int chunk, float* values, int64_t* indices, int first, void* workspace, size_t workspace_bytes, void* stream);

/* From encoder outputs to index postings and query batches (csrc/ivf_pack.h, DESIGN.md section 10, "Building postings and query
 * batches"): the per-token loops of the reference's citadel_eval_task.py:43-70 and citadel_retrieval_task.py:104-125 as two operations.
 * dprhot_ivf_compact lists the kept slots of a repr dict.  expert_ids int32 [B, L, K], weights fp32 [B, L, K] or NULL (every weight 1),
 * att uint8 [B, L], row_ids int32 [B] (the corpus id or the query row of a sequence).  Slot (b, t, k) is kept when att[b, t] > 0 and
 * (test_weight == 0 or weight > min_weight; a NaN weight is never kept).  seq_off int32 [B + 1]: seq_off[b] = kept slots of the
 * sequences before b, seq_off[B] = their total n.  Record r is the r-th kept slot in (b, t, k) order: out_expert[r] its expert id,
 * out_row[r] = row_ids[b], out_slot[r] = (b L + t) K + k, out_weight[r] its weight.  Records at or beyond `capacity` (the length of
 * the four record arrays) are not written and the call still returns OK: the caller reads seq_off[B].  One wave per sequence, ranks by
 * ballot: no atomics, every element has one owner, two runs are bit-identical.
 * Limits (DPRHOT_E_INVALID): 1 <= K <= 8, L >= 1, 1 <= B <= 65535, B L K < 2^31.
 * dprhot_ivf_gather writes the weighted vectors of n records: output row i takes record r = perm[i] (r = i when perm is NULL), token
 * row slot[r] / K of repr fp32 [n_rows, d] (row stride repr_ld elements) and weight weights[slot[r]] (1 when NULL):
 *   v = round_prod(w * x)  ->  entry_round == DPRHOT_IVF_ENTRY_FP16: v = fp16(v)  ->  out fp32: v;  out bf16: bf16(v)
 * every rounding to nearest even, the product one plain fp32 multiply; round_prod rounds to prod_round (fp32: nothing); out_kind is
 * DPRHOT_IVF_FP32 or DPRHOT_IVF_BF16.  This is what
 * torch computes on the host for a weight and a row of the dtype prod_round names (their widening to fp32 is exact).  Columns d .. out_ld - 1 are
 * written as zeros; a record outside [0, n) or a slot outside the n_rows K slots gives a row of zeros.  n == 0 launches nothing.
 * Limits (DPRHOT_E_INVALID): d >= 1, out_ld >= d, repr_ld >= d, 1 <= K <= 8, 0 <= n < 2^31, n_rows >= 1. */
#define DPRHOT_IVF_FP32 0
#define DPRHOT_IVF_BF16 1
#define DPRHOT_IVF_FP16 2
#define DPRHOT_IVF_ENTRY_NONE 0
#define DPRHOT_IVF_ENTRY_FP16 1
int dprhot_ivf_compact(const int32_t* expert_ids, const float* weights, const uint8_t* att, const int32_t* row_ids, int B, int L, int K,
                       int test_weight, float min_weight, int32_t* seq_off, int32_t* out_expert, int32_t* out_row, int32_t* out_slot,
                       float* out_weight, int64_t capacity, void* stream);
int dprhot_ivf_gather(const float* repr, int64_t repr_ld, int64_t n_rows, const float* weights, const int32_t* slot, const int64_t* perm,
                      int64_t n, int d, int K, int prod_round, int entry_round, int out_kind, void* out, int64_t out_ld, void* stream);

/* Exhaustive MaxSim search of ColBERT (csrc/colbert.h):
 *   score(n, doc) = POOL over query tokens i < LQ of max(0, max over stored tokens j of doc of <q[n,i], c[doc,j]>),  POOL = sum or max
 * Index (device): token blocks of 16 rows, tok bf16 [n_blk * 16, dp] (dp = d zero-padded to a multiple of 32, 16-byte aligned rows) and
 * doc_blk int64 [corpus_len + 1], non-decreasing block offsets: passage doc owns blocks doc_blk[doc] .. doc_blk[doc + 1], the rows behind
 * its last token are zero (a zero row scores exactly 0, which the clamp makes neutral).  Only attended tokens are stored; a passage
 * without a token scores 0.  q_tok bf16 [nq, LQ, dp], padded query tokens are zero rows.  The clamp makes the score the training and
 * rerank score on any padded batch in which every passage has a padded slot.  A NaN product never wins: its token counts as absent.
 * dprhot_colbert_score WRITES S[n][doc - doc_begin] for doc_begin <= doc < doc_begin + cols <= corpus_len, every cell and nothing else
 * of S [nq, ld].  One owner per cell, query-token terms pooled in one fixed order, no floating-point atomics: two runs are bit-identical
 * and a cell does not depend on the chunk, the id range, the other queries or the other passages.  Offsets are clamped to [0, n_blk]:
 * nothing is read behind row n_blk * 16 - 1.
 * dprhot_colbert_search runs doc ids [id_begin, id_end) in chunks of `chunk` (a multiple of 8): the chunk's scores into the workspace,
 * then the streaming top-k (dprhot_topk_update; dprhot_topk_update_wide for k > 4096) with col_offset = the chunk's first id.  values /
 * indices / first as in dprhot_search: disjoint id ranges may be folded into one result; score descending, ties to the lower doc id.
 * workspace: dprhot_colbert_workspace_bytes(nq, chunk) (+ dprhot_topk_wide_workspace_bytes(nq, k) behind it when k > 4096);
 * DPRHOT_E_WORKSPACE when smaller.
 * Limits (DPRHOT_E_INVALID): 1 <= LQ <= DPRHOT_MAXSIM_MAX_LEN, dp % 32 == 0, corpus_len < 2^31, n_blk < 2^36, 1 <= k <= corpus_len,
 * chunk % 8 == 0, pool one of DPRHOT_POOL_SUM / DPRHOT_POOL_MAX; dp > 768: DPRHOT_E_UNSUPPORTED.  No limit on a passage's length. */
int dprhot_colbert_workspace_bytes(int nq, int chunk, size_t* bytes);
int dprhot_colbert_score(const dprhot_bf16* tok, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok,
                         int nq, int LQ, int pool, int64_t doc_begin, int cols, float* S, int64_t ld, void* stream);
int dprhot_colbert_search(const dprhot_bf16* tok, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok,
                          int nq, int LQ, int pool, int64_t id_begin, int64_t id_end, int k, int chunk, float* values, int64_t* indices,
                          int first, void* workspace, size_t workspace_bytes, void* stream);

/* MaxSim over candidate lists (csrc/colbert_cand.h): the score above for a different, ragged list of passages per
 * query -- the hot path of ColBERT search with centroid pruning.  Index and queries as for dprhot_colbert_score.  Query n owns the
 * entries cand_off[n] .. cand_off[n + 1] of cand_doc int32 [n_cand] (cand_off int64 [nq + 1]); its candidate at POSITION p is
 * cand_doc[cand_off[n] + p].
 * dprhot_colbert_cand_score WRITES S[n][j] for n < nq, j < cols, every cell and nothing else of S [nq, ld].  With p = pos_begin + j: where
 * p is below the query's count and the doc id lies in [0, corpus_len), the cell is score(n, doc), bit for bit the cell
 * dprhot_colbert_score writes for the same query rows and passage rows (the same MFMA operands, k order, fmaxf chain from 0, one owner
 * pooling in ascending token order; no floating-point atomics).  Every other cell is a quiet NaN, "no candidate": both streaming top-k
 * entry points never select a NaN.  A cell depends on its query's and its passage's rows only: not on the window, the rest of the list
 * or the other queries; two runs are bit-identical.
 * Bounds: a query's pair of cand_off is clamped to [0, n_cand] and an end below its begin counts as the begin; a doc id outside the
 * corpus is never used as an index; block offsets are clamped to [0, n_blk], an end below its begin counts as the begin.  Nothing
 * behind tok[n_blk * 16 * dp - 1], cand_doc[n_cand - 1] or doc_blk[corpus_len] is read whatever the lists hold.  n_cand == 0 (cand_doc
 * may then be NULL), a query without candidates and a passage without tokens (score 0) are ordinary inputs.
 * dprhot_colbert_cand_search runs positions [0, max_count) in chunks of `chunk` (a multiple of 8): the chunk's scores into the
 * workspace, then the streaming top-k (dprhot_topk_update; dprhot_topk_update_wide for k > 4096) with col_offset = the chunk's first
 * position, always from an empty state; ONE final launch replaces every selected position of row n by cand_doc[cand_off[n] + position]
 * (-1 stays -1).  Lists sorted ascending and free of duplicates therefore give score descending with ties to the lower doc id; for any
 * other list ties go to the lower POSITION, and a doc id listed twice may be returned twice.  A query with fewer than k candidates ends
 * in -inf / -1.  max_count is the longest list's length (a shorter one only leaves the positions behind it unsearched).
 * workspace: dprhot_colbert_cand_workspace_bytes(nq, chunk) (+ dprhot_topk_wide_workspace_bytes(nq, k) behind it when k > 4096);
 * DPRHOT_E_WORKSPACE when smaller.
 * Limits (DPRHOT_E_INVALID): those of dprhot_colbert_score, plus 0 <= n_cand < 2^40, nq <= 65535, 0 < max_count < 2^31,
 * 0 <= pos_begin, pos_begin + cols < 2^31, 1 <= k <= corpus_len, chunk % 8 == 0; dp > 768: DPRHOT_E_UNSUPPORTED. */
int dprhot_colbert_cand_workspace_bytes(int nq, int chunk, size_t* bytes);
int dprhot_colbert_cand_score(const dprhot_bf16* tok, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok,
                              int nq, int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t pos_begin,
                              int cols, float* S, int64_t ld, void* stream);
int dprhot_colbert_cand_search(const dprhot_bf16* tok, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok,
                               int nq, int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t max_count,
                               int k, int chunk, float* values, int64_t* indices, void* workspace, size_t workspace_bytes, void* stream);

/* Centroid interaction (csrc/colbert_cen.h): every candidate of a list scored approximately, each passage token
 * replaced by its centroid, so that the exact score above is computed for the best few only.  centroids bf16 [C, dp]; per passage the
 * sorted, duplicate-free centroid ids of its stored tokens, doc_cen int32 [n_pairs] under doc_cen_off int64 [corpus_len + 1].
 * dprhot_colbert_cen_table WRITES every cell of T fp32 [nq, C, LT], LT = 16 * ceil(LQ / 16), and nothing else:
 *   T[n][c][i] = <q_tok[n, i], centroid_c> for i < LQ, 0 for LQ <= i < LT
 * each product computed as dprhot_colbert_score computes a token's (the centroid block is the MFMA's A operand, 16 query tokens are B,
 * k-steps ascending from a zero accumulator).
 * dprhot_colbert_cen_score has the window contract of dprhot_colbert_cand_score: it WRITES S[n][j] for n < nq, j < cols, every cell and
 * nothing else of S [nq, ld].  With p = pos_begin + j: where p is below the query's count and the doc id lies in [0, corpus_len), the
 * cell is
 *   approx(n, doc) = POOL over i < LQ of max(0, max over c in doc's list of T[n][c][i])
 * every maximum an fmaxf from a start of 0, ONE owner pooling the LQ terms in ascending token order, no floating-point atomics: bit for
 * bit the cell dprhot_colbert_score writes for an index of the same doc_blk whose token rows are centroids[tok_centroid] (zero rows on
 * padding).  Every other cell is the quiet NaN of dprhot_colbert_cand_score.  A cell depends on its query's table and its passage's
 * list only; two runs are bit-identical.
 * Bounds: a pair of cand_off is clamped to [0, n_cand] and a pair of doc_cen_off to [0, n_pairs], an end below its begin counts as the
 * begin; a doc id outside the corpus is never used as an index; a centroid id outside [0, C) is skipped and never used as an index; an
 * empty list scores 0.  Nothing behind doc_cen[n_pairs - 1], doc_cen_off[corpus_len], cand_doc[n_cand - 1] or T[nq * C * LT - 1] is
 * read whatever the lists hold.  n_pairs == 0 and n_cand == 0 are ordinary inputs (doc_cen / cand_doc may then be NULL).
 * dprhot_colbert_cen_search is dprhot_colbert_cand_search with this score: positions [0, max_count) in chunks, the streaming top-k from
 * an empty state, ONE final launch from positions to doc ids; approx descending, ties to the lower position, -inf / -1 tails.
 * workspace: dprhot_colbert_cen_workspace_bytes(nq, chunk) = dprhot_colbert_workspace_bytes(nq, chunk) (+
 * dprhot_topk_wide_workspace_bytes(nq, k) behind it when k > 4096); DPRHOT_E_WORKSPACE when smaller.
 * Limits (DPRHOT_E_INVALID): 1 <= LQ <= DPRHOT_MAXSIM_MAX_LEN, 1 <= C < 2^31, 1 <= nq <= 65535, dp % 32 == 0 (table), corpus_len < 2^31,
 * 0 <= n_pairs < 2^40, 0 <= n_cand < 2^40, T 16-byte aligned, 0 < max_count < 2^31, 0 <= pos_begin, pos_begin + cols < 2^31,
 * 1 <= k <= corpus_len, chunk % 8 == 0, pool one of DPRHOT_POOL_SUM / DPRHOT_POOL_MAX; dp > 768: DPRHOT_E_UNSUPPORTED. */
int dprhot_colbert_cen_table(const dprhot_bf16* centroids, int C, int dp, const dprhot_bf16* q_tok, int nq, int LQ, float* T, void* stream);
int dprhot_colbert_cen_workspace_bytes(int nq, int chunk, size_t* bytes);
int dprhot_colbert_cen_score(const int64_t* doc_cen_off, const int32_t* doc_cen, int64_t n_pairs, int64_t corpus_len, int C, const float* T,
                             int nq, int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t pos_begin,
                             int cols, float* S, int64_t ld, void* stream);
int dprhot_colbert_cen_search(const int64_t* doc_cen_off, const int32_t* doc_cen, int64_t n_pairs, int64_t corpus_len, int C, const float* T,
                              int nq, int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t max_count,
                              int k, int chunk, float* values, int64_t* indices, void* workspace, size_t workspace_bytes, void* stream);

/* Residual-compressed token index under the pruned search (csrc/colbert_res.h): the ColBERTv2 format.  nbits (NB)
 * in {1, 2, 4}, dp in {32, 64, 96, 128}, rb = dp * NB / 8 bytes per row; ONE bucket set per index, cutoffs fp32 [2^NB - 1] (ascending)
 * and weights fp32 [2^NB].  The block layout is that of dprhot_colbert_score; a token row is tok_centroid int32 [n_blk * 16] (its
 * centroid among centroids bf16 [C, dp]) and res_code uint8 [n_blk * 16, rb] with
 *   code(r, t) = (res_code[r][t * NB / 8] >> (NB * (t mod (8 / NB)))) & (2^NB - 1)        (little-endian inside a byte)
 * The index stands for the dense index
 *   tok[r][t] = 0 <= tok_centroid[r] < C ? bf16_rne(float(centroids[tok_centroid[r]][t]) + weights[code(r, t)]) : 0
 * (ONE fp32 addition, then round to nearest even; non-finite centroids are outside the contract).  A row whose id is negative (padding)
 * or >= C is an exact zero whatever its code bytes hold and its id is never used as an index; every code value decodes.
 * dprhot_colbert_res_encode WRITES every byte of res_code [n_rows, rb] and nothing else, for tok bf16 [n_rows, dp] (any rows, not only
 * a block layout) and their ids tok_centroid [n_rows]:
 *   code(r, t) = number of j with float(tok[r][t]) - float(centroids[tok_centroid[r]][t]) > cutoffs[j]       (one fp32 subtraction)
 * which is torch.bucketize(res, cutoffs) for a non-NaN residual; a NaN residual encodes as 0; a row whose id lies outside [0, C) gets
 * zero bytes.  Two runs are bit-identical.
 * dprhot_colbert_res_score has the contract of dprhot_colbert_cand_score over the decoded index: the same window, the same NaN cells,
 * every other cell bit for bit the cell dprhot_colbert_cand_score writes for `tok` above (the bf16 fed to the MFMA is the decoded
 * row's, in the same k order).  Bounds: those of dprhot_colbert_cand_score; nothing behind res_code[n_blk * 16 * rb - 1],
 * tok_centroid[n_blk * 16 - 1] or centroids[C * dp - 1] is read whatever the index holds.  n_blk == 0 scores 0 for present candidates.
 * dprhot_colbert_res_search is dprhot_colbert_cand_search with this score: positions [0, max_count) through the one chunk driver, the
 * streaming top-k from an empty state (the wide selection above k = 4096), ONE final launch from positions to doc ids.
 * workspace: dprhot_colbert_cand_workspace_bytes(nq, chunk) (+ dprhot_topk_wide_workspace_bytes(nq, k) behind it when k > 4096);
 * DPRHOT_E_WORKSPACE when smaller.
 * Limits (DPRHOT_E_INVALID): those of dprhot_colbert_cand_score / _search, plus nbits in {1, 2, 4}, C >= 1, dp % 32 == 0, non-NULL
 * centroids / weights / cutoffs / tok_centroid (with n_blk > 0 / n_rows > 0), res_code, tok and centroids 16-byte aligned,
 * 0 <= n_rows < 2^40; dp > 128: DPRHOT_E_UNSUPPORTED. */
int dprhot_colbert_res_encode(const dprhot_bf16* tok, const int32_t* tok_centroid, int64_t n_rows, int dp, const dprhot_bf16* centroids,
                              int C, const float* cutoffs, int nbits, uint8_t* res_code, void* stream);
int dprhot_colbert_res_score(const uint8_t* res_code, const int32_t* tok_centroid, const dprhot_bf16* centroids, int C, const float* weights,
                             int nbits, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok, int nq,
                             int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t pos_begin, int cols,
                             float* S, int64_t ld, void* stream);
int dprhot_colbert_res_search(const uint8_t* res_code, const int32_t* tok_centroid, const dprhot_bf16* centroids, int C, const float* weights,
                              int nbits, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok, int nq,
                              int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t max_count, int k,
                              int chunk, float* values, int64_t* indices, void* workspace, size_t workspace_bytes, void* stream);

/* Product-quantised token index for the ColBERT search (csrc/colbert_pq.h).  dsub in {2, 4, 8}, m = dp / dsub,
 * dp in {32, 64, 96, 128}, ONE codebook bf16 [m, 256, dsub] per index (the layout and the decode rule of the product-quantised postings
 * above).  The block layout is that of dprhot_colbert_score; a token row is m code bytes, tok_code uint8 [n_blk * 16, m], and blk_rows
 * uint8 [n_blk] is the number of real token rows of every block (above 16 counts as 16).  The index stands for the dense index
 *   tok[r, j * dsub + t] = (r mod 16) < blk_rows[r / 16] ? codebook[j, tok_code[r, j], t] : 0
 * (a row at or behind blk_rows is an exact zero whatever its code bytes hold), and dprhot_colbert_pq_score / dprhot_colbert_pq_search
 * return, bit for bit, what dprhot_colbert_score / dprhot_colbert_search return over it: owners, order of additions, chunks, ties, NaN
 * and the workspace (dprhot_colbert_workspace_bytes) are unchanged.  No byte behind tok_code[n_blk * 16 * m - 1] or blk_rows[n_blk - 1]
 * is read.  n_blk == 0 scores 0 everywhere (tok_code and blk_rows may then be NULL).
 * dprhot_colbert_pq_encode is dprhot_pq_encode (same rule, same kernel) for rows of dp <= 128.
 * Limits: those of the dense entry points; dsub not in {2, 4, 8}, dp % 32 != 0, a NULL codebook, a NULL blk_rows with n_blk > 0, a
 * tok_code or codebook that is not 16-byte aligned: DPRHOT_E_INVALID; dp > 128: DPRHOT_E_UNSUPPORTED. */
int dprhot_colbert_pq_encode(const dprhot_bf16* vec, int64_t n, int dp, const dprhot_bf16* codebook, int dsub, uint8_t* codes,
                             void* stream);
int dprhot_colbert_pq_score(const uint8_t* tok_code, const uint8_t* blk_rows, const dprhot_bf16* codebook, int dsub, const int64_t* doc_blk,
                            int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok, int nq, int LQ, int pool,
                            int64_t doc_begin, int cols, float* S, int64_t ld, void* stream);
int dprhot_colbert_pq_search(const uint8_t* tok_code, const uint8_t* blk_rows, const dprhot_bf16* codebook, int dsub, const int64_t* doc_blk,
                             int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok, int nq, int LQ, int pool,
                             int64_t id_begin, int64_t id_end, int k, int chunk, float* values, int64_t* indices, int first,
                             void* workspace, size_t workspace_bytes, void* stream);

/* SPAR retrieval (spar/spar_retrieval.py, spar_weight_tuning.py; csrc/spar.h): a dense retriever and a lexical
 * model searched together, for a whole grid of weights in one pass over the corpus.  Two resident indexes C1 bf16 [n_ctx, d1] and
 * C2 bf16 [n_ctx, d2] (passage id = row), queries Q1 bf16 [nq, d1] and Q2 bf16 [nq, d2], row-major without padding between rows,
 * d1 and d2 positive multiples of 32 (pad with zeros), weights lam fp32 [W] on the HOST (passed to the kernel by value), 1 <= W <= 32:
 *   s[w][i][j] = fmaf(lam[w], <Q2[i], C2[j]>, <Q1[i], C1[j]>)
 * bf16 products, fp32 accumulators, ONE fp32 fma per score.  The order of the additions inside the two dot products is fixed: a score
 * depends on its four rows and lam[w] only, and has the same bits whether dprhot_spar_score stores it or dprhot_spar_search ranks it.
 * dprhot_spar_score WRITES S[w * nq + i][j - doc_begin] for doc_begin <= j < doc_begin + cols <= n_ctx, every cell and nothing else of
 * S [W * nq, ld] (ld >= cols, ld % 8 == 0).
 * dprhot_spar_search folds passage ids [id_begin, id_end) into values / indices [W * nq, k] (row w * nq + i): total order, `first`,
 * the -inf / -1 unfilled tail and "a NaN is never selected" as in dprhot_topk_update; disjoint id ranges may be folded into one result,
 * which for every w equals dprhot_topk over the dprhot_spar_score matrix of those ranges bit for bit.  k <= 1024: the first chunk of an
 * empty state is materialised and selected from, every other chunk leaves the GEMM tile as candidate lists (only scores that rank ahead
 * of their row's k-th entry) which the streaming top-k merges; k > 1024: every chunk is materialised (k > 4096: the HBM-resident
 * selection).  workspace: dprhot_spar_workspace_bytes(nq, W, chunk) (+ dprhot_topk_wide_workspace_bytes(W * nq, k) behind it when
 * k > 4096); DPRHOT_E_WORKSPACE when smaller.
 * Limits (DPRHOT_E_INVALID): NULL or not 16-byte aligned pointers, d1 / d2 % 32, W outside 1 .. 32, a non-finite weight, W * nq >= 2^31,
 * W * nq * chunk >= 2^40, not 0 <= id_begin < id_end <= n_ctx < 2^31, not 1 <= k <= n_ctx, chunk % 8. */
int dprhot_spar_workspace_bytes(int nq, int W, int chunk, size_t* bytes);
int dprhot_spar_score(const dprhot_bf16* Q1, const dprhot_bf16* Q2, int nq, int d1, int d2, const dprhot_bf16* C1, const dprhot_bf16* C2,
                      int64_t n_ctx, const float* lam, int W, int64_t doc_begin, int cols, float* S, int64_t ld, void* stream);
int dprhot_spar_search(const dprhot_bf16* Q1, const dprhot_bf16* Q2, int nq, int d1, int d2, const dprhot_bf16* C1, const dprhot_bf16* C2,
                       int64_t n_ctx, const float* lam, int W, int64_t id_begin, int64_t id_end, int k, int chunk, float* values,
                       int64_t* indices, int first, void* workspace, size_t workspace_bytes, void* stream);

/* The fp8 dense index (csrc/dense_fp8.h; dpr_scale_amd/dense_fp8.py): a dense corpus as OCP e4m3fn codes
 * (NOT the fnuz form) with one power-of-two fp32 scale per row, d + 4 bytes per passage instead of 2 d.  codes uint8 [n, dp],
 * dp = round_up(d, 32), the features behind d are code 0x00; scale fp32 [n].  With amax = max |x_t| = f * 2^p (1 <= f < 2):
 * e = p - 8 + (f > 1.75 ? 1 : 0) clamped to [-64, 64] and scale = 2^e, the smallest power of two with amax <= 448 * scale, read off the
 * float's bits; code_t = e4m3fn(x_t / scale), an exact division, rounded to nearest even, saturating at +-448 (which only the clamp can
 * make happen); -0 stays -0; a row with amax == 0 has scale 1; a row with a non-finite element has scale NaN and codes 0x00.  Every
 * decoded value value(code) * scale of a finite row is exact in bf16.
 * dprhot_fp8_encode: rows fp32 (is_bf16 = 0) or bf16 (1) [n, d], row-major without padding -> codes [n, dp] (the zero padding included)
 * and scale [n].  Queries are quantised by the same rule.
 *   s[i][j] = (acc[i][j] * qs[i]) * cs[j],   acc[i][j] = sum_t value(Qc[i][t]) * value(Cc[j][t])
 * acc is accumulated in fp32 by the MFMA unit, t ascending; two fp32 multiplies follow.  A score depends on its two code rows and its two
 * scales only, and has the same bits whether dprhot_dense_fp8_score stores it or dprhot_dense_fp8_search ranks it.  A NaN scale or a NaN
 * code (0x7F / 0xFF) makes its scores NaN; a NaN is never selected.
 * dprhot_dense_fp8_score WRITES S[i][j - doc_begin] for doc_begin <= j < doc_begin + cols <= n_ctx, every cell and nothing else of
 * S [nq, ld] (ld >= cols, ld % 8 == 0).
 * dprhot_dense_fp8_search folds passage ids [id_begin, id_end) into values / indices [nq, k]: total order, `first`, the -inf / -1
 * unfilled tail and "a NaN is never selected" as in dprhot_topk_update; disjoint id ranges may be folded into one result, which equals
 * dprhot_topk over the dprhot_dense_fp8_score matrix of those ranges bit for bit.  k <= 1024: the first chunk of an empty state is
 * materialised and selected from, every other chunk leaves the tile as candidate lists which the streaming top-k merges; k > 1024: every
 * chunk is materialised (k > 4096: the HBM-resident selection).  workspace: dprhot_dense_fp8_workspace_bytes(nq, chunk), which equals
 * dprhot_search_workspace_bytes(nq, chunk) (+ dprhot_topk_wide_workspace_bytes(nq, k) behind it when k > 4096); DPRHOT_E_WORKSPACE when
 * smaller.
 * Limits (DPRHOT_E_INVALID): NULL pointers, code rows / S / workspace not 16-byte aligned, dp % 32, d outside 1 .. dp, nq < 1,
 * nq * chunk >= 2^40, not 0 <= id_begin < id_end <= n_ctx < 2^31, not 1 <= k <= n_ctx, chunk % 8. */
int dprhot_fp8_encode(const void* rows, int is_bf16, int64_t n, int d, int dp, uint8_t* codes, float* scale, void* stream);
int dprhot_dense_fp8_workspace_bytes(int nq, int chunk, size_t* bytes);
int dprhot_dense_fp8_score(const uint8_t* Qc, const float* qs, int nq, const uint8_t* Cc, const float* cs, int64_t n_ctx, int dp,
                           int64_t doc_begin, int cols, float* S, int64_t ld, void* stream);
int dprhot_dense_fp8_search(const uint8_t* Qc, const float* qs, int nq, const uint8_t* Cc, const float* cs, int64_t n_ctx, int dp,
                            int64_t id_begin, int64_t id_end, int k, int chunk, float* values, int64_t* indices, int first, void* workspace,
                            size_t workspace_bytes, void* stream);

/* The CITADEL / SPLADE encoder head behind the MLM logits (dpr_scale/models/citadel_models/citadel_model.py:46-82, splade_model.py:26-32;
 * csrc/router_head.h), forward and backward without a [B, T, V] temporary.  logits [B, T1, V] of `dtype` (0 bf16,
 * 1 fp16, 2 fp32) with unit column stride and ELEMENT strides stride_b / stride_t (a [:, 1:, :] view or a column slice of a wider buffer
 * passes as it is; nothing beyond the element's own alignment is assumed); mask uint8 [B, T1] (non-zero = a real token).  The first
 * `skip` token rows take no part; T = T1 - skip; x[b,t,v] = logits[b, t + skip, v], m[b,t] = mask[b, t + skip]:
 *   f               = m ? log(1 + relu(x)) : 0                        (fp32; a NaN logit gives f = 0)
 *   router_repr     [B, V]      max_t f, argmax [B, V] int32 its token (the lowest t among equals)
 *   expert_weights, expert_ids [B, T, k] (ids int32)   the k largest f of the row: value descending, then column ascending, zeros
 *                               included (a masked token gets columns 0 .. k-1 with weight 0); k = 0: none (SPLADE), the pointers may be NULL
 *   router_mask     [B, V]      how many (t, j) route to the column with a weight > 0
 *   softmax_sum     [B, V]      sum_t softmax_v(x[b,t,:]), padded tokens included; only with want_softmax (else it may be NULL)
 * Float outputs are of `dtype`, computed in fp32.  The workspace (dprhot_router_head_workspace_bytes(B, T, V, k, want_softmax); 0 bytes and
 * NULL allowed without want_softmax) keeps the rows' logsumexp for the backward: leave it unchanged until then.
 * Backward: dlogits [B, T1, V] contiguous, of `dtype`, every element written once (rows below `skip` are zeros):
 *   dlogits[b, t + skip, v] = (g_router_repr[b,v] [t == argmax[b,v]] + sum_j g_expert_weights[b,t,j] [v == expert_ids[b,t,j]]) m (x > 0) / (1 + x)
 *                           + p (g_softmax_sum[b,v] - sum_u p[b,t,u] g_softmax_sum[b,u]),   p = softmax_v(x[b,t,:])
 * The three incoming gradients are fp32 and each may be NULL; without g_softmax_sum there is no reduction and the logits are read only
 * where a gradient lands.  No floating-point atomics: two runs are bit-identical.
 * Limits (DPRHOT_E_INVALID): 0 <= k <= 8, V >= max(k, 1), T >= 1 (skip <= T1 - 1), B <= 65535, stride_t >= V. */
int dprhot_router_head_workspace_bytes(int B, int T, int V, int k, int want_softmax, size_t* bytes);
int dprhot_router_head_fwd(const void* logits, int dtype, int B, int T1, int V, int64_t stride_b, int64_t stride_t, const uint8_t* mask,
                           int skip, int k, int want_softmax, void* router_repr, int32_t* argmax, void* expert_weights,
                           int32_t* expert_ids, void* router_mask, void* softmax_sum, void* workspace, size_t workspace_bytes,
                           void* stream);
int dprhot_router_head_bwd(const void* logits, int dtype, int B, int T1, int V, int64_t stride_b, int64_t stride_t, const uint8_t* mask,
                           int skip, int k, const int32_t* argmax, const int32_t* expert_ids, const void* workspace,
                           size_t workspace_bytes, const float* g_router_repr, const float* g_expert_weights, const float* g_softmax_sum,
                           void* dlogits, void* stream);

/* The step as the autograd operator of dpr_scale_amd/hotpath.py runs it (dpr_task.py:197-212 + its backward inside the forward call):
 * dprhot_inbatch_step_f32 / _packed_f32 with
 *   loss_scale   loss_out[0] = loss_scale * sum_i row_loss[i]: pass 1 / Nq_global and the mean of dpr_task.py:212 leaves the kernel
 *                ready (and the stamp of the packed form carries that value)
 *   d_scale      DEVICE scalar the gradients are scaled by (required): the grad_output the caller expects backward() to deliver
 *   dq_part      NULL, or -- when dprhot_train_dq_slabs(B, Nc, d) = n > 0 -- a caller buffer [n][B][d] fp32: the step then leaves
 *                dQ as n unscaled split-K partial slabs there (dQ itself untouched) and skips its own reduction launch; the
 *                caller's dprhot_rescale_grads forms dQ from them (the operator's backward launches that anyway)
 *   dC_part      fp32 (dc_kind = 2), or bf16 (dc_kind = 0: the wire format of the reduce-scatter written by the dC epilogue itself,
 *                no loss stamp; DPRHOT_E_UNSUPPORTED at shapes whose plan has no such epilogue -- the caller then asks for fp32)
 * No S_out, no h_scale (= 1). */
int dprhot_train_dq_slabs(int B, int Nc, int d, int* h_nslabs);
int dprhot_train_step_f32(const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d, const int64_t* y,
                          int64_t y_offset, const uint8_t* colmask, float inv_T, float grad_scale, float loss_scale, const float* d_scale,
                          float* row_loss, float* row_lse, float* loss_out, dprhot_bf16* G, float* dQ, float* dq_part, void* dC_part,
                          int dc_kind, void* workspace, size_t workspace_bytes, void* stream);
int dprhot_train_step_packed_f32(const float* q, const dprhot_bf16* gathered, dprhot_bf16* Qb, int B, int W, int rank, int n_ctx, int d,
                                 const int64_t* y, float inv_T, float grad_scale, float loss_scale, const float* d_scale, float* row_loss,
                                 float* row_lse, float* loss_out, dprhot_bf16* G, float* dQ, float* dq_part, void* dC_part, int dc_kind,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* backward() of that operator: the gradients were computed for grad_output = *used; the autograd engine delivers *go.
 *   nslabs > 0         dQ[0..n_dq) = *go * sum of the nslabs slabs of dq_part, in slab order (bit-reproducible)
 *   if (*go != *used)  dQ (nslabs == 0) and dC[0..n_dc) are multiplied by *go / *used   (AMP's loss scale changes once in thousands
 *                      of steps; otherwise their workgroups read two floats and leave)
 *   out2[0] = *go   (what the gradients are now scaled by)
 *   out2[1] = *go if it is a finite, normal, non-zero number, else 1   (the d_scale the next forward should expect)
 * out2 is a fresh 2-float buffer (never go / used).  dQ fp32, dC fp32 (dc_kind 2) or bf16 (0); either may be NULL with count 0;
 * counts are multiples of 8. */
int dprhot_rescale_grads(float* dQ, size_t n_dq, const float* dq_part, int nslabs, void* dC, size_t n_dc, int dc_kind, const float* go,
                         const float* used, float* out2, void* stream);

/* Gradient all-reduce of the encoder towers (reference: dpr_scale/task/dpr_task.py:90-92 registers torch's fp16_compress_hook on
 * the DDP model: bucket -> fp16 -> ONE ring all-reduce -> fp32).  The hook of dpr_scale_amd/comm_hooks.py moves a bucket as
 *   pack -> all-to-all (every pair of GPUs owns an xGMI link) -> sum of the W received shards in fp32 -> all-gather -> unpack;
 * these are its three local legs, one pass over HBM each.  Wire kinds: 0 = bf16 (RNE), 1 = fp16 (RNE, the reference's), 2 = fp32.
 *   dprhot_grad_pack        send[i] = wire(bucket[i] * scale) for i < n, 0 for n <= i < n_padded (n_padded % 8 == 0; = W * shard)
 *   dprhot_grad_sum_shards  out[i] = sum_r recv[r * shard + i], fp32 accumulation in rank order r = 0 .. W-1 (deterministic), ONE
 *                           rounding into out_kind (= wire kind, or 2 for an fp32 return leg); shard % 8 == 0
 *   dprhot_grad_unpack      bucket[i] = float(full[i]) for i < n (kind of `full` = the return leg's) */
int dprhot_grad_pack(const float* bucket, size_t n, float scale, int wire, void* send, size_t n_padded, void* stream);
int dprhot_grad_sum_shards(const void* recv, int W, size_t shard, int wire, int out_kind, void* out, void* stream);
int dprhot_grad_unpack(const void* full, int kind, float* bucket, size_t n, void* stream);

/* Optional communicator: the collectives of the path (dpr_task.py:166-176 gathers; the autograd split of :192-195)
 * issued directly on the caller's stream through the RCCL library already present in the process (dlopen; no
 * link-time dependency) instead of through torch.distributed -- no stream hand-over, ~3x less host time per call.
 *   dprhot_comm_unique_id   rank 0: 128-byte id to be handed to every rank (any side channel)
 *   dprhot_comm_init        COLLECTIVE over the W ranks, on the current HIP device; *h is the communicator handle
 *   dprhot_allgather_ctx    recv[r * bytes_per_rank ...] = rank r's send  (the packed context buffer of dprhot_pack_ctx)
 *   dprhot_reducescatter_dc recv[0 .. count_per_rank) = sum over ranks of send[rank * count_per_rank ...]  (fp32 dC partials)
 *   dprhot_reducescatter_rows the same for dC partials of any storage kind (0 bf16, 1 fp16, 2 fp32: the wire formats of the backward)
 *   dprhot_allreduce_sum    in place, fp32 (the loss numerator)
 *   dprhot_allgather_allpairs      the same result as dprhot_allgather_ctx by a DIRECT ALL-PAIRS exchange: one grouped send / receive of
 *                                  the one send buffer to / from every peer (SURVEY 8(e) "Topology": on the fully connected node every
 *                                  pair of GPUs owns an xGMI link, so the W - 1 transfers use W - 1 links at once instead of a ring's
 *                                  W - 1 sequential hops)
 *   dprhot_reducescatter_allpairs  the same result as dprhot_reducescatter_rows: chunk k of send goes to rank k, the W chunks received
 *                                  land in tmp [W * count_per_rank] (caller-owned, storage kind `kind`), then ONE kernel adds them in
 *                                  fp32 in rank order (deterministic; a half-width wire is rounded once per partial, never inside the
 *                                  sum) into recv, stored as `out_kind` (= kind, or 2 for fp32)
 *   dprhot_comm_has_allpairs       LOCAL, no communication: 1 when this process's RCCL has ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd
 *                                  (the two all-pairs entry points would run), 0 when not -- what a rank checks BEFORE its peers enter a
 *                                  send / receive group (dist.try_direct_comm, dist.choose_path_collectives)
 * One communicator per rank process, used from one thread; every rank issues the same calls in the same order. */
int dprhot_comm_unique_id(void* id128);
int dprhot_comm_init(const void* id128, int W, int rank, void** h);
int dprhot_comm_destroy(void* h);
int dprhot_allgather_ctx(void* h, const void* send, void* recv, size_t bytes_per_rank, void* stream);
int dprhot_reducescatter_dc(void* h, const float* send, float* recv, size_t count_per_rank, void* stream);
int dprhot_reducescatter_rows(void* h, const void* send, void* recv, size_t count_per_rank, int kind, void* stream);
int dprhot_allreduce_sum(void* h, float* buf, size_t count, void* stream);
int dprhot_allgather_allpairs(void* h, const void* send, void* recv, size_t bytes_per_rank, void* stream);
int dprhot_reducescatter_allpairs(void* h, const void* send, void* tmp, void* recv, size_t count_per_rank, int kind, int out_kind, void* stream);
int dprhot_comm_has_allpairs(void* h);

#ifdef __cplusplus
}
#endif
#endif /* DPRHOT_H */
