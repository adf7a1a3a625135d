/*
 * dprhot_union.h -- the candidate stage of ColBERT search with centroid pruning (csrc/colbert_union.h): per
 * query the sorted, duplicate-free union of the inverted lists of the centroids its tokens probe, built by kernels.  The entry points
 * are exported by libdprhot.so next to those of dprhot.h and follow that header's conventions to the letter: device pointers owned by
 * the caller, status codes and dprhot_last_error(), host-side validation before any launch, no allocation, and the stream contract -- a
 * call only enqueues kernel launches on `stream` (no memset, no copy), does not synchronise, reads every loop bound that lives in
 * device memory on the device, every time, and may be captured into a HIP graph after one eager call at the same shape
 * (tests/test_colbert_union_gpu.py holds both stream-taking entry points to this).  DPRHOT_VERSION is that of dprhot.h.
 *
 * Inputs   cids int64 [nq, LQ, nprobe]   the probed centroid ids of every query token
 *          q_tok bf16 [nq, LQ, dp]       the query tokens: token (n, i) is LIVE when any of its dp features is not zero -- a NaN is not
 *                                        zero, -0.0 is zero; a token that is not live (padding) probes nothing
 *          cen_off int64 [C + 1], cen_doc int32 [n_list]   per centroid its list of doc ids (any order, duplicates allowed)
 * The set of query n: the doc ids in [0, corpus_len) of the lists of every id in [0, C) that a live token of n probes.  Ids outside
 * [0, C) are skipped (the -1 that the probe gives a NaN token among them); a pair of cen_off is clamped to [0, n_list] and an end below
 * its begin counts as the begin; a doc id outside [0, corpus_len) is skipped and never used as an index.  Nothing behind
 * cen_doc[n_list - 1] is read whatever the tensors hold.
 *
 * dprhot_colbert_union_count WRITES cand_off int64 [nq + 1] (cand_off[0] = 0, then the running set sizes) and totals int64 [2] =
 * (n_cand = cand_off[nq], the largest set size), and nothing else outside the workspace.  It leaves the membership state in the
 * workspace -- one bit per (query, doc id) and prefix counts per block of 8192 doc ids -- which arrives with arbitrary contents: the
 * call clears what it needs itself.  Membership is set by an idempotent vector atomic OR, so the result does not depend on the order in
 * which lanes meet and two runs are bit-identical.
 * dprhot_colbert_union_fill READS the state that the _count call before it left in the same workspace (same nq, same corpus_len) and
 * WRITES query n's set, doc ids ascending, at cand_doc[cand_off[n] ..].  n_cand is a CAPACITY: nothing at or behind cand_doc[n_cand]
 * (and nothing before cand_doc[0]) is written, a query whose range would cross the capacity is truncated there, and the entries between
 * cand_off[nq] and n_cand are left alone.  With a caller-chosen capacity the pair therefore runs without a host read of `totals` and
 * replays in a graph on other inputs.
 *
 * workspace: dprhot_colbert_union_workspace_bytes(nq, corpus_len), monotone in both; 16-byte aligned.  DPRHOT_E_WORKSPACE when smaller.
 * Limits (DPRHOT_E_INVALID): 1 <= nq <= 65535, 1 <= LQ <= DPRHOT_MAXSIM_MAX_LEN, nprobe >= 1, 1 <= C < 2^31, 1 <= corpus_len < 2^31,
 * 0 <= n_list < 2^40 (cen_doc may be NULL at 0), dp a positive multiple of 32, 0 <= n_cand < 2^40 (cand_doc may be NULL at 0), non-NULL
 * pointers, a workspace that is not 16-byte aligned.  nq * LQ * nprobe >= 2^33 (more waves than one launch has): DPRHOT_E_UNSUPPORTED.
 */
#ifndef DPRHOT_UNION_H
#define DPRHOT_UNION_H

#include "dprhot.h"

#ifdef __cplusplus
extern "C" {
#endif

int dprhot_colbert_union_workspace_bytes(int nq, int64_t corpus_len, size_t* bytes);
int dprhot_colbert_union_count(const int64_t* cids, const dprhot_bf16* q_tok, int dp, int nq, int LQ, int nprobe, int C, const int64_t* cen_off,
                               const int32_t* cen_doc, int64_t n_list, int64_t corpus_len, int64_t* cand_off, int64_t* totals, void* workspace,
                               size_t workspace_bytes, void* stream);
int dprhot_colbert_union_fill(int nq, int64_t corpus_len, const int64_t* cand_off, int32_t* cand_doc, int64_t n_cand, const void* workspace,
                              size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DPRHOT_UNION_H */
