"""TEST-ONLY `kernels` stand-in for the centroid-interaction stage of the pruned ColBERT search (dpr_scale_amd/colbert.py, DESIGN.md
section 12.3) on CPU tensors: the candidate stand-in of tests/_colbert_cand_standin.py plus the four colbert_cen_* methods by their
definitions in float64, a cell rounded to fp32 once.

Also the host-side restatements the CPU and GPU tests compare with: the per-passage centroid lists from tok_centroid, the passages with
every token replaced by its centroid, and the approximate score of one list from a table."""
import torch

import _colbert_cand_standin as CS

NAN = float("nan")


def doc_lists_from_assignment(tok_centroid, doc_blk):
    """(doc_cen_off, doc_cen) as Python lists from tok_centroid on the host: per passage the sorted set of its tokens' centroids."""
    blk, tc = doc_blk.tolist(), tok_centroid.tolist()
    off, cen = [0], []
    for doc in range(len(blk) - 1):
        cen += sorted({tc[r] for r in range(blk[doc] * 16, blk[doc + 1] * 16) if tc[r] >= 0})
        off.append(len(cen))
    return off, cen


def centroid_passages(index):
    """The passages of `index` with every stored token replaced by its centroid: a list of float32 [len_i, d] row tensors."""
    blk, tc, cen = index.doc_blk.tolist(), index.tok_centroid.cpu().long(), index.centroids.cpu().float()[:, :index.d]
    out = []
    for doc in range(index.corpus_len):
        mine = tc[blk[doc] * 16: blk[doc + 1] * 16]
        out.append(cen[mine[mine >= 0]])
    return out


def approx_of_list(T64, ids, LQ, pool):
    """float64 scalar: POOL_i max(0, max over the centroid ids (those outside [0, C) skipped) of T64[c, i]) for one query's table
    T64 [C, LT]."""
    ids = [c for c in ids if 0 <= c < T64.shape[0]]
    m = torch.zeros(LQ, dtype=torch.float64)
    if ids:
        rows = T64[ids, :LQ]
        rows = torch.where(torch.isnan(rows), torch.full_like(rows, float("-inf")), rows)
        m = rows.max(0).values.clamp(min=0.0)
    return m.sum() if pool in ("sum", 0) else m.max()


class ColbertCenKernels(CS.ColbertCandKernels):
    name = "colbert-cen-test-standin"

    def colbert_cen_workspace(self, nq, chunk, k, like):
        assert chunk > 0 and chunk % 8 == 0
        return torch.empty(0, dtype=torch.uint8)

    def colbert_cen_table(self, index, q, T):
        nq, LQ, dp = q.shape
        assert q.dtype == torch.bfloat16 and dp == index.dp and T.dtype == torch.float32
        assert T.shape == (nq, index.centroids.shape[0], (LQ + 15) // 16 * 16)
        T.zero_()
        T[:, :, :LQ] = torch.einsum("nid,cd->nci", q.double(), index.centroids.double()).float()

    def colbert_cen_score(self, index, T, LQ, pool, cand_off, cand_doc, pos_begin, cols, S):
        assert T.dtype == torch.float32 and T.shape[2] == (LQ + 15) // 16 * 16 and cand_off.dtype == torch.int64 and cand_doc.dtype == torch.int32
        doc_cen_off, doc_cen = index.doc_centroids()
        assert doc_cen_off.dtype == torch.int64 and doc_cen_off.shape == (index.corpus_len + 1,) and doc_cen.dtype == torch.int32
        cen, docs, T64 = doc_cen.tolist(), cand_doc.tolist(), T.double()
        mine = CS.ranges(doc_cen_off, len(cen))  # a pair of doc_cen_off is read as a pair of cand_off is
        for n, (lo, hi) in enumerate(CS.ranges(cand_off, len(docs))):
            for j in range(cols):
                p = pos_begin + j
                doc = docs[lo + p] if p < hi - lo else -1
                if 0 <= doc < index.corpus_len:
                    S[n, j] = approx_of_list(T64[n], cen[mine[doc][0]:mine[doc][1]], LQ, pool).float()
                else:
                    S[n, j] = NAN

    def colbert_cen_search(self, index, T, LQ, pool, cand_off, cand_doc, max_count, values, indices, chunk, ws):
        assert chunk > 0 and chunk % 8 == 0 and max_count > 0
        nq, k = values.shape
        S = torch.empty((nq, max_count), dtype=torch.float32)
        self.colbert_cen_score(index, T, LQ, pool, cand_off, cand_doc, 0, max_count, S)
        v, i = CS.topk_of_positions(S, k, cand_off, cand_doc)
        values.copy_(v)
        indices.copy_(i)
