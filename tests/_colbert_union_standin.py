"""TEST-ONLY `kernels` stand-in for the candidate stage of the pruned ColBERT search on CPU tensors: the
stand-in of tests/_colbert_cand_standin.py plus the three colbert_union_* methods written from their definition with Python sets, as
`union_of_lists` is -- the rules of include/dprhot_union.h included: live tokens, ids outside [0, C), clamped list offsets, doc ids
outside the corpus, and the capacity rule of the fill.  The "workspace" is a Python list that holds one sorted list per query.

`clean_lists` restates the contract's reading of hostile inputs as well-formed ones, so that `union_of_lists` can be the oracle of the
GPU tests on those inputs too."""
import torch

from _colbert_cand_standin import ColbertCandKernels


def clean_lists(cen_off, cen_doc, C, corpus_len):
    """(cen_off, cen_doc) as Python lists for C + 1 centroids: per centroid the entries the contract reads -- its pair of offsets
    clamped to [0, n_list], an end below its begin counting as the begin, doc ids outside [0, corpus_len) dropped -- and an EMPTY list
    number C, where `clean_ids` sends every id outside [0, C)."""
    off_in, doc_in = [int(v) for v in cen_off], [int(v) for v in cen_doc]
    n_list = len(doc_in)
    off, docs = [0], []
    for c in range(C):
        lo, hi = (min(max(v, 0), n_list) for v in off_in[c:c + 2])
        docs += [d for d in doc_in[lo:max(lo, hi)] if 0 <= d < corpus_len]
        off.append(len(docs))
    return off + [len(docs)], docs


def clean_ids(cids, C):
    """Probed ids with everything outside [0, C) replaced by C, the empty list of `clean_lists`."""
    return torch.where((cids >= 0) & (cids < C), cids, torch.full_like(cids, C))


def live_tokens(qb):
    """bool [nq, LQ]: any feature of the token is not zero (a NaN is not zero, -0.0 is)."""
    return (qb != 0).any(2)


class ColbertUnionKernels(ColbertCandKernels):
    name = "colbert-union-test-standin"

    def colbert_union_workspace(self, nq, corpus_len, like):
        assert nq >= 1 and corpus_len >= 1
        return []

    def colbert_union_count(self, index, cids, qb, cand_off, totals, ws):
        nq, LQ, _ = qb.shape
        assert cids.dtype == torch.int64 and cids.shape[:2] == (nq, LQ) and qb.dtype == torch.bfloat16
        assert cand_off.dtype == torch.int64 and cand_off.shape == (nq + 1,) and totals.dtype == torch.int64 and totals.shape == (2,)
        C = int(index.cen_off.shape[0]) - 1
        off, docs = clean_lists(index.cen_off.tolist(), index.cen_doc.tolist(), C, index.corpus_len)
        live, ids = live_tokens(qb).tolist(), clean_ids(cids, C).tolist()
        del ws[:]
        for n in range(nq):
            s = set()
            for i in range(LQ):
                if live[n][i]:
                    for c in ids[n][i]:
                        s.update(docs[off[c]:off[c + 1]])
            ws.append(sorted(s))
        sizes = [len(s) for s in ws]
        cand_off[0] = 0
        cand_off[1:] = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0)
        totals[0], totals[1] = sum(sizes), max(sizes)

    def colbert_union_fill(self, index, cand_off, cand_doc, ws):
        assert cand_off.dtype == torch.int64 and cand_doc.dtype == torch.int32 and len(ws) == cand_off.shape[0] - 1
        cap = int(cand_doc.shape[0])
        for n, s in enumerate(ws):
            at = int(cand_off[n])
            for j, doc in enumerate(s):
                if 0 <= at + j < cap:  # the capacity: nothing at or behind cand_doc[cap] is written
                    cand_doc[at + j] = doc
