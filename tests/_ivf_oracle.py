"""TEST-ONLY checker of the inverted-index retrieval score, in float64, from the UNPACKED structures:

    postings   {expert_id: (ids int64 [n], reprs [n, d])}          what the index files hold
    queries    [ {expert_id: [vector, ...]}, ... ]                 what the retrieval task hands to index.search
    score(n, doc) = sum over entries (e, u) of query n of max(0, max over postings (doc, v) of expert e of <u, v>) + <cls_q[n], cls_doc[doc]>

An entry whose expert has no posting for a doc adds 0; every doc id in [0, corpus_len) has a score.  `bf16=True` rounds every operand
to bf16 first (round to nearest even), which is what the HIP path computes from.  Nothing here knows the packed device layout.

Non-finite products ("Limits"): with p the fp64 dot product of an entry and a posting,

    contribution of the entry to a doc = max over the doc's postings of (p if p > 0 else 0)

so a NaN product counts as absent (it fails `p > 0`, whatever else the doc holds), a +inf product is positive and is added (the cell
becomes +inf), -inf adds 0 -- and whether a doc HAS a posting (m, A below) is decided by the posting, not by the product's value."""
import numpy as np
import torch


def _r(x, bf16):
    t = torch.as_tensor(np.asarray(x, dtype=np.float32) if not torch.is_tensor(x) else x).float()
    if bf16:
        t = t.to(torch.bfloat16).float()
    return t.double().numpy()


def score_matrix(postings, queries, corpus_len, cls_q=None, cls_doc=None, bf16=False, return_abs=False):
    """[nq, corpus_len] float64.  With return_abs also (A, m): A[n, doc] = sum over the entries of the |u_k v_k| sum of the winning
    posting (0 for a clamped entry, the largest such sum among the doc's postings otherwise: an upper bound for the error model) and
    m[n, doc] = number of entries of n that have a posting for doc."""
    nq = len(queries)
    S = np.zeros((nq, corpus_len), np.float64)
    A = np.zeros((nq, corpus_len), np.float64)
    m = np.zeros((nq, corpus_len), np.int64)
    post = {int(e): (np.asarray(ids, dtype=np.int64), _r(v, bf16)) for e, (ids, v) in postings.items()}
    for n, by_expert in enumerate(queries):
        for e, vecs in by_expert.items():
            if int(e) not in post:
                continue
            ids, V = post[int(e)]
            for u in vecs:
                u = _r(u, bf16).reshape(-1)
                with np.errstate(invalid="ignore"):  # (inf x 0 and inf - inf are NaN products, by the rule above)
                    dots = V @ u
                    absd = np.abs(V) @ np.abs(u)  # (A is an error model for finite operands; a NaN operand makes it a NaN)
                best = np.zeros(corpus_len)
                np.maximum.at(best, ids, np.where(dots > 0, dots, 0.0))  # (NaN > 0 is False: nothing folded here is a NaN)
                babs = np.zeros(corpus_len)
                with np.errstate(invalid="ignore"):
                    np.maximum.at(babs, ids, absd)
                has = np.zeros(corpus_len, dtype=bool)
                has[ids] = True
                S[n, has] += best[has]
                A[n, has] += babs[has]
                m[n, has] += 1
    if cls_q is not None and len(cls_q):
        cq, cd = _r(cls_q, bf16), _r(cls_doc, bf16)
        S += cq @ cd.T
        A += np.abs(cq) @ np.abs(cd).T
    return (S, A, m) if return_abs else S


def topk(S, k):
    """(scores [nq, k], ids [nq, k]): score descending, ties by lower doc id."""
    ids = np.stack([np.lexsort((np.arange(S.shape[1]), -row))[:k] for row in S])
    return np.take_along_axis(S, ids, 1), ids


def search(postings, queries, corpus_len, k, cls_q=None, cls_doc=None, bf16=False):
    return topk(score_matrix(postings, queries, corpus_len, cls_q, cls_doc, bf16), k)
