"""TEST-ONLY `kernels` stand-in for ColBERT search with centroid pruning (dpr_scale_amd/colbert.py) on CPU
tensors: the dense stand-in of tests/_colbert_oracle.py plus the three colbert_cand_* methods by their definitions in float64, and the
dense search methods CorpusSearch calls (tests/_oracle_kernels.py) so that assignment and probing take the product's route.

Also the host-side restatements the CPU and GPU tests compare with: the inverted lists from tok_centroid, the union of probed lists and
the total-order top-k of a score matrix restricted to a candidate list."""
import torch

import _colbert_oracle as CO
from _oracle_kernels import OracleKernels

NAN = float("nan")


def ranges(cand_off, n_cand):
    """[(lo, hi)] per query: a pair of cand_off clamped to [0, n_cand], an end below its begin counts as the begin."""
    off = [min(max(int(v), 0), int(n_cand)) for v in cand_off.tolist()]
    return [(a, max(a, b)) for a, b in zip(off, off[1:])]


class ColbertCandKernels(CO.ColbertKernels, OracleKernels):
    name = "colbert-cand-test-standin"

    def colbert_cand_workspace(self, nq, chunk, k, like):
        assert chunk > 0 and chunk % 8 == 0
        return torch.empty(0, dtype=torch.uint8)

    def colbert_cand_score(self, index, q, pool, cand_off, cand_doc, pos_begin, cols, S):
        assert q.dtype == torch.bfloat16 and q.shape[2] == index.dp and cand_off.dtype == torch.int64 and cand_doc.dtype == torch.int32
        q64, tok, blk, docs = q.double(), index.tok.double(), index.doc_blk.tolist(), cand_doc.tolist()
        for n, (lo, hi) in enumerate(ranges(cand_off, len(docs))):
            for j in range(cols):
                p = pos_begin + j
                doc = docs[lo + p] if p < hi - lo else -1
                if 0 <= doc < index.corpus_len:
                    S[n, j] = CO.doc_score(q64[n:n + 1], tok[blk[doc] * 16: blk[doc + 1] * 16], pool).float()
                else:
                    S[n, j] = NAN

    def colbert_cand_search(self, index, q, pool, cand_off, cand_doc, max_count, values, indices, chunk, ws):
        assert chunk > 0 and chunk % 8 == 0 and max_count > 0
        nq, k = values.shape
        S = torch.empty((nq, max_count), dtype=torch.float32)
        self.colbert_cand_score(index, q, pool, cand_off, cand_doc, 0, max_count, S)
        v, i = topk_of_positions(S, k, cand_off, cand_doc)
        values.copy_(v)
        indices.copy_(i)


def topk_of_positions(S, k, cand_off, cand_doc):
    """(values [nq, k], doc ids int64 [nq, k]) of a candidate score matrix S [nq, max_count] (NaN: no candidate): score descending,
    ties to the lower position, then positions mapped to doc ids; a row with fewer than k candidates ends in -inf / -1."""
    S, cand_off, cand_doc = S.cpu(), cand_off.cpu(), cand_doc.cpu()
    nq = S.shape[0]
    values = torch.full((nq, k), float("-inf"), dtype=S.dtype)
    ids = torch.full((nq, k), -1, dtype=torch.int64)
    for n, (lo, hi) in enumerate(ranges(cand_off, cand_doc.shape[0])):
        pos = torch.nonzero(~torch.isnan(S[n])).reshape(-1)
        order = pos[torch.sort(S[n, pos], descending=True, stable=True).indices[:k]]
        values[n, : order.shape[0]] = S[n, order]
        ids[n, : order.shape[0]] = cand_doc[lo + order].long()
    return values, ids


def lists_from_assignment(tok_centroid, doc_blk, n_centroids):
    """(cen_off, cen_doc) as Python lists from tok_centroid on the host: per centroid the sorted set of passages with a token there."""
    blk, tc = doc_blk.tolist(), tok_centroid.tolist()
    sets = [set() for _ in range(n_centroids)]
    for doc in range(len(blk) - 1):
        for r in range(blk[doc] * 16, blk[doc + 1] * 16):
            if tc[r] >= 0:
                sets[tc[r]].add(doc)
    off, docs = [0], []
    for s in sets:
        docs += sorted(s)
        off.append(len(docs))
    return off, docs


def union_of_lists(probed, live, cen_off, cen_doc):
    """(cand_off, cand_doc) as Python lists: per query the sorted union of the lists of the centroids its live tokens probe.  probed
    int64 [nq, LQ, nprobe], live bool [nq, LQ]."""
    off, docs = [0], []
    cen_off, cen_doc = [int(v) for v in cen_off], [int(v) for v in cen_doc]
    for n in range(probed.shape[0]):
        s = set()
        for i in range(probed.shape[1]):
            if live[n, i]:
                for c in probed[n, i].tolist():
                    s.update(cen_doc[cen_off[c]:cen_off[c + 1]])
        docs += sorted(s)
        off.append(len(docs))
    return off, docs
