"""TEST-ONLY CPU stand-in for HipKernels.ivf_workspace / ivf_score / ivf_search, built on the float64 oracle (tests/_ivf_oracle.py),
so that the CPU suite can drive IVFIndex.search and the drop-in CITADELRetrievalTask: the chunk loop, the folding of disjoint doc-id
ranges, the CLS part and the top-k order.  It unpacks the device layout back into the dictionaries the oracle takes."""
import numpy as np
import torch

import _ivf_oracle as O


def unpack_index(index):
    off = index.exp_off.tolist()
    post = {}
    for e in range(index.n_experts):
        a, b = off[e], off[e + 1]
        if b > a:
            post[e] = (index.post_doc[a:b].long().numpy(), index.post_vec[a:b].float().numpy())
    return post


def unpack_queries(qb):
    queries = [dict() for _ in range(qb.nq)]
    boff = qb.boff.tolist()
    for j, e in enumerate(qb.bexp.tolist()):
        for i in range(boff[j], boff[j + 1]):
            queries[int(qb.ent_q[i])].setdefault(e, []).append(qb.ent_vec[i].float())
    return queries


class IvfKernels:
    name = "ivf-test-standin"

    def __init__(self):
        self.calls = []

    def ivf_workspace(self, nq, n_entries, chunk, has_cls, k, like):
        return torch.empty(nq * chunk * 4, dtype=torch.uint8)

    def _scores(self, index, qb):
        cq = None if qb.cls is None else qb.cls.float()
        cd = None if index.cls is None else index.cls[: index.corpus_len].float()
        return O.score_matrix(unpack_index(index), unpack_queries(qb), index.corpus_len, cq, cd)

    def ivf_score(self, index, qb, doc_begin, cols, S):
        full = O.score_matrix(unpack_index(index), unpack_queries(qb), index.corpus_len)
        S[:, :cols] += torch.from_numpy(full[:, doc_begin:doc_begin + cols]).float()

    def ivf_search(self, index, qb, id_begin, id_end, values, indices, first, chunk, ws):
        assert chunk % 8 == 0 and 0 <= id_begin < id_end <= index.corpus_len
        full = self._scores(index, qb)
        if first:
            values.fill_(float("-inf"))
            indices.fill_(-1)
        k = values.shape[1]
        for j0 in range(id_begin, id_end, chunk):
            j1 = min(j0 + chunk, id_end)
            self.calls.append((j0, j1))
            v = np.concatenate([values.double().numpy(), full[:, j0:j1]], 1)
            i = np.concatenate([indices.numpy(), np.broadcast_to(np.arange(j0, j1), (qb.nq, j1 - j0))], 1)
            for n in range(qb.nq):
                valid = np.nonzero(i[n] >= 0)[0]
                order = valid[np.lexsort((i[n][valid], -v[n][valid]))][:k]
                values[n] = float("-inf")
                indices[n] = -1
                values[n, : len(order)] = torch.from_numpy(v[n][order]).float()
                indices[n, : len(order)] = torch.from_numpy(i[n][order])
