"""TEST-ONLY checker of the ColBERT retrieval score (dpr_scale_amd/colbert.py): a float64 restatement on
bf16-rounded operands, the total-order top-k, a seeded generator of padded batches and a `kernels` stand-in built on the restatement so
that the CPU suite can drive ColBERTIndex, the builder, load_index and the tasks.

    score(n, doc) = POOL_i max(0, max_j <q[n, i], c[doc, j]>)   over the stored (attended) tokens j; a NaN product counts as absent
"""
import numpy as np
import torch

POOL = {"sum": 0, "max": 1}


def bf16(x):
    return torch.as_tensor(x).to(torch.bfloat16).double()


def doc_score(q64, c64, pool):
    """[nq] float64: queries q64 [nq, LQ, d] against ONE passage's stored rows c64 [len, d]."""
    if c64.shape[0] == 0:
        return torch.zeros(q64.shape[0], dtype=torch.float64)
    s = torch.einsum("nid,jd->nij", q64, c64)
    s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
    m = s.max(-1).values.clamp(min=0.0)
    return m.sum(1) if pool in ("sum", 0) else m.max(1).values


def score(q, passages, pool="sum"):
    """float64 [nq, len(passages)]: q [nq, LQ, d], passages a list of [len_i, d] row tensors (doc id = list position)."""
    q64 = bf16(q)
    return torch.stack([doc_score(q64, bf16(c).reshape(-1, q64.shape[2]), pool) for c in passages], 1)


def magnitude(q, passages):
    """A[n, doc] = sum_i max_j sum_k |q_ik c_jk| (float64): what the rounding bound of a cell scales with."""
    q64 = bf16(q).abs()
    cols = []
    for c in passages:
        c64 = bf16(c).reshape(-1, q64.shape[2]).abs()
        cols.append(torch.einsum("nid,jd->nij", q64, c64).max(-1).values.sum(1) if c64.shape[0] else torch.zeros(q64.shape[0], dtype=torch.float64))
    return torch.stack(cols, 1)


def topk(S, k, col_offset=0):
    """(values [rows, k], ids int64 [rows, k]) by the total order: score descending, ties to the lower id."""
    order = torch.sort(S, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(S, 1, order), order + col_offset


def passages_of(c, att):
    """The stored rows of a padded batch c [N, LD, d], att [N, LD]: the slots with attention > 0, in order."""
    return [c[i][att[i] > 0] for i in range(c.shape[0])]


def make_padded(seed, nq, LQ, N, LD, d, lengths=None, q_pad=1, grid=True):
    """(q [nq, LQ, d], c [N, LD, d], att int64 [N, LD]) as ColBERT's encoders return them: padded slots are zero rows.  Every passage
    has at least one padded slot (asserted): the condition under which the retrieval score is the training / rerank score.  The last
    `q_pad` tokens of query 0 are padding.  grid: multiples of 1/4 in [-1, 1] (every score exact in fp32), else bf16-rounded gaussians."""
    g = np.random.default_rng(seed)

    def feats(n, L):
        if grid:
            return g.integers(-4, 5, size=(n, L, d)).astype(np.float32) / 4.0
        return torch.from_numpy(g.standard_normal((n, L, d)).astype(np.float32)).to(torch.bfloat16).float().numpy()

    q, c = feats(nq, LQ), feats(N, LD)
    if q_pad:
        q[0, LQ - q_pad:] = 0.0
    lens = np.asarray(lengths if lengths is not None else g.integers(0, LD, size=N))
    assert lens.shape == (N,) and lens.min() >= 0 and lens.max() <= LD - 1, "every passage needs at least one padded slot"
    att = (np.arange(LD)[None, :] < lens[:, None]).astype(np.int64)
    c = c * att[..., None]
    assert (att.sum(1) < LD).all()
    return torch.from_numpy(q), torch.from_numpy(c.astype(np.float32)), torch.from_numpy(att)


class ColbertKernels:
    """Stand-in for HipKernels.colbert_workspace / colbert_score / colbert_search on CPU tensors: reads the packed layout (tok, doc_blk) of
    a ColBERTIndex, scores in float64 and rounds a cell to fp32 once."""

    name = "colbert-test-standin"

    def colbert_workspace(self, nq, chunk, k, like):
        assert chunk > 0 and chunk % 8 == 0
        return torch.empty(0, dtype=torch.uint8)

    def colbert_score(self, index, q, pool, doc_begin, cols, S):
        assert q.dtype == torch.bfloat16 and q.shape[2] == index.dp and index.tok.shape[0] == index.n_blk * 16
        q64, tok, blk = q.double(), index.tok.double(), index.doc_blk.tolist()
        assert blk[0] == 0 and blk[-1] == index.n_blk and all(a <= b for a, b in zip(blk, blk[1:]))
        for j in range(cols):
            doc = doc_begin + j
            S[:, j] = doc_score(q64, tok[blk[doc] * 16: blk[doc + 1] * 16], pool).float()

    def colbert_search(self, index, q, pool, id_begin, id_end, values, indices, first, chunk, ws):
        k = values.shape[1]
        for j0 in range(id_begin, id_end, chunk):
            cols = min(chunk, id_end - j0)
            S = torch.empty((q.shape[0], cols), dtype=torch.float32)
            self.colbert_score(index, q, pool, j0, cols, S)
            ids = torch.arange(j0, j0 + cols).expand(q.shape[0], cols)
            if not (first and j0 == id_begin):
                S, ids = torch.cat([values, S], 1), torch.cat([indices, ids], 1)
            if S.shape[1] < k:  # fewer candidates than k so far: -inf / -1 fill, as the streaming top-k keeps them
                pad = k - S.shape[1]
                S = torch.cat([S, torch.full((S.shape[0], pad), float("-inf"))], 1)
                ids = torch.cat([ids, torch.full((ids.shape[0], pad), -1, dtype=torch.int64)], 1)
            # total order: score descending, then id ascending
            by_id = torch.sort(ids, dim=1, stable=True)
            S, ids = torch.gather(S, 1, by_id.indices), by_id.values
            order = torch.sort(S, dim=1, descending=True, stable=True).indices[:, :k]
            values.copy_(torch.gather(S, 1, order))
            indices.copy_(torch.gather(ids, 1, order))
