"""TEST-ONLY `kernels` stand-in for the product-quantised ColBERT index (dpr_scale_amd/colbert.py) on CPU
tensors: the three kernel methods by their definitions -- encode is tests/_pq_oracle.py, score and search decode the index
(pq_decode, rows at or behind blk_rows zero) and call the dense stand-in of tests/_colbert_oracle.py."""
import torch

import _colbert_oracle as CO
import _pq_oracle as PO
from dpr_scale_amd import ivf


GPU_LENGTHS = [0, 1, 15, 16, 17, 31, 33, 64, 65, 180, 513] + [1 + (7 * j) % 12 for j in range(40)]  # block edges, many tiles, 40 short ones


def grid_corpus(dsub, d=128, lengths=GPU_LENGTHS, nq=3, LQ=33, seed=0):
    """(q [nq, LQ, d], passages: a list of [len, d] rows) with every feature on a grid of 256 ** (1 / dsub) levels (2, 4 or 16 bf16-exact
    values): no subspace of `dsub` features has more than 256 distinct sub-vectors, so a codebook can hold them all."""
    levels = {2: 16, 4: 4, 8: 2}[dsub]
    g = torch.Generator().manual_seed(seed + dsub)
    draw = lambda *shape: (torch.randint(0, levels, shape, generator=g).float() - levels / 2 + 0.5) / (levels / 2)
    q = draw(nq, LQ, d)
    q[0, LQ - 2:] = 0.0
    return q, [draw(n, d) for n in lengths]


class _Decoded:
    """What ColbertKernels.colbert_score reads of an index: tok, doc_blk, n_blk, dp."""

    def __init__(self, index):
        tok = ivf.pq_decode(index.tok_code, index.codebook)
        rows = index.blk_rows.long().clamp(max=16)
        tok[(torch.arange(16).unsqueeze(0) >= rows.unsqueeze(1)).reshape(-1)] = 0
        self.tok, self.doc_blk, self.n_blk, self.dp = tok, index.doc_blk, index.n_blk, index.dp


class ColbertPQKernels(CO.ColbertKernels):
    name = "colbert-pq-test-standin"

    def colbert_pq_encode(self, vec, codebook):
        assert vec.dtype == torch.bfloat16 and codebook.dtype == torch.bfloat16 and vec.shape[1] == codebook.shape[0] * codebook.shape[2]
        return torch.from_numpy(PO.encode(vec.float().numpy(), codebook.float().numpy()))

    def colbert_pq_score(self, index, q, pool, doc_begin, cols, S):
        self.colbert_score(_Decoded(index), q, pool, doc_begin, cols, S)

    def colbert_pq_search(self, index, q, pool, *tail):
        self.colbert_search(_Decoded(index), q, pool, *tail)
