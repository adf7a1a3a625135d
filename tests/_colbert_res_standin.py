"""TEST-ONLY `kernels` stand-in for the residual-compressed ColBERT index (dpr_scale_amd/colbert.py) on CPU
tensors: the centroid-interaction stand-in of tests/_colbert_cen_standin.py plus the colbert_res_* methods, which decode the index with
the rule of section 12.4 restated here in torch, feature by feature, and call the inherited candidate stand-in on the decoded rows.

Also the restatements of the encode and the decode rule the CPU and GPU tests compare with (they run on any device)."""
import types

import torch

import _colbert_cen_standin as CEN

BF16 = torch.bfloat16


def code_of(res_code, t, nbits):
    """int64 [n]: feature t's code, (res_code[r, t * NB / 8] >> (NB * (t mod (8 / NB)))) & (2^NB - 1)."""
    return (res_code[:, t * nbits // 8].to(torch.int64) >> (nbits * (t % (8 // nbits)))) & ((1 << nbits) - 1)


def decode_rule(res_code, tok_centroid, centroids, weights, nbits):
    """bf16 [n, dp]: bf16(float(centroids[tok_centroid[r], t]) + weights[code(r, t)]) where 0 <= tok_centroid[r] < C, else 0."""
    C, dp = centroids.shape
    tc = tok_centroid.to(torch.int64)
    ok = (tc >= 0) & (tc < C)
    out = torch.zeros((res_code.shape[0], dp), dtype=BF16, device=res_code.device)
    cen = centroids.float()[tc[ok]]
    for t in range(dp):
        out[ok, t] = (cen[:, t] + weights[code_of(res_code[ok], t, nbits)]).to(BF16)
    return out


def encode_rule(rows, tok_centroid, centroids, cutoffs, nbits):
    """uint8 [n, dp * NB / 8]: code = number of j with float(row) - float(centroid) > cutoffs[j] (NaN: 0), packed little-endian inside a
    byte; zero bytes for a row whose id lies outside [0, C)."""
    C, dp = centroids.shape
    tc = tok_centroid.to(torch.int64)
    ok = (tc >= 0) & (tc < C)
    out = torch.zeros((rows.shape[0], dp * nbits // 8), dtype=torch.int64, device=rows.device)
    res = rows.float()[ok] - centroids.float()[tc[ok]]
    for t in range(dp):
        code = (res[:, t].unsqueeze(1) > cutoffs.unsqueeze(0)).sum(1)
        out[ok, t * nbits // 8] |= code << (nbits * (t % (8 // nbits)))
    return out.to(torch.uint8)


def decoded(index):
    """What the candidate stand-in reads of a dense index, for the decoded rows of a ColBERTResidualIndex."""
    tok = decode_rule(index.res_code, index.tok_centroid, index.centroids, index.weights, index.nbits)
    return types.SimpleNamespace(tok=tok, doc_blk=index.doc_blk, corpus_len=index.corpus_len, dp=index.dp)


class ColbertResKernels(CEN.ColbertCenKernels):
    name = "colbert-res-test-standin"

    def colbert_res_workspace(self, nq, chunk, k, like):
        return self.colbert_cand_workspace(nq, chunk, k, like)

    def colbert_res_encode(self, rows, cutoffs, nbits, tok_centroid=None, centroids=None):
        if tok_centroid is None:
            rows, tok_centroid, centroids = rows.tok, rows.tok_centroid, rows.centroids
        assert rows.dtype == BF16 and centroids.dtype == BF16 and tok_centroid.dtype == torch.int32 and cutoffs.dtype == torch.float32
        assert tok_centroid.shape == (rows.shape[0],) and cutoffs.shape == ((1 << nbits) - 1,)
        return encode_rule(rows, tok_centroid, centroids, cutoffs, nbits)

    def colbert_res_score(self, index, q, pool, cand_off, cand_doc, pos_begin, cols, S):
        self.colbert_cand_score(decoded(index), q, pool, cand_off, cand_doc, pos_begin, cols, S)

    def colbert_res_search(self, index, q, pool, cand_off, cand_doc, max_count, values, indices, chunk, ws):
        self.colbert_cand_search(decoded(index), q, pool, cand_off, cand_doc, max_count, values, indices, chunk, ws)
