"""TEST-ONLY `kernels` stand-in for the fp8 dense index (dpr_scale_amd/dense_fp8.py) on CPU tensors: fp8_encode / dense_fp8_workspace /
dense_fp8_score / dense_fp8_search by their definitions -- the encode rule and the float64 score of tests/_fp8_oracle.py, the score
rounded to fp32 once, folded with the total-order top-k of tests/_topk_oracle.py.  It inherits the dense stand-in
(tests/_oracle_kernels.py), so hotpath.CorpusSearch runs on it as well."""
import numpy as np
import torch

import _fp8_oracle as FO
import _topk_oracle as TO
from _oracle_kernels import OracleKernels


class DenseFP8Kernels(OracleKernels):
    name = "dense-fp8-test-standin"

    def __init__(self):
        self.calls = []  # (method, rows) of every call

    def fp8_encode(self, rows, codes, scale):
        assert rows.dtype in (torch.float32, torch.bfloat16) and rows.dim() == 2 and rows.is_contiguous()
        assert codes.dtype == torch.uint8 and codes.shape == (rows.shape[0], FO.padded_width(rows.shape[1])) and scale.shape == (rows.shape[0],)
        self.calls.append(("encode", rows.shape[0]))
        c, s = FO.encode(rows.float().numpy())
        codes.copy_(torch.from_numpy(c))
        scale.copy_(torch.from_numpy(s))

    def dense_fp8_workspace(self, nq, chunk, k, like):
        assert chunk > 0 and chunk % 8 == 0
        return torch.empty(0, dtype=torch.uint8)

    def _scores(self, index, qc, qs, doc_begin, cols):
        assert qc.dtype == torch.uint8 and qs.dtype == torch.float32 and qc.shape[1] == index.codes.shape[1] and qc.shape[1] % 32 == 0
        rows = slice(doc_begin, doc_begin + cols)
        with np.errstate(over="ignore"):
            return FO.score(qc.numpy(), qs.numpy(), index.codes[rows].numpy(), index.scale[rows].numpy()).astype(np.float32)

    def dense_fp8_score(self, index, qc, qs, doc_begin, cols, S):
        self.calls.append(("score", cols))
        S[:, :cols] = torch.from_numpy(self._scores(index, qc, qs, doc_begin, cols))

    def dense_fp8_search(self, index, qc, qs, id_begin, id_end, values, indices, first, chunk, ws):
        self.calls.append(("search", id_end - id_begin))
        k = values.shape[1]
        state = None if first else (values.numpy(), indices.numpy())
        for j0 in range(id_begin, id_end, chunk):
            cols = min(chunk, id_end - j0)
            state = TO.fold(state, self._scores(index, qc, qs, j0, cols), j0, k)
        values.copy_(torch.from_numpy(state[0]))
        indices.copy_(torch.from_numpy(state[1]))
