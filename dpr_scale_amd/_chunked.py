"""What the device-resident indexes (ivf.py, colbert.py) share: the kernel table, the chunk size and the walk over doc-id ranges that
folds every range into one running top-k.  The chunk loop inside a range is the library's (the chunk driver of csrc/dprhot.hip)."""
import collections

import torch


def _default_kernels(kernels):
    if kernels is None:
        from . import hotpath

        kernels = hotpath.default_kernels()
    return kernels


class ChunkedIndex:
    """Base of an index that is searched chunk by chunk.  A subclass sets `device` and `corpus_len` and calls `_init_search`."""

    def _init_search(self, chunk, kernels):
        self.chunk = None if chunk is None else int(chunk)
        self.kn = kernels
        self.latency = collections.defaultdict(float)
        self.latency["encode_time"] += 0.0  # test_epoch_end of the retrieval task pops this key

    def _kernels(self):
        self.kn = _default_kernels(self.kn)
        return self.kn

    def default_chunk(self, nq):
        """Doc ids per pass: the chunk's score buffer is nq x chunk fp32 (at most 8 MiB by default, at least 1024 ids)."""
        c = self.chunk if self.chunk is not None else max(1024, min(262144, (1 << 21) // max(nq, 1)))
        c = min(c, (self.corpus_len + 7) // 8 * 8)
        return max(8, c // 8 * 8)

    def _fold(self, nq, topk, id_ranges, chunk, workspace, search):
        """(values fp32 [nq, topk], indices int64 [nq, topk]) over the disjoint (begin, end) doc-id ranges (default: the whole corpus).
        workspace(chunk) allocates what search(begin, end, values, indices, first, chunk, ws) needs; the first range starts the state."""
        if not 1 <= topk <= self.corpus_len:
            raise ValueError(f"topk={topk} out of range (1 .. corpus_len={self.corpus_len})")
        chunk =self.default_chunk(nq) if chunk is None else int(chunk)
        values = torch.empty((nq, topk), dtype=torch.float32, device=self.device)
        indices = torch.empty((nq, topk), dtype=torch.int64, device=self.device)
        ws = workspace(chunk)
        first = True
        for b, e in (id_ranges if id_ranges is not None else [(0, self.corpus_len)]):
            search(int(b), int(e), values, indices, first, chunk, ws)
            first = False
        return values, indices
