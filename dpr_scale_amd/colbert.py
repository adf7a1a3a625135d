"""End-to-end retrieval for ColBERT: an exhaustive MaxSim search over a device-resident token index.

    score(n, doc) = POOL over query tokens i < LQ of  max(0, max over stored tokens j of doc of <q[n, i], c[doc, j]>)
    POOL = sum (query_pool="sum") or max (query_pool="max")

Only tokens with attention > 0 are stored; a passage without a stored token scores 0.  The clamp at 0 is what makes the score the
training and rerank score (hotpath.expert_sim_score / expert_score_only on a ColBERT repr dict): the reference multiplies token vectors
by the attention mask, so a padded slot enters its max as a dot product of exactly 0 -- the scores are equal on any padded batch in
which every passage has at least one padded slot (the rule and the condition of DESIGN.md section 10).  Padded query tokens are zero rows
and add 0, so a query batch is a dense [nq, LQ, d] block without a mask.

Device layout (csrc/colbert.h): token blocks of 16 rows, `tok` bf16 [n_blk * 16, dp] with dp = d zero-padded to a multiple of 32, and
`doc_blk` int64 [corpus_len + 1] block offsets; the rows behind a passage's last token are zero, which the clamp makes neutral.  Passages
may have any length.  On disk: `tokens_{rank:04}.pkl`, a protocol-4 pickle of (ids int64 [n], lengths int32 [n], reprs bfloat16
[sum(lengths), d]) -- the vectors are stored as the bf16 that is searched, so a loaded index searches bit-identically to one built in
memory, however the passages were split over ranks.

Precision: operands are rounded to bf16 once (round to nearest even); products are exact in fp32 and accumulation is fp32.  Scoring and
top-k run in libdprhot.so (dprhot_colbert_search); there is no torch fallback.  `kernels` is the injection point of ivf.py.

Not supported (out of scope): compressed or residual token vectors, centroid pruning (PLAID-style candidate generation), an index
across several GPUs, a CPU index.
"""
import glob
import os
import pickle
import time

import torch

from ._chunked import ChunkedIndex

_BF16 = torch.bfloat16
_POOL = {"sum": 0, "max": 1}  # DPRHOT_POOL_SUM / DPRHOT_POOL_MAX
BLOCK = 16                    # token rows per block: one MFMA fragment, one passage
MAX_QUERY_LEN = 512           # DPRHOT_MAXSIM_MAX_LEN


def _bf16_padded(x, dp):
    """bf16 image of rows x [..., d], zero-padded to dp columns."""
    d = x.shape[-1]
    if d == dp:
        return x.to(_BF16).contiguous()
    out = torch.zeros(x.shape[:-1] + (dp,), dtype=_BF16, device=x.device)
    out[..., :d].copy_(x)
    return out


class ColBERTIndex(ChunkedIndex):
    """Device-resident token index of a ColBERT corpus; `search` is the exhaustive MaxSim top-k."""

    def __init__(self, doc_ids, lengths, rows, corpus_len, device, chunk=None, kernels=None):
        """From unpadded token rows grouped by passage: doc_ids int64 [n], lengths [n] (tokens of each passage), rows [sum(lengths), d]
        in the order of doc_ids.  Ids that never appear get zero blocks; an id given twice is a ValueError."""
        corpus_len = int(corpus_len)
        if not 0 < corpus_len < 2 ** 31:
            raise ValueError(f"corpus_len={corpus_len} out of range (1 .. 2^31 - 1)")
        device = torch.device(device)
        ids = torch.as_tensor(doc_ids).reshape(-1).to(device, torch.int64)
        lens = torch.as_tensor(lengths).reshape(-1).to(device, torch.int64)
        rows = torch.as_tensor(rows).to(device)
        if rows.dim() != 2 or ids.shape != lens.shape:
            raise ValueError(f"ids {tuple(ids.shape)}, lengths {tuple(lens.shape)} and rows {tuple(rows.shape)} do not belong together")
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= corpus_len or int(lens.min()) < 0):
            raise ValueError("doc ids must lie in [0, corpus_len) and lengths must be non-negative")
        if int(lens.sum()) != rows.shape[0]:
            raise ValueError(f"{rows.shape[0]} token rows for lengths that sum to {int(lens.sum())}")
        seen = torch.bincount(ids, minlength=corpus_len)
        if ids.numel() and int(seen.max()) > 1:
            raise ValueError(f"doc id {int(torch.nonzero(seen > 1)[0])} appears more than once")
        d = int(rows.shape[1])
        dp = (max(d, 1) + 31) // 32 * 32
        doc_len = torch.zeros(corpus_len, dtype=torch.int64, device=device)
        doc_len[ids] = lens
        doc_blk = torch.zeros(corpus_len + 1, dtype=torch.int64, device=device)
        torch.cumsum((doc_len + (BLOCK - 1)) // BLOCK, 0, out=doc_blk[1:])
        n_blk = int(doc_blk[-1])
        tok = torch.zeros((n_blk * BLOCK, dp), dtype=_BF16, device=device)
        if rows.shape[0]:
            start = torch.cumsum(lens, 0) - lens              # first input row of every listed passage
            first = doc_blk[ids] * BLOCK - start              # + input row number = the row in `tok`
            dest = torch.arange(rows.shape[0], device=device) + torch.repeat_interleave(first, lens)
            tok[dest, :d] = rows.to(_BF16)
        self._set(tok, doc_blk, corpus_len, d, chunk, kernels)

    @classmethod
    def from_packed(cls, tok, doc_blk, corpus_len, d, chunk=None, kernels=None):
        """From tensors already in the device layout (csrc/colbert.h), on their device: tok bf16 [n_blk * 16, dp], doc_blk int64
        [corpus_len + 1]."""
        self = cls.__new__(cls)
        self._set(tok, doc_blk, int(corpus_len), int(d), chunk, kernels)
        return self

    @classmethod
    def from_repr(cls, expert_repr, attention, corpus_ids, corpus_len, device=None, chunk=None, kernels=None):
        """From a padded batch: expert_repr [N, LD, d], attention [N, LD]; the slots with attention > 0 are kept, in order."""
        device = expert_repr.device if device is None else device
        ids, lens, rows = _kept_rows(expert_repr, attention, corpus_ids)
        return cls(ids, lens, rows, corpus_len, device, chunk=chunk, kernels=kernels)

    def _set(self, tok, doc_blk, corpus_len, d, chunk, kernels):
        assert tok.dtype == _BF16 and doc_blk.dtype == torch.int64 and tok.dim() == 2 and tok.shape[1] % 32 == 0 and tok.shape[0] % BLOCK == 0
        assert doc_blk.shape[0] == corpus_len + 1 and tok.is_contiguous() and doc_blk.is_contiguous()
        self.device = doc_blk.device
        self.tok, self.doc_blk = tok, doc_blk
        self.corpus_len, self.d, self.dp = corpus_len, d, int(tok.shape[1])
        self.n_blk = int(tok.shape[0]) // BLOCK
        self._init_search(chunk, kernels)

    @property
    def nbytes(self):
        """Bytes of device memory the index holds (token rows and block offsets)."""
        return sum(t.numel() * t.element_size() for t in (self.tok, self.doc_blk))

    def _queries(self, q):
        if isinstance(q, dict):
            q = q["expert_repr"]
        q = q.detach()
        if q.dim() != 3 or q.shape[0] == 0:
            raise ValueError(f"queries {tuple(q.shape)}; [nq, LQ, d] with nq >= 1 expected")
        if q.shape[2] != self.d:
            raise ValueError(f"query tokens of {q.shape[2]} features, index of {self.d}")
        if not 1 <= q.shape[1] <= MAX_QUERY_LEN:
            raise ValueError(f"{q.shape[1]} query tokens; 1 .. {MAX_QUERY_LEN} are supported")
        return _bf16_padded(q.to(self.device), self.dp)

    @staticmethod
    def _pool(query_pool):
        if query_pool not in _POOL:
            raise NotImplementedError("Invalid query pooling! Available: [max, sum]")
        return _POOL[query_pool]

    def search(self, q, topk, query_pool="sum", id_ranges=None, chunk=None):
        """(scores fp32 [nq, topk], ids int64 [nq, topk]) on the index's device, score descending with ties to the lower doc id.  q:
        [nq, LQ, d] or a repr dict with `expert_repr`.  `id_ranges`: disjoint (begin, end) doc-id ranges folded into one result."""
        pool, topk = self._pool(query_pool), int(topk)
        tic = time.perf_counter()
        qb = self._queries(q)
        self.latency["encode_time"] += time.perf_counter() - tic
        tic = time.perf_counter()
        kn = self._kernels()
        nq = int(qb.shape[0])
        out = self._fold(nq, topk, id_ranges, chunk, lambda chunk: kn.colbert_workspace(nq, chunk, topk, self.doc_blk),
                         lambda *tail: kn.colbert_search(self, qb, pool, *tail))
        self.latency["search_time"] += time.perf_counter() - tic
        return out

    def score(self, q, doc_begin=0, cols=None, query_pool="sum"):
        """The score matrix fp32 [nq, cols] of doc ids doc_begin .. doc_begin + cols (default: to the end of the corpus)."""
        pool, doc_begin = self._pool(query_pool), int(doc_begin)
        cols = self.corpus_len - doc_begin if cols is None else int(cols)
        if doc_begin < 0 or cols < 1 or doc_begin + cols > self.corpus_len:
            raise ValueError(f"doc ids {doc_begin} .. +{cols} outside the corpus of {self.corpus_len}")
        qb = self._queries(q)
        S = torch.empty((qb.shape[0], cols), dtype=torch.float32, device=self.device)
        self._kernels().colbert_score(self, qb, pool, doc_begin, cols, S)
        return S


def _kept_rows(expert_repr, attention, corpus_ids):
    """(ids int64 [N], lengths int64 [N], rows [kept, d]) of a padded batch: the slots with attention > 0, in order."""
    if isinstance(expert_repr, dict):
        expert_repr = expert_repr["expert_repr"]
    x = expert_repr.detach()
    keep = attention.detach().to(x.device) > 0
    if x.dim() != 3 or keep.shape != x.shape[:2]:
        raise ValueError(f"expert_repr {tuple(x.shape)} and attention {tuple(keep.shape)} do not belong together")
    ids = torch.as_tensor(corpus_ids).reshape(-1).to(x.device, torch.int64)
    if ids.shape[0] != x.shape[0]:
        raise ValueError(f"{ids.shape[0]} corpus ids for {x.shape[0]} passages")
    return ids, keep.sum(1), x[keep]


class TokenIndexBuilder:
    """Collects the attended token rows of context batches (as the bf16 that is searched) and turns them into the on-disk index
    (`write`) or straight into a ColBERTIndex (`finish`), which equals load_index of the files `write` produces."""

    def __init__(self, corpus_len=None, device=None, kernels=None):
        self.corpus_len = None if corpus_len is None else int(corpus_len)
        self.device = None if device is None else torch.device(device)
        self.kn = kernels
        self.parts = []

    def add(self, contexts_repr, attention, corpus_ids):
        """One context batch: contexts_repr a repr dict or expert_repr [B, LD, d], attention [B, LD].  Returns the rows kept."""
        ids, lens, rows = _kept_rows(contexts_repr, attention, corpus_ids)
        self.parts.append((ids, lens, rows.to(_BF16)))
        return int(rows.shape[0])

    def _cat(self):
        if not self.parts:
            raise ValueError("no context batch was added")
        return tuple(torch.cat([p[i] for p in self.parts], 0) for i in range(3))

    def write(self, ctx_embeddings_dir, rank=0):
        """tokens_{rank:04}.pkl = (ids int64 [n], lengths int32 [n], reprs bfloat16 [sum(lengths), d]), pickle protocol 4."""
        ids, lens, rows = self._cat()
        os.makedirs(ctx_embeddings_dir, exist_ok=True)
        path = os.path.join(ctx_embeddings_dir, f"tokens_{rank:04}.pkl")
        with open(path, "wb") as f:
            pickle.dump((ids.cpu(), lens.to(torch.int32).cpu(), rows.cpu()), f, protocol=4)
        return path

    def finish(self, chunk=None):
        if self.corpus_len is None:
            raise ValueError("corpus_len is needed to build the index")
        ids, lens, rows = self._cat()
        return ColBERTIndex(ids, lens, rows, self.corpus_len, rows.device if self.device is None else self.device, chunk=chunk, kernels=self.kn)


def read_tokens(ctx_embeddings_dir):
    """Reads every tokens_*.pkl under the directory, in rank order: (ids int64 [n], lengths int64 [n], rows bf16 [sum(lengths), d])."""
    files = sorted(glob.glob(os.path.join(ctx_embeddings_dir, "tokens_*.pkl")))
    if not files:
        raise FileNotFoundError(f"no tokens_*.pkl under {ctx_embeddings_dir}")
    ids, lens, rows = [], [], []
    for path in files:
        with open(path, "rb") as f:
            i, n, r = pickle.load(f)
        i, n, r = torch.as_tensor(i).long().reshape(-1), torch.as_tensor(n).long().reshape(-1), torch.as_tensor(r)
        if r.dim() != 2 or i.shape != n.shape or int(n.sum()) != r.shape[0]:
            raise ValueError(f"{path}: ids {tuple(i.shape)}, lengths {tuple(n.shape)} and reprs {tuple(r.shape)} do not match")
        ids.append(i)
        lens.append(n)
        rows.append(r)
    if len({r.shape[1] for r in rows}) != 1:
        raise ValueError("token vectors of different widths")
    return torch.cat(ids), torch.cat(lens), torch.cat(rows, 0)


def load_index(ctx_embeddings_dir, corpus_len, device=None, chunk=None, kernels=None):
    """Reads every `tokens_{rank:04}.pkl` under `ctx_embeddings_dir` and merges all ranks' passages by doc id into ONE index on `device`."""
    device = torch.device(device) if device is not None else torch.device("cuda", 0)
    ids, lens, rows = read_tokens(ctx_embeddings_dir)
    return ColBERTIndex(ids, lens, rows, corpus_len, device, chunk=chunk, kernels=kernels)
