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

Product quantisation: `ColBERTIndex.quantize` / `load_index(..., quantizer="pq")` /
`TokenIndexBuilder.finish(quantizer="pq")` give a `ColBERTPQIndex` whose token rows are 8-bit codes over sub-vectors of 2, 4 or 8
features under one bf16 codebook (64, 32 or 16 bytes per token at d = 128 instead of 256); `blk_rows` uint8 [n_blk] holds the real
token rows of every block.  Its search returns, bit for bit, the dense search over the decoded rows (`ColBERTPQIndex.decode`).  The
two builders encode file by file / part by part: the dense index is never needed to make the quantised one.

Not supported (out of scope): residual token vectors, centroid pruning (PLAID-style candidate generation), an index across several
GPUs, a CPU index.
"""
import glob
import os
import pickle
import time

import torch

from . import ivf
from ._chunked import ChunkedIndex, _default_kernels

_BF16 = torch.bfloat16
_POOL = {"sum": 0, "max": 1}  # DPRHOT_POOL_SUM / DPRHOT_POOL_MAX
BLOCK = 16                    # token rows per block: one MFMA fragment, one passage
MAX_QUERY_LEN = 512           # DPRHOT_MAXSIM_MAX_LEN
PQ_MAX_DP = 128               # dprhot_colbert_pq_score keeps the codebook (dp * 512 bytes) in LDS and the query fragments in registers


def _bf16_padded(x, dp):
    """bf16 image of rows x [..., d], zero-padded to dp columns."""
    d = x.shape[-1]
    if d == dp:
        return x.to(_BF16).contiguous()
    out = torch.zeros(x.shape[:-1] + (dp,), dtype=_BF16, device=x.device)
    out[..., :d].copy_(x)
    return out


def _layout(doc_ids, lengths, corpus_len, device):
    """(ids, lens, doc_len int64 [corpus_len], doc_blk int64 [corpus_len + 1]) on `device` for passages listed by id with their token
    counts.  Ids that never appear get no block; an id given twice is a ValueError."""
    ids = torch.as_tensor(doc_ids).reshape(-1).to(device, torch.int64)
    lens = torch.as_tensor(lengths).reshape(-1).to(device, torch.int64)
    if ids.shape != lens.shape:
        raise ValueError(f"ids {tuple(ids.shape)} and lengths {tuple(lens.shape)} do not belong together")
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= corpus_len or int(lens.min()) < 0):
        raise ValueError("doc ids must lie in [0, corpus_len) and lengths must be non-negative")
    seen = torch.bincount(ids, minlength=corpus_len)
    if ids.numel() and int(seen.max()) > 1:
        raise ValueError(f"doc id {int(torch.nonzero(seen > 1)[0])} appears more than once")
    doc_len = torch.zeros(corpus_len, dtype=torch.int64, device=device)
    doc_len[ids] = lens
    doc_blk = torch.zeros(corpus_len + 1, dtype=torch.int64, device=device)
    torch.cumsum((doc_len + (BLOCK - 1)) // BLOCK, 0, out=doc_blk[1:])
    return ids, lens, doc_len, doc_blk


def _dest_rows(doc_blk, ids, lens):
    """int64 [sum(lens)]: the row of the block layout that every input row (grouped by passage, in the order of ids) goes to."""
    start = torch.cumsum(lens, 0) - lens              # first input row of every listed passage
    first = doc_blk[ids] * BLOCK - start              # + input row number = the row in the layout
    return torch.arange(int(lens.sum()), device=lens.device) + torch.repeat_interleave(first, lens)


def _blk_rows(doc_len, doc_blk):
    """uint8 [n_blk]: the real token rows of every block (16 but for a passage's last block)."""
    per_doc = doc_blk[1:] - doc_blk[:-1]
    doc = torch.repeat_interleave(torch.arange(doc_len.shape[0], device=doc_len.device), per_doc)
    within = torch.arange(int(doc_blk[-1]), device=doc_len.device) - doc_blk[doc]
    return (doc_len[doc] - within * BLOCK).clamp(max=BLOCK).to(torch.uint8)


def _real_rows(blk_rows):
    """bool [n_blk * 16]: True for the rows that hold a token."""
    return (torch.arange(BLOCK, device=blk_rows.device).unsqueeze(0) < blk_rows.unsqueeze(1)).reshape(-1)


class _TokenSearch(ChunkedIndex):
    """What the dense and the product-quantised token index share: query packing, `search` and `score` over the kernels named by
    _SEARCH / _SCORE.  A subclass sets device, doc_blk, corpus_len, d, dp and calls `_init_search`."""

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
                         lambda *tail: getattr(kn, self._SEARCH)(self, qb, pool, *tail))
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
        getattr(self._kernels(), self._SCORE)(self, qb, pool, doc_begin, cols, S)
        return S


class ColBERTIndex(_TokenSearch):
    """Device-resident token index of a ColBERT corpus; `search` is the exhaustive MaxSim top-k."""

    _SEARCH, _SCORE = "colbert_search", "colbert_score"

    def __init__(self, doc_ids, lengths, rows, corpus_len, device, chunk=None, kernels=None):
        """From unpadded token rows grouped by passage: doc_ids int64 [n], lengths [n] (tokens of each passage), rows [sum(lengths), d]
        in the order of doc_ids.  Ids that never appear get zero blocks; an id given twice is a ValueError."""
        corpus_len = int(corpus_len)
        if not 0 < corpus_len < 2 ** 31:
            raise ValueError(f"corpus_len={corpus_len} out of range (1 .. 2^31 - 1)")
        device = torch.device(device)
        rows = torch.as_tensor(rows).to(device)
        if rows.dim() != 2:
            raise ValueError(f"rows {tuple(rows.shape)}; [sum(lengths), d] expected")
        ids, lens, doc_len, doc_blk = _layout(doc_ids, lengths, corpus_len, device)
        if int(lens.sum()) != rows.shape[0]:
            raise ValueError(f"{rows.shape[0]} token rows for lengths that sum to {int(lens.sum())}")
        d = int(rows.shape[1])
        dp = (max(d, 1) + 31) // 32 * 32
        n_blk = int(doc_blk[-1])
        tok = torch.zeros((n_blk * BLOCK, dp), dtype=_BF16, device=device)
        if rows.shape[0]:
            tok[_dest_rows(doc_blk, ids, lens), :d] = rows.to(_BF16)
        self._set(tok, doc_blk, corpus_len, d, chunk, kernels, _blk_rows(doc_len, doc_blk))

    @classmethod
    def from_packed(cls, tok, doc_blk, corpus_len, d, chunk=None, kernels=None, blk_rows=None):
        """From tensors already in the device layout (csrc/colbert.h), on their device: tok bf16 [n_blk * 16, dp], doc_blk int64
        [corpus_len + 1].  blk_rows uint8 [n_blk] (the real token rows of every block; only `quantize` reads it) defaults to the rows
        up to a block's last non-zero one."""
        self = cls.__new__(cls)
        self._set(tok, doc_blk, int(corpus_len), int(d), chunk, kernels, blk_rows)
        return self

    @classmethod
    def from_repr(cls, expert_repr, attention, corpus_ids, corpus_len, device=None, chunk=None, kernels=None):
        """From a padded batch: expert_repr [N, LD, d], attention [N, LD]; the slots with attention > 0 are kept, in order."""
        device = expert_repr.device if device is None else device
        ids, lens, rows = _kept_rows(expert_repr, attention, corpus_ids)
        return cls(ids, lens, rows, corpus_len, device, chunk=chunk, kernels=kernels)

    def _set(self, tok, doc_blk, corpus_len, d, chunk, kernels, blk_rows=None):
        assert tok.dtype == _BF16 and doc_blk.dtype == torch.int64 and tok.dim() == 2 and tok.shape[1] % 32 == 0 and tok.shape[0] % BLOCK == 0
        assert doc_blk.shape[0] == corpus_len + 1 and tok.is_contiguous() and doc_blk.is_contiguous()
        self.device = doc_blk.device
        self.tok, self.doc_blk = tok, doc_blk
        self.corpus_len, self.d, self.dp = corpus_len, d, int(tok.shape[1])
        self.n_blk = int(tok.shape[0]) // BLOCK
        assert blk_rows is None or (blk_rows.dtype == torch.uint8 and blk_rows.shape == (self.n_blk,))
        self._blk_rows = blk_rows
        self._init_search(chunk, kernels)

    @property
    def nbytes(self):
        """Bytes of device memory the index holds (token rows and block offsets)."""
        return sum(t.numel() * t.element_size() for t in (self.tok, self.doc_blk))

    @property
    def blk_rows(self):
        """uint8 [n_blk]: the real token rows of every block."""
        if self._blk_rows is None:
            used = (self.tok.view(self.n_blk, BLOCK, self.dp) != 0).any(2)
            last = (used * torch.arange(1, BLOCK + 1, device=self.device)).amax(1) if self.n_blk else used.sum(1)
            self._blk_rows = last.to(torch.uint8)
        return self._blk_rows

    def quantize(self, dsub=8, codebook=None, **train_kwargs):
        """The ColBERTPQIndex of this index: token rows replaced by 8-bit codes over sub-vectors of `dsub` features (DESIGN.md section
        12.1).  Trains a codebook on the index's own token rows (train_pq(**train_kwargs)) unless one is given; the result shares
        doc_blk with this index and keeps no reference to the dense rows.  The code bytes of a padding row are 0."""
        kn = self._kernels()
        blk_rows = self.blk_rows
        real = torch.nonzero(_real_rows(blk_rows)).reshape(-1)
        if codebook is None:
            pick = _sample(int(real.shape[0]), train_kwargs.get("train_size", 65536), train_kwargs.get("seed", 0))
            codebook = train_pq(self.tok[real if pick is None else real[pick.to(self.device)]], dsub=dsub, kernels=kn, **train_kwargs)
        elif train_kwargs:
            raise TypeError(f"a codebook was given: nothing to train with {sorted(train_kwargs)}")
        codebook = ivf._check_codebook(codebook, self.dp, dsub, PQ_MAX_DP).to(self.device).contiguous()
        codes = torch.zeros((self.n_blk * BLOCK, self.dp // int(dsub)), dtype=torch.uint8, device=self.device)
        for lo in range(0, int(real.shape[0]), 1 << 22):
            part = real[lo:lo + (1 << 22)]
            codes[part] = kn.colbert_pq_encode(self.tok[part], codebook)
        return ColBERTPQIndex.from_packed(codes, blk_rows, codebook, self.doc_blk, self.corpus_len, self.d, chunk=self.chunk, kernels=kn)


# ---- product-quantised token rows ---------------------------------------------------------------------------

def _sample(n, train_size, seed):
    """Sorted int64 positions of a seeded sample of `train_size` out of n rows (ivf.train_pq's own choice), None: all of them."""
    if n <= int(train_size):
        return None
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[: int(train_size)].sort().values


def train_pq(rows, dsub=8, iters=10, train_size=65536, seed=0, kernels=None, on_iteration=None):
    """Codebook bf16 [dp / dsub, 256, dsub] for token rows [n, d] (any float dtype; searched as bf16, zero-padded to dp = a multiple of
    32, at most 128) on a HIP device: ivf.train_pq -- its sample, initialisation and Lloyd iterations -- with the assignment by
    dprhot_colbert_pq_encode."""
    kn = _default_kernels(kernels)
    rows = torch.as_tensor(rows)
    if rows.dim() != 2:
        raise ValueError(f"rows {tuple(rows.shape)}; [n, d] expected")
    dp = (max(int(rows.shape[1]), 1) + 31) // 32 * 32
    return ivf.train_pq(_bf16_padded(rows, dp), dsub=dsub, iters=iters, train_size=train_size, seed=seed, kernels=kn,
                        on_iteration=on_iteration, max_dp=PQ_MAX_DP, encode=kn.colbert_pq_encode)


class ColBERTPQIndex(_TokenSearch):
    """Token index with product-quantised rows: tok_code uint8 [n_blk * 16, m], blk_rows uint8 [n_blk] and ONE codebook bf16
    [m, 256, dsub] instead of tok.  `search` / `score` return, bit for bit, what `decode()` -- the ColBERTIndex over the decoded rows,
    the rows at or behind blk_rows zero -- returns."""

    _SEARCH, _SCORE = "colbert_pq_search", "colbert_pq_score"
    FORMAT = "dpr_scale_amd.colbert_pq/1"

    def __init__(self, *args, **kwargs):
        raise TypeError("a ColBERTPQIndex comes from ColBERTIndex.quantize, ColBERTPQIndex.from_packed, load_pq_index or a quantizer='pq' build")

    @classmethod
    def from_packed(cls, tok_code, blk_rows, codebook, doc_blk, corpus_len, d, chunk=None, kernels=None):
        """From tensors in the device layout (csrc/colbert_pq.h), on their device."""
        self = cls.__new__(cls)
        m, _, dsub = codebook.shape
        ivf._check_codebook(codebook, m * dsub, dsub, PQ_MAX_DP)
        corpus_len = int(corpus_len)
        assert tok_code.dtype == torch.uint8 and blk_rows.dtype == torch.uint8 and doc_blk.dtype == torch.int64
        assert tok_code.dim() == 2 and tok_code.shape[1] == m and tok_code.shape[0] == blk_rows.shape[0] * BLOCK
        assert doc_blk.shape[0] == corpus_len + 1 and all(t.is_contiguous() for t in (tok_code, blk_rows, codebook, doc_blk))
        self.device = doc_blk.device
        self.tok_code, self.blk_rows, self.codebook, self.doc_blk = tok_code, blk_rows, codebook, doc_blk
        self.corpus_len, self.d, self.dp, self.dsub = corpus_len, int(d), int(m * dsub), int(dsub)
        self.n_blk = int(blk_rows.shape[0])
        self._init_search(chunk, kernels)
        return self

    def _tensors(self):
        return dict(tok_code=self.tok_code, blk_rows=self.blk_rows, codebook=self.codebook, doc_blk=self.doc_blk)

    @property
    def nbytes(self):
        """Bytes of device memory the index holds (codes, row counts, codebook and block offsets)."""
        return sum(t.numel() * t.element_size() for t in self._tensors().values())

    def decode(self):
        """The ColBERTIndex this one searches, by definition: tok = pq_decode(tok_code, codebook), the rows at or behind blk_rows zero."""
        tok = ivf.pq_decode(self.tok_code, self.codebook)
        tok[~_real_rows(self.blk_rows)] = 0
        return ColBERTIndex.from_packed(tok.contiguous(), self.doc_blk, self.corpus_len, self.d, chunk=self.chunk, kernels=self.kn,
                                        blk_rows=self.blk_rows.clamp(max=BLOCK))

    def quantize(self, *args, **kwargs):
        raise TypeError("the index is quantised already")

    def save(self, path):
        """One torch.save of the tensors (on the CPU) and sizes; load_pq_index reads it back."""
        blob = {k: t.cpu() for k, t in self._tensors().items()}
        blob.update(format=self.FORMAT, corpus_len=self.corpus_len, d=self.d, dsub=self.dsub)
        torch.save(blob, path)
        return path


def load_pq_index(path, device=None, chunk=None, kernels=None):
    """The ColBERTPQIndex that ColBERTPQIndex.save wrote, placed on `device`."""
    device = torch.device(device) if device is not None else torch.device("cuda", 0)
    blob = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(blob, dict) or blob.get("format") != ColBERTPQIndex.FORMAT:
        raise ValueError(f"{path}: not a product-quantised ColBERT index file")
    mv = lambda t: t.contiguous().to(device)
    return ColBERTPQIndex.from_packed(mv(blob["tok_code"]), mv(blob["blk_rows"]), mv(blob["codebook"]), mv(blob["doc_blk"]),
                                      blob["corpus_len"], blob["d"], chunk=chunk, kernels=kernels)


def _plain(quantizer, codebook, train_kwargs):
    """True for quantizer=None (with nothing to quantise with), False for "pq"."""
    if quantizer in (None, "None"):
        if codebook is not None or train_kwargs:
            raise TypeError(f"quantizer=None takes no codebook and no training arguments {sorted(train_kwargs)}")
        return True
    if quantizer != "pq":
        raise NotImplementedError(f"quantizer={quantizer!r}: None or 'pq'")
    return False


def _build_pq(parts, corpus_len, device, dsub, codebook, train_kwargs, chunk, kernels):
    """The ColBERTPQIndex of the passages that parts() yields as (ids, lengths, rows) pieces -- ColBERTIndex(all of them).quantize(
    codebook=the codebook) in codes, blk_rows and doc_blk -- with never more than ONE piece's dense rows on the device.  parts() is
    walked twice: layout and a seeded sample of token rows (the train_size smallest of one uniform key per row, kept on the host), then
    the codes piece by piece."""
    corpus_len, dsub, device = int(corpus_len), int(dsub), torch.device(device)
    if not 0 < corpus_len < 2 ** 31:
        raise ValueError(f"corpus_len={corpus_len} out of range (1 .. 2^31 - 1)")
    kn = _default_kernels(kernels)
    if codebook is not None and train_kwargs:
        raise TypeError(f"a codebook was given: nothing to train with {sorted(train_kwargs)}")
    train_size, seed = int(train_kwargs.get("train_size", 65536)), int(train_kwargs.get("seed", 0))
    gen = torch.Generator().manual_seed(seed)
    ids, lens, keys, sample, d = [], [], [], [], None
    for i, n, r in parts():
        i, n, r = torch.as_tensor(i).reshape(-1).long().cpu(), torch.as_tensor(n).reshape(-1).long().cpu(), torch.as_tensor(r)
        if r.dim() != 2 or i.shape != n.shape or int(n.sum()) != r.shape[0] or (d is not None and r.shape[1] != d):
            raise ValueError(f"ids {tuple(i.shape)}, lengths {tuple(n.shape)} and rows {tuple(r.shape)} do not belong together")
        d = int(r.shape[1])
        ids.append(i)
        lens.append(n)
        if codebook is None and r.shape[0]:
            key = torch.rand(r.shape[0], generator=gen, dtype=torch.float64)
            keep = torch.sort(key, stable=True).indices[:train_size].sort().values
            keys.append(key[keep])
            sample.append(r[keep.to(r.device)].to(_BF16).cpu())
    if d is None:
        raise ValueError("no token rows to build an index from")
    dp = (max(d, 1) + 31) // 32 * 32
    if codebook is None:
        ivf._check_pq_shape(dp, dsub, PQ_MAX_DP)
        rows = torch.cat(sample, 0) if sample else torch.zeros((0, d), dtype=_BF16)
        if rows.shape[0] > train_size:
            rows = rows[torch.sort(torch.cat(keys), stable=True).indices[:train_size].sort().values]
        codebook = train_pq(rows.to(device), dsub=dsub, kernels=kn, **dict(train_kwargs, train_size=max(train_size, rows.shape[0])))
    codebook = ivf._check_codebook(codebook, dp, dsub, PQ_MAX_DP).to(device).contiguous()
    _, _, doc_len, doc_blk = _layout(torch.cat(ids), torch.cat(lens), corpus_len, device)
    blk_rows = _blk_rows(doc_len, doc_blk)
    codes = torch.zeros((int(doc_blk[-1]) * BLOCK, dp // dsub), dtype=torch.uint8, device=device)
    for i, n, r in parts():
        r = torch.as_tensor(r)
        if r.shape[0]:
            dest = _dest_rows(doc_blk, torch.as_tensor(i).reshape(-1).to(device, torch.int64), torch.as_tensor(n).reshape(-1).to(device, torch.int64))
            codes[dest] = kn.colbert_pq_encode(_bf16_padded(r.to(device), dp), codebook)
    return ColBERTPQIndex.from_packed(codes, blk_rows, codebook, doc_blk, corpus_len, d, chunk=chunk, kernels=kn)


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

    def finish(self, chunk=None, quantizer=None, sub_vec_dim=8, codebook=None, **train_kwargs):
        """The index of the batches added so far.  quantizer="pq": a ColBERTPQIndex (sub_vec_dim in {2, 4, 8}; a codebook, or
        train_pq(**train_kwargs) on a seeded sample), encoded batch by batch -- the batches are never concatenated."""
        if self.corpus_len is None:
            raise ValueError("corpus_len is needed to build the index")
        if not _plain(quantizer, codebook, train_kwargs):
            if not self.parts:
                raise ValueError("no context batch was added")
            device = self.parts[0][2].device if self.device is None else self.device
            return _build_pq(lambda: iter(self.parts), self.corpus_len, device, sub_vec_dim, codebook, train_kwargs, chunk, self.kn)
        ids, lens, rows = self._cat()
        return ColBERTIndex(ids, lens, rows, self.corpus_len, rows.device if self.device is None else self.device, chunk=chunk, kernels=self.kn)


def _token_files(ctx_embeddings_dir):
    files = sorted(glob.glob(os.path.join(ctx_embeddings_dir, "tokens_*.pkl")))
    if not files:
        raise FileNotFoundError(f"no tokens_*.pkl under {ctx_embeddings_dir}")
    return files


def _read_token_file(path):
    with open(path, "rb") as f:
        i, n, r = pickle.load(f)
    i, n, r = torch.as_tensor(i).long().reshape(-1), torch.as_tensor(n).long().reshape(-1), torch.as_tensor(r)
    if r.dim() != 2 or i.shape != n.shape or int(n.sum()) != r.shape[0]:
        raise ValueError(f"{path}: ids {tuple(i.shape)}, lengths {tuple(n.shape)} and reprs {tuple(r.shape)} do not match")
    return i, n, r


def read_tokens(ctx_embeddings_dir):
    """Reads every tokens_*.pkl under the directory, in rank order: (ids int64 [n], lengths int64 [n], rows bf16 [sum(lengths), d])."""
    ids, lens, rows = zip(*(_read_token_file(path) for path in _token_files(ctx_embeddings_dir)))
    if len({r.shape[1] for r in rows}) != 1:
        raise ValueError("token vectors of different widths")
    return torch.cat(ids), torch.cat(lens), torch.cat(rows, 0)


def load_index(ctx_embeddings_dir, corpus_len, device=None, chunk=None, kernels=None, quantizer=None, sub_vec_dim=8, codebook=None,
               **train_kwargs):
    """Reads every `tokens_{rank:04}.pkl` under `ctx_embeddings_dir` and merges all ranks' passages by doc id into ONE index on `device`.

    quantizer="pq" (sub_vec_dim in {2, 4, 8}): a ColBERTPQIndex under `codebook`, or under train_pq(**train_kwargs) of a seeded sample
    of token rows taken across the files; the files are read one at a time (twice) and encoded one at a time, so the device never holds
    more than one file's dense rows."""
    device = torch.device(device) if device is not None else torch.device("cuda", 0)
    if not _plain(quantizer, codebook, train_kwargs):
        files = _token_files(ctx_embeddings_dir)
        return _build_pq(lambda: (_read_token_file(path) for path in files), corpus_len, device, sub_vec_dim, codebook, train_kwargs, chunk,
                         kernels)
    ids, lens, rows = read_tokens(ctx_embeddings_dir)
    return ColBERTIndex(ids, lens, rows, corpus_len, device, chunk=chunk, kernels=kernels)
