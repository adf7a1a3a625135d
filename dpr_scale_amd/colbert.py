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

Centroid pruning: `ColBERTIndex.build_centroids` assigns every stored token to its nearest of C unit-norm
centroids and keeps, per centroid, the sorted list of passages with a token there.  `search_pruned(q, topk, nprobe)` probes the
`nprobe` best centroids of every query token, unites their lists into one sorted candidate list per query and scores ONLY those
passages -- with the exhaustive score, bit for bit (dprhot_colbert_cand_search) -- so its result is the exhaustive top-k restricted to
the candidate set; what it may lose is a passage none of whose tokens lies in a probed centroid.  Assignment and probing are exact bf16
top-k searches on the MFMA path (hotpath.CorpusSearch), ties to the lower centroid id.

Candidate lists: the union is built by kernels (dprhot_colbert_union_count / _fill: a bitmap of the corpus per
query, marked with atomic ORs and read out in order -- no sort) whenever the index's kernel set defines `colbert_union_count`, as
hotpath.HipKernels does; queries go through in batches whose bitmaps stay under UNION_WS_BYTES.  A kernel set without that method takes
`_union_torch`, the same lists from torch.unique: it is the definition the kernels are held to.

Centroid interaction: `search_pruned(..., ndocs=n)` first scores every candidate approximately, each passage
token replaced by its centroid --

    approx(n, doc) = POOL over query tokens i < LQ of  max(0, max over c in doc's centroid list of <q[n, i], centroid_c>)

from a per-query table of query-token x centroid products (`centroid_table`) and the passages' sorted centroid lists (`doc_centroids`,
built from `tok_centroid` on first use), keeps the best `ndocs` per query (dprhot_colbert_cen_search) and runs the exact score on those
only: the result is the exhaustive top-k restricted to the survivors, bit for bit.  `approx` is, bit for bit, the exhaustive score of
the index whose token rows are `centroids[tok_centroid]`.  No token row is read by the approximate stage.

Residual compression: `ColBERTIndex.compress(nbits)` / `load_index(..., quantizer="residual")` /
`TokenIndexBuilder.finish(quantizer="residual")` give a `ColBERTResidualIndex`, the ColBERTv2 format: per token its centroid id (the
`tok_centroid` the pruned search already holds) plus 1, 2 or 4 bits per feature of row - centroid under one bucket set (20, 36 or 68
bytes per token at d = 128 instead of 256).  It is searched with centroid pruning only: probing, the inverted lists and the centroid
interaction are shared with the dense index (the `_CentroidPruning` mixin) and the exact stage decodes the surviving candidates at the
MFMA's operand read (dprhot_colbert_res_search).  Every result is, bit for bit, that of `ColBERTResidualIndex.decode()`.

Not supported (out of scope): a residual index searched exhaustively, a candidate kernel over the product-quantised rows, per-dimension
buckets, PLAID's centroid-score threshold, an index across several GPUs, a CPU index.
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
CEN_TABLE_BYTES = 1 << 28     # centroid interaction: queries go through in batches whose table fp32 [b, C, LT] stays under this (b >= 1)
UNION_WS_BYTES = 1 << 28      # candidate lists: queries go through in batches whose membership bitmaps stay under this (b >= 1)
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


class _CentroidPruning:
    """The pruned search that the dense and the residual token index share (DESIGN.md sections 12.2 to 12.4): centroids, probing, the
    union of inverted lists, the centroid-interaction stage and `search_pruned`.  A class mixes it into a _TokenSearch that sets device,
    doc_blk, corpus_len, d, dp and n_blk, calls `_set_centroids`, and supplies the exact stage as two hooks:
      _score_lists(kn, qb, pool, cand_off, cand_doc, pos_begin, cols, S)                       a window of candidate positions into S
      _search_lists(kn, qb, pool, cand_off, cand_doc, max_count, values, indices, chunk)      the top-k of every list, as doc ids"""

    centroids = tok_centroid = cen_off = cen_doc = _doc_cen = None

    def _set_centroids(self, centroids, tok_centroid, cen_off, cen_doc):
        C = int(centroids.shape[0])
        assert centroids.dtype == _BF16 and centroids.shape == (C, self.dp) and C >= 1
        assert tok_centroid.dtype == torch.int32 and tok_centroid.shape == (self.n_blk * BLOCK,)
        assert cen_off.dtype == torch.int64 and cen_off.shape == (C + 1,) and cen_doc.dtype == torch.int32 and cen_doc.dim() == 1
        self.centroids, self.tok_centroid, self.cen_off, self.cen_doc = centroids, tok_centroid, cen_off, cen_doc
        self._doc_cen = None

    def _need_centroids(self):
        if self.centroids is None:
            raise ValueError("the index has no centroids: build_centroids or load_centroids first")
        return int(self.centroids.shape[0])

    def save_centroids(self, path):
        """A protocol-4 pickle of (centroids, tok_centroid, cen_off, cen_doc) on the CPU; load_centroids reads it back."""
        self._need_centroids()
        with open(path, "wb") as f:
            pickle.dump(tuple(t.cpu() for t in (self.centroids, self.tok_centroid, self.cen_off, self.cen_doc)), f, protocol=4)
        return path

    def load_centroids(self, path):
        """The centroids save_centroids wrote for an index of the same layout: it then probes and searches bit-identically."""
        with open(path, "rb") as f:
            blob = pickle.load(f)
        if not isinstance(blob, tuple) or len(blob) != 4:
            raise ValueError(f"{path}: not a centroid file")
        cen, tc, off, doc = (torch.as_tensor(t).contiguous().to(self.device) for t in blob)
        if cen.dim() != 2 or cen.shape[1] != self.dp or tc.shape != (self.n_blk * BLOCK,) or off.shape != (cen.shape[0] + 1,):
            raise ValueError(f"{path}: centroids {tuple(cen.shape)} over {tuple(tc.shape)} token rows do not belong to this index "
                             f"(dp={self.dp}, {self.n_blk * BLOCK} rows)")
        self._set_centroids(cen, tc, off, doc)
        return self

    def _probe(self, qb, nprobe):
        C, nprobe = self._need_centroids(), int(nprobe)
        if not 1 <= nprobe <= C:
            raise ValueError(f"nprobe={nprobe} out of range (1 .. n_centroids={C})")
        nq, LQ, dp = qb.shape
        return _nearest(self._kernels(), qb.reshape(nq * LQ, dp), self.centroids, nprobe).view(nq, LQ, nprobe)

    def probe(self, q, nprobe):
        """int64 [nq, LQ, nprobe]: the exact top-`nprobe` centroids of every query token by inner product (bf16 MFMA path), best first,
        ties to the lower centroid id.  An all-zero (padding) query token gets ids too; `candidates` drops it."""
        return self._probe(self._queries(q), nprobe)

    def _candidates(self, qb, nprobe):
        return self._union(qb, self._probe(qb, nprobe))

    def _union(self, qb, cids):
        """(cand_off, cand_doc, n_cand, max_count) of `candidates` from the probed centroid ids [nq, LQ, nprobe].  Runs the kernels of
        DESIGN.md section 12.5 (dprhot_colbert_union_count / _fill) when the index's kernel set defines `colbert_union_count` --
        hotpath.HipKernels does -- and `_union_torch`, the definition, otherwise.  The kernel route takes the queries in batches whose
        workspace stays under UNION_WS_BYTES; each batch makes ONE host read (its two counts, which size cand_doc)."""
        kn = self._kernels()
        if not hasattr(kn, "colbert_union_count"):  # the one capability check: kernel sets written before section 12.5 keep the torch route
            return self._union_torch(qb, cids)
        self._need_centroids()
        nq, dev = int(qb.shape[0]), self.device
        cids = cids.to(torch.int64).contiguous()
        cand_off = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        parts, n_cand, max_count = [], 0, 0
        for lo, hi in self._union_batches(nq):
            ws = kn.colbert_union_workspace(hi - lo, self.corpus_len, self.cen_off)
            off, totals = cand_off[lo:hi + 1], torch.empty(2, dtype=torch.int64, device=dev)
            if lo:  # a later batch counts into a buffer of its own: its offsets start at 0 and are shifted behind the fill
                off = torch.empty(hi - lo + 1, dtype=torch.int64, device=dev)
            kn.colbert_union_count(self, cids[lo:hi], qb[lo:hi], off, totals, ws)
            n, longest = totals.tolist()
            docs = torch.empty(n, dtype=torch.int32, device=dev)
            kn.colbert_union_fill(self, off, docs, ws)
            if lo:
                cand_off[lo + 1:hi + 1] = off[1:] + n_cand
            parts.append(docs)
            n_cand, max_count = n_cand + n, max(max_count, longest)
        return cand_off, parts[0] if len(parts) == 1 else torch.cat(parts), n_cand, max_count

    def _union_batches(self, nq):
        """(lo, hi) query ranges whose union workspace (a bitmap of corpus_len bits per query) stays under UNION_WS_BYTES, at least one
        query each; no range has more than the 65535 queries of one launch."""
        from . import _lib

        per_query = _lib.colbert_union_workspace_bytes(1, self.corpus_len)  # host code; n queries need at most n times this
        step = min(65535, max(1, UNION_WS_BYTES // per_query))
        return [(lo, min(lo + step, nq)) for lo in range(0, nq, step)]

    def _union_torch(self, qb, cids):
        """(cand_off, cand_doc, n_cand, max_count) of `candidates` from the probed centroid ids [nq, LQ, nprobe]; ONE host read of its
        own (the two counts) -- torch.unique and repeat_interleave size their outputs on the host themselves."""
        C, dev = self._need_centroids(), self.device
        nq = int(qb.shape[0])
        live = (qb != 0).any(2).unsqueeze(2) & (cids >= 0)                           # padded query tokens probe nothing (-1: a NaN token)
        qid = torch.arange(nq, device=dev).view(nq, 1, 1).expand_as(cids)[live]
        pair = torch.unique(qid * C + cids[live])                                    # a query names a centroid once
        qid, cid = pair // C, pair % C
        lens = self.cen_off[cid + 1] - self.cen_off[cid]
        seg = torch.repeat_interleave(torch.arange(pair.shape[0], device=dev), lens)
        within = torch.arange(seg.shape[0], device=dev) - (torch.cumsum(lens, 0) - lens)[seg]
        docs = self.cen_doc[self.cen_off[cid][seg] + within].to(torch.int64)
        key = torch.unique(qid[seg] * self.corpus_len + docs)                        # sorted: by query, then by doc id
        counts = torch.bincount(key // self.corpus_len, minlength=nq)
        cand_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=cand_off[1:])
        n_cand, max_count = torch.stack([cand_off[-1], counts.max()]).tolist()
        return cand_off, (key % self.corpus_len).to(torch.int32), int(n_cand), int(max_count)

    def candidates(self, q, nprobe):
        """(cand_off int64 [nq + 1], cand_doc int32 [n_cand]): per query the sorted, duplicate-free union of the inverted lists of the
        centroids its (non-padding) tokens probe, built on the device."""
        return self._candidates(self._queries(q), nprobe)[:2]

    def score_candidates(self, q, cand_off, cand_doc, query_pool="sum"):
        """fp32 [nq, max_count]: cell [n, p] is the exhaustive score of query n and its p-th candidate, bit for bit; a cell at or behind
        the query's count (or whose doc id lies outside the corpus) is NaN, "no candidate"."""
        pool, qb = self._pool(query_pool), self._queries(q)
        cand_off, cand_doc, max_count = self._lists(qb, cand_off, cand_doc)
        S = torch.empty((qb.shape[0], max_count), dtype=torch.float32, device=self.device)
        if max_count:
            self._score_lists(self._kernels(), qb, pool, cand_off, cand_doc, 0, max_count, S)
        return S

    # ---- centroid interaction ----
    def doc_centroids(self):
        """(doc_cen_off int64 [corpus_len + 1], doc_cen int32): per passage the sorted, duplicate-free centroid ids of its stored tokens
        -- the transpose of cen_off / cen_doc -- built on first use from tok_centroid (one torch.unique of doc * C + centroid) and kept;
        a passage without tokens has an empty list."""
        C = self._need_centroids()
        if self._doc_cen is None:
            # ids >= C belong to no list (as the kernels skip them): unmasked, doc * C + id would land in another passage's list.  No
            # index that build_centroids made holds one; from_packed and a loaded centroid file may.
            tc = self.tok_centroid
            self._doc_cen = _doc_centroid_lists(torch.where(tc < C, tc, torch.full_like(tc, -1)), self.doc_blk, C, self.corpus_len)
        return self._doc_cen

    def _centroid_table(self, qb):
        nq, LQ, _ = qb.shape
        T = torch.empty((nq, self._need_centroids(), (LQ + BLOCK - 1) // BLOCK * BLOCK), dtype=torch.float32, device=self.device)
        self._kernels().colbert_cen_table(self, qb, T)
        return T

    def centroid_table(self, q):
        """T fp32 [nq, C, LT], LT = 16 * ceil(LQ / 16): T[n, c, i] = <q[n, i], centroid_c> as the exhaustive kernel computes a token's
        product; the columns behind LQ are 0."""
        return self._centroid_table(self._queries(q))

    def _cen_batches(self, qb):
        """(lo, hi) query ranges whose centroid table stays under CEN_TABLE_BYTES, at least one query each."""
        nq, LQ, _ = qb.shape
        per_query = self._need_centroids() * ((LQ + BLOCK - 1) // BLOCK * BLOCK) * 4
        step = max(1, CEN_TABLE_BYTES // per_query)
        return [(lo, min(lo + step, nq)) for lo in range(0, nq, step)]

    def _lists(self, qb, cand_off, cand_doc):
        cand_off = cand_off.to(self.device, torch.int64).contiguous()
        cand_doc = cand_doc.to(self.device, torch.int32).contiguous()
        if cand_off.shape != (qb.shape[0] + 1,):
            raise ValueError(f"cand_off {tuple(cand_off.shape)} for {qb.shape[0]} queries")
        off = cand_off.clamp(0, int(cand_doc.shape[0]))  # the kernel's own reading of a pair of offsets
        return cand_off, cand_doc, int((off[1:] - off[:-1]).max().clamp(min=0))

    def approx_candidates(self, q, cand_off, cand_doc, query_pool="sum"):
        """fp32 [nq, max_count]: cell [n, p] is approx(n, the query's p-th candidate); a cell at or behind the query's count (or whose
        doc id lies outside the corpus) is NaN, "no candidate".  The mirror of score_candidates."""
        pool, qb = self._pool(query_pool), self._queries(q)
        cand_off, cand_doc, max_count = self._lists(qb, cand_off, cand_doc)
        S = torch.empty((qb.shape[0], max_count), dtype=torch.float32, device=self.device)
        if max_count:
            kn = self._kernels()
            for lo, hi in self._cen_batches(qb):
                kn.colbert_cen_score(self, self._centroid_table(qb[lo:hi]), qb.shape[1], pool, cand_off[lo:hi + 1].contiguous(), cand_doc, 0,
                                     max_count, S[lo:hi])
        return S

    def prune_candidates(self, q, cand_off, cand_doc, ndocs, query_pool="sum"):
        """int32 [nq, ndocs]: per query its best `ndocs` candidates by approx (ties to the lower position of its list: the lower doc id
        of a sorted list), the row sorted ascending with its -1 entries (fewer than ndocs candidates) first."""
        pool, qb = self._pool(query_pool), self._queries(q)
        cand_off, cand_doc, max_count = self._lists(qb, cand_off, cand_doc)
        return self._prune(qb, pool, cand_off, cand_doc, max_count, int(ndocs))

    def _prune(self, qb, pool, cand_off, cand_doc, max_count, ndocs, chunk=None):
        if ndocs < 1:
            raise ValueError(f"ndocs={ndocs} out of range (>= 1)")
        nq, LQ, kn = int(qb.shape[0]), int(qb.shape[1]), self._kernels()
        keep = torch.full((nq, ndocs), -1, dtype=torch.int64, device=self.device)
        k = min(ndocs, self.corpus_len)
        if max_count:
            for lo, hi in self._cen_batches(qb):
                T = self._centroid_table(qb[lo:hi])
                c = self.default_chunk(hi - lo) if chunk is None else int(chunk)
                c = max(8, min(c, (max_count + 7) // 8 * 8))
                values = torch.empty((hi - lo, k), dtype=torch.float32, device=self.device)
                indices = torch.empty((hi - lo, k), dtype=torch.int64, device=self.device)
                ws = kn.colbert_cen_workspace(hi - lo, c, k, self.doc_blk)
                kn.colbert_cen_search(self, T, LQ, pool, cand_off[lo:hi + 1].contiguous(), cand_doc, max_count, values, indices, c, ws)
                keep[lo:hi, :k] = indices
        return torch.sort(keep.to(torch.int32), dim=1).values

    def search_pruned(self, q, topk, nprobe, query_pool="sum", chunk=None, ndocs=None):
        """`search` over the candidates of `candidates(q, nprobe)` only: (scores fp32 [nq, topk], ids int64 [nq, topk]), score
        descending with ties to the lower doc id -- the exhaustive top-k restricted to the candidate set, bit for bit.  A query with
        fewer than topk candidates ends in -inf / -1.  latency: encode_time, candidate_time (probe and union), search_time.

        ndocs (>= topk; None: every candidate is scored exactly): the centroid-interaction stage keeps every query's best `ndocs`
        candidates by approximate score (prune_candidates) and the exact score runs on those only -- the exhaustive top-k restricted
        to the survivors, bit for bit.  The stage is skipped when no query has more than `ndocs` candidates.  latency gains
        interaction_time."""
        pool, topk = self._pool(query_pool), int(topk)
        if not 1 <= topk <= self.corpus_len:
            raise ValueError(f"topk={topk} out of range (1 .. corpus_len={self.corpus_len})")
        if ndocs is not None:
            ndocs = int(ndocs)
            if topk > ndocs:
                raise ValueError(f"topk={topk} above ndocs={ndocs}: the exact stage scores ndocs candidates per query")
        tic = time.perf_counter()
        qb = self._queries(q)
        self.latency["encode_time"] += time.perf_counter() - tic
        tic = time.perf_counter()
        cand_off, cand_doc, _, max_count = self._candidates(qb, nprobe)
        self.latency["candidate_time"] += time.perf_counter() - tic
        if ndocs is not None and ndocs < max_count:
            tic = time.perf_counter()
            # the survivors, sorted, ARE the exact stage's lists: -1 entries score NaN there, so nothing is compacted or read back
            cand_doc = self._prune(qb, pool, cand_off, cand_doc, max_count, ndocs, chunk).reshape(-1)
            cand_off = torch.arange(qb.shape[0] + 1, dtype=torch.int64, device=self.device) * ndocs
            max_count = ndocs
            self.latency["interaction_time"] += time.perf_counter() - tic
        tic = time.perf_counter()
        out = self._search_candidates(qb, pool, topk, cand_off, cand_doc, max_count, chunk)
        self.latency["search_time"] += time.perf_counter() - tic
        return out

    def _search_candidates(self, qb, pool, topk, cand_off, cand_doc, max_count, chunk=None):
        nq, kn = int(qb.shape[0]), self._kernels()
        values = torch.full((nq, topk), float("-inf"), dtype=torch.float32, device=self.device)
        indices = torch.full((nq, topk), -1, dtype=torch.int64, device=self.device)
        if max_count:
            chunk = self.default_chunk(nq) if chunk is None else int(chunk)
            chunk = max(8, min(chunk, (max_count + 7) // 8 * 8))
            self._search_lists(kn, qb, pool, cand_off, cand_doc, max_count, values, indices, chunk)
        return values, indices


class ColBERTIndex(_CentroidPruning, _TokenSearch):
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
        self.centroids = self.tok_centroid = self.cen_off = self.cen_doc = None  # build_centroids / load_centroids
        self._doc_cen = None                                                      # doc_centroids, on first use
        self._init_search(chunk, kernels)

    @property
    def nbytes(self):
        """Bytes of device memory the index holds (token rows and block offsets; with centroids: those, the tokens' assignment and the
        inverted lists; the per-passage centroid lists once doc_centroids has built them)."""
        held = (self.tok, self.doc_blk, self.centroids, self.tok_centroid, self.cen_off, self.cen_doc) + (self._doc_cen or ())
        return sum(t.numel() * t.element_size() for t in held if t is not None)

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

    def compress(self, nbits=2, buckets=None, train_size=65536, seed=0):
        """The ColBERTResidualIndex of this index: every token row replaced by its centroid id -- tok_centroid
        as it is, nothing is re-assigned -- plus `nbits` in {1, 2, 4} bits per feature of row - centroid under ONE bucket set.
        `buckets` = (cutoffs [2^nbits - 1], weights [2^nbits]) trains nothing; otherwise train_buckets on the residuals of a seeded
        sample of `train_size` stored token rows (at most 2^24 / dp of them: torch.quantile's limit of 2^24 elements).  The result
        shares doc_blk, the centroids, tok_centroid and the inverted lists with this index and keeps no reference to the dense rows.
        ValueError without centroids."""
        C, kn, nbits = self._need_centroids(), self._kernels(), _check_res_shape(nbits, self.dp)
        if buckets is None:
            real = torch.nonzero((self.tok_centroid >= 0) & (self.tok_centroid < C)).reshape(-1)
            if not real.numel():
                raise ValueError("no token row with a centroid to train buckets on")
            pick = _sample(int(real.shape[0]), min(int(train_size), QUANTILE_MAX // self.dp), seed)
            rows = real if pick is None else real[pick.to(self.device)]
            buckets = train_buckets(_residuals(self.tok[rows], self.tok_centroid[rows], self.centroids)[:, :self.d], nbits)
        cutoffs, weights = _check_buckets(buckets, nbits, self.device)
        codes = kn.colbert_res_encode(self, cutoffs, nbits)
        return ColBERTResidualIndex.from_packed(codes, self.tok_centroid, self.centroids, cutoffs, weights, self.doc_blk, self.corpus_len,
                                                self.d, cen_off=self.cen_off, cen_doc=self.cen_doc, chunk=self.chunk, kernels=kn)

    # ---- centroid pruning ----
    def build_centroids(self, n_centroids, iters=10, train_size=1 << 18, seed=0, centroids=None):
        """Gives the index `n_centroids` unit-norm centroids (spherical k-means on a seeded sample of `train_size` stored token rows --
        train_centroids -- unless `centroids` [n_centroids, d] are given), assigns every stored token row to argmax_c <tok, centroid_c>
        (bf16 MFMA path, ties to the lower centroid id) and builds the inverted lists.  The index then holds
          centroids     bf16 [C, dp]
          tok_centroid  int32 [n_blk * 16], -1 on padding rows
          cen_off int64 [C + 1], cen_doc int32: per centroid the sorted, duplicate-free doc ids with at least one token there
        The lists come from one device sort (torch.unique of centroid * corpus_len + doc): no host loop over centroids or passages."""
        C, kn = int(n_centroids), self._kernels()
        real = torch.nonzero(_real_rows(self.blk_rows)).reshape(-1)
        if centroids is None:
            if not 1 <= C <= int(real.shape[0]):
                raise ValueError(f"n_centroids={C} out of range (1 .. the index's {int(real.shape[0])} token rows)")
            pick = _sample(int(real.shape[0]), train_size, seed)
            cen = train_centroids(self.tok[real if pick is None else real[pick.to(self.device)]], C, iters=iters, seed=seed, kernels=kn)
        else:
            cen = torch.as_tensor(centroids)
            if cen.dim() != 2 or cen.shape[0] != C or C < 1 or cen.shape[1] != self.d:
                raise ValueError(f"centroids {tuple(cen.shape)}; [{C}, {self.d}] expected")
            cen = _bf16_padded(cen.to(self.device), self.dp)
        tok_centroid = torch.full((self.n_blk * BLOCK,), -1, dtype=torch.int32, device=self.device)
        for lo in range(0, int(real.shape[0]), 1 << 22):
            part = real[lo:lo + (1 << 22)]
            tok_centroid[part] = _nearest(kn, self.tok[part], cen, 1)[:, 0].to(torch.int32)
        self._set_centroids(cen.contiguous(), tok_centroid, *_centroid_lists(tok_centroid, self.doc_blk, C, self.corpus_len))
        return self

    def _score_lists(self, kn, qb, pool, cand_off, cand_doc, pos_begin, cols, S):
        kn.colbert_cand_score(self, qb, pool, cand_off, cand_doc, pos_begin, cols, S)

    def _search_lists(self, kn, qb, pool, cand_off, cand_doc, max_count, values, indices, chunk):
        ws = kn.colbert_cand_workspace(int(qb.shape[0]), chunk, values.shape[1], self.doc_blk)
        kn.colbert_cand_search(self, qb, pool, cand_off, cand_doc, max_count, values, indices, chunk, ws)


def _nearest(kn, rows, centroids, k):
    """int64 [n, k]: the exact top-k rows of `centroids` bf16 [C, dp] for every row of `rows` bf16 [n, dp] by inner product, best
    first, ties to the lower id: hotpath.CorpusSearch (dprhot_search, bf16 MFMA) in batches of 16384 rows."""
    from . import hotpath

    n, C = int(rows.shape[0]), int(centroids.shape[0])
    out = torch.empty((n, int(k)), dtype=torch.int64, device=rows.device)
    chunk = min((C + 7) // 8 * 8, 4096)  # the search workspace is 16384 x chunk x 8 bytes
    for lo in range(0, n, 1 << 14):
        s = hotpath.CorpusSearch(rows[lo:lo + (1 << 14)], int(k), chunk=chunk, kernels=kn)
        s.add(centroids)
        out[lo:lo + (1 << 14)] = s.result()[1]
    return out


def _centroid_lists(tok_centroid, doc_blk, n_centroids, corpus_len):
    """(cen_off int64 [C + 1], cen_doc int32): per centroid the sorted, duplicate-free doc ids with a token assigned to it."""
    dev = tok_centroid.device
    doc_of_blk = torch.repeat_interleave(torch.arange(corpus_len, device=dev), doc_blk[1:] - doc_blk[:-1])
    real = torch.nonzero(tok_centroid >= 0).reshape(-1)
    key = torch.unique(tok_centroid[real].to(torch.int64) * corpus_len + doc_of_blk[real // BLOCK])
    cen_off = torch.zeros(n_centroids + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(key // corpus_len, minlength=n_centroids), 0, out=cen_off[1:])
    return cen_off, (key % corpus_len).to(torch.int32)


def _doc_centroid_lists(tok_centroid, doc_blk, n_centroids, corpus_len):
    """(doc_cen_off int64 [corpus_len + 1], doc_cen int32): per passage the sorted, duplicate-free centroid ids of its stored tokens."""
    dev = tok_centroid.device
    doc_of_blk = torch.repeat_interleave(torch.arange(corpus_len, device=dev), doc_blk[1:] - doc_blk[:-1])
    real = torch.nonzero(tok_centroid >= 0).reshape(-1)
    key = torch.unique(doc_of_blk[real // BLOCK] * n_centroids + tok_centroid[real].to(torch.int64))
    doc_cen_off = torch.zeros(corpus_len + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(key // n_centroids, minlength=corpus_len), 0, out=doc_cen_off[1:])
    return doc_cen_off, (key % n_centroids).to(torch.int32)


def train_centroids(rows, n_centroids, iters=10, seed=0, kernels=None):
    """Unit-norm centroids bf16 [C, dp] of bf16 token rows [n, dp] by spherical k-means, deterministic for a seed:
      init    C rows of a seeded permutation of the sample, normalised
      assign  argmax_c <row, centroid_c> on the bf16 centroids (CorpusSearch, k = 1; ties to the lower id)
      update  fp32 sum of a centroid's rows in sample order by ONE owner (stable sort by centroid, torch.segment_reduce: no floating-point
              atomics), renormalised; an empty cluster is re-seeded with the next unused row of the permutation (wrapping around)."""
    kn = _default_kernels(kernels)
    n, C, dev = int(rows.shape[0]), int(n_centroids), rows.device
    if rows.dtype != _BF16 or rows.dim() != 2 or not 1 <= C <= n:
        raise ValueError(f"rows {rows.dtype} {tuple(rows.shape)} for {C} centroids; bf16 [n >= C, dp] expected")
    order = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed))).to(dev)
    unit = lambda x: x / x.norm(dim=1, keepdim=True).clamp(min=1e-30)
    x = rows.float()
    cen, used = unit(x[order[:C]]).to(_BF16), C
    for _ in range(int(iters)):
        assign = _nearest(kn, rows, cen, 1)[:, 0]
        counts = torch.bincount(assign, minlength=C)
        sums = torch.segment_reduce(x[torch.sort(assign, stable=True).indices], "sum", lengths=counts, axis=0, unsafe=True)
        empty = torch.nonzero(counts == 0).reshape(-1)
        if empty.numel():
            sums[empty] = x[order[(used + torch.arange(empty.numel(), device=dev)) % n]]
            used += int(empty.numel())
        cen = unit(sums).to(_BF16)
    return cen


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

    def search_pruned(self, *args, **kwargs):
        raise NotImplementedError("centroid pruning: dense rows only (the candidate kernel reads ColBERTIndex.tok; decode() gives one)")

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


# ---- residual-compressed token rows under the pruned search ------------------------------------------------

RES_NBITS = (1, 2, 4)         # bits per feature of row - centroid
RES_MAX_DP = 128              # dprhot_colbert_res_score keeps the query fragments and a block's raw operands in registers
QUANTILE_MAX = 1 << 24        # torch.quantile's limit on the elements of its input


def _check_res_shape(nbits, dp):
    if nbits not in RES_NBITS:
        raise ValueError(f"nbits={nbits!r}: {RES_NBITS} bits per feature")
    if dp > RES_MAX_DP:
        raise NotImplementedError(f"dp={dp}: the residual index is built for dp <= {RES_MAX_DP}")
    return int(nbits)


def _check_buckets(buckets, nbits, device):
    """(cutoffs fp32 [2^nbits - 1], weights fp32 [2^nbits]) on `device`, contiguous."""
    cutoffs, weights = (torch.as_tensor(t).detach().to(device, torch.float32).contiguous() for t in buckets)
    if cutoffs.shape != ((1 << nbits) - 1,) or weights.shape != (1 << nbits,):
        raise ValueError(f"buckets {tuple(cutoffs.shape)} / {tuple(weights.shape)}; cutoffs [{(1 << nbits) - 1}] and weights [{1 << nbits}] "
                         f"expected for nbits={nbits}")
    return cutoffs, weights


def _residuals(rows, tok_centroid, centroids):
    """fp32 [n, dp]: float(row) - float(its centroid), one fp32 subtraction; the ids must lie in [0, C)."""
    return rows.float() - centroids[tok_centroid.long()].float()


def train_buckets(residuals, nbits):
    """(cutoffs fp32 [2^nbits - 1], weights fp32 [2^nbits]) of fp32 residuals (any shape, flattened; at most 2^24 elements) by
    torch.quantile: the cutoffs are the quantiles j / 2^nbits, j = 1 .. 2^nbits - 1, the weights the quantiles (j + 1/2) / 2^nbits,
    j = 0 .. 2^nbits - 1 -- ColBERTv2's one bucket set per index."""
    if nbits not in RES_NBITS:
        raise ValueError(f"nbits={nbits!r}: {RES_NBITS} bits per feature")
    x = torch.as_tensor(residuals).detach().float().reshape(-1)
    if not 0 < x.numel() <= QUANTILE_MAX:
        raise ValueError(f"{x.numel()} residuals; 1 .. 2^24 (torch.quantile's limit) expected")
    nb = 1 << int(nbits)
    cutoffs = torch.quantile(x, torch.arange(1, nb, device=x.device, dtype=torch.float32) / nb)
    weights = torch.quantile(x, (torch.arange(nb, device=x.device, dtype=torch.float32) + 0.5) / nb)
    return cutoffs, weights


def res_unpack(res_code, nbits):
    """int64 [n, rb * 8 / nbits]: code(r, t) = (res_code[r, t * nbits / 8] >> (nbits * (t mod (8 / nbits)))) & (2^nbits - 1)."""
    per = 8 // nbits
    shifts = torch.arange(per, device=res_code.device, dtype=torch.int64) * nbits
    return ((res_code.to(torch.int64).unsqueeze(2) >> shifts) & ((1 << nbits) - 1)).reshape(res_code.shape[0], -1)


class ColBERTResidualIndex(_CentroidPruning, _TokenSearch):
    """Token index in the ColBERTv2 format: per row its centroid id (tok_centroid int32 [n_blk * 16]) and `nbits` bits per feature of
    row - centroid (res_code uint8 [n_blk * 16, dp * nbits / 8]) under ONE bucket set (cutoffs, weights) instead of tok.  Searched with
    centroid pruning only -- probe, candidates, score_candidates, approx_candidates, prune_candidates, search_pruned -- and every
    result is, bit for bit, what `decode()` returns for the same call."""

    FORMAT = "dpr_scale_amd.colbert_res/1"

    def __init__(self, *args, **kwargs):
        raise TypeError("a ColBERTResidualIndex comes from ColBERTIndex.compress, ColBERTResidualIndex.from_packed, load_residual_index "
                        "or a quantizer='residual' build")

    @classmethod
    def from_packed(cls, res_code, tok_centroid, centroids, cutoffs, weights, doc_blk, corpus_len, d, cen_off=None, cen_doc=None,
                    chunk=None, kernels=None):
        """From tensors in the device layout (csrc/colbert_res.h), on their device.  The inverted lists default to the lists of
        tok_centroid (ids outside [0, C) belong to no list)."""
        self = cls.__new__(cls)
        corpus_len, C, dp = int(corpus_len), int(centroids.shape[0]), int(centroids.shape[1])
        assert cutoffs.dtype == torch.float32 and weights.dtype == torch.float32 and weights.dim() == 1
        nbits = int(weights.shape[0]).bit_length() - 1
        _check_res_shape(nbits, dp)
        _check_buckets((cutoffs, weights), nbits, weights.device)
        assert res_code.dtype == torch.uint8 and res_code.dim() == 2 and res_code.shape[1] == dp * nbits // 8 and dp % 32 == 0
        assert res_code.shape[0] % BLOCK == 0 and doc_blk.dtype == torch.int64 and doc_blk.shape[0] == corpus_len + 1
        assert all(t.is_contiguous() for t in (res_code, tok_centroid, centroids, cutoffs, weights, doc_blk))
        self.device = doc_blk.device
        self.res_code, self.cutoffs, self.weights, self.doc_blk = res_code, cutoffs, weights, doc_blk
        self.corpus_len, self.d, self.dp, self.nbits = corpus_len, int(d), dp, nbits
        self.n_blk = int(res_code.shape[0]) // BLOCK
        if cen_off is None:
            inside = torch.where(tok_centroid < C, tok_centroid, torch.full_like(tok_centroid, -1))
            cen_off, cen_doc = _centroid_lists(inside, doc_blk, C, corpus_len)
        self._set_centroids(centroids, tok_centroid, cen_off, cen_doc)
        self._init_search(chunk, kernels)
        return self

    def _tensors(self):
        return dict(res_code=self.res_code, tok_centroid=self.tok_centroid, centroids=self.centroids, cutoffs=self.cutoffs,
                    weights=self.weights, doc_blk=self.doc_blk, cen_off=self.cen_off, cen_doc=self.cen_doc)

    @property
    def nbytes(self):
        """Bytes of device memory the index holds: codes, centroid ids, centroids, inverted lists, buckets and block offsets (and the
        per-passage centroid lists once doc_centroids has built them)."""
        return sum(t.numel() * t.element_size() for t in tuple(self._tensors().values()) + (self._doc_cen or ()))

    def decode(self, rows_per_pass=1 << 20):
        """The ColBERTIndex this one searches, by definition: tok[r, t] = bf16(float(centroids[tok_centroid[r], t]) + weights[code(r, t)])
        -- one fp32 addition, round to nearest even -- and an exact zero row where tok_centroid[r] lies outside [0, C); the same four
        centroid tensors, nothing re-assigned."""
        C = int(self.centroids.shape[0])
        tok = torch.zeros((self.n_blk * BLOCK, self.dp), dtype=_BF16, device=self.device)
        for lo in range(0, self.n_blk * BLOCK, int(rows_per_pass)):
            tc = self.tok_centroid[lo:lo + rows_per_pass].long()
            ok = (tc >= 0) & (tc < C)
            part = (self.centroids[tc.clamp(0, C - 1)].float() + self.weights[res_unpack(self.res_code[lo:lo + rows_per_pass], self.nbits)])
            tok[lo:lo + rows_per_pass] = torch.where(ok.unsqueeze(1), part.to(_BF16), torch.zeros((), dtype=_BF16, device=self.device))
        dense = ColBERTIndex.from_packed(tok, self.doc_blk, self.corpus_len, self.d, chunk=self.chunk, kernels=self.kn)
        dense._set_centroids(self.centroids, self.tok_centroid, self.cen_off, self.cen_doc)
        return dense

    def _score_lists(self, kn, qb, pool, cand_off, cand_doc, pos_begin, cols, S):
        kn.colbert_res_score(self, qb, pool, cand_off, cand_doc, pos_begin, cols, S)

    def _search_lists(self, kn, qb, pool, cand_off, cand_doc, max_count, values, indices, chunk):
        ws = kn.colbert_res_workspace(int(qb.shape[0]), chunk, values.shape[1], self.doc_blk)
        kn.colbert_res_search(self, qb, pool, cand_off, cand_doc, max_count, values, indices, chunk, ws)

    def _exhaustive(self, *args, **kwargs):
        raise NotImplementedError("the residual index is searched with centroid pruning only (search_pruned); decode() gives the dense "
                                  "index it stands for")

    search = score = compress = quantize = _exhaustive

    def save(self, path):
        """One torch.save of the tensors (on the CPU) and sizes; load_residual_index reads it back."""
        blob = {k: t.cpu() for k, t in self._tensors().items()}
        blob.update(format=self.FORMAT, corpus_len=self.corpus_len, d=self.d, nbits=self.nbits)
        torch.save(blob, path)
        return path


def load_residual_index(path, device=None, chunk=None, kernels=None):
    """The ColBERTResidualIndex that ColBERTResidualIndex.save wrote, placed on `device`."""
    device = torch.device(device) if device is not None else torch.device("cuda", 0)
    blob = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(blob, dict) or blob.get("format") != ColBERTResidualIndex.FORMAT:
        raise ValueError(f"{path}: not a residual ColBERT index file")
    t = {k: blob[k].contiguous().to(device) for k in ("res_code", "tok_centroid", "centroids", "cutoffs", "weights", "doc_blk", "cen_off",
                                                       "cen_doc")}
    return ColBERTResidualIndex.from_packed(t["res_code"], t["tok_centroid"], t["centroids"], t["cutoffs"], t["weights"], t["doc_blk"],
                                            blob["corpus_len"], blob["d"], cen_off=t["cen_off"], cen_doc=t["cen_doc"], chunk=chunk,
                                            kernels=kernels)


def _walk_parts(parts, need_sample, train_size, gen):
    """One walk over parts(): (ids, lengths, d, sample) -- the layout's inputs and, when asked for, a seeded sample of at most
    train_size token rows (bf16, on the host; the train_size smallest of one uniform key per row, in corpus order)."""
    ids, lens, keys, sample, d = [], [], [], [], None
    for i, n, r in parts():
        i, n, r = torch.as_tensor(i).reshape(-1).long().cpu(), torch.as_tensor(n).reshape(-1).long().cpu(), torch.as_tensor(r)
        if r.dim() != 2 or i.shape != n.shape or int(n.sum()) != r.shape[0] or (d is not None and r.shape[1] != d):
            raise ValueError(f"ids {tuple(i.shape)}, lengths {tuple(n.shape)} and rows {tuple(r.shape)} do not belong together")
        d = int(r.shape[1])
        ids.append(i)
        lens.append(n)
        if need_sample and r.shape[0]:
            key = torch.rand(r.shape[0], generator=gen, dtype=torch.float64)
            keep = torch.sort(key, stable=True).indices[:train_size].sort().values
            keys.append(key[keep])
            sample.append(r[keep.to(r.device)].to(_BF16).cpu())
    if d is None:
        raise ValueError("no token rows to build an index from")
    rows = torch.cat(sample, 0) if sample else torch.zeros((0, d), dtype=_BF16)
    if rows.shape[0] > train_size:
        rows = rows[torch.sort(torch.cat(keys), stable=True).indices[:train_size].sort().values]
    return torch.cat(ids), torch.cat(lens), d, rows


def _build_residual(parts, corpus_len, device, nbits, n_centroids, centroids, buckets, train_kwargs, chunk, kernels):
    """The ColBERTResidualIndex of the passages that parts() yields as (ids, lengths, rows) pieces -- in every tensor
    ColBERTIndex(all of them).build_centroids(C, centroids=the centroids).compress(nbits, buckets=the buckets) -- with never more than
    ONE piece's dense rows on the device.  parts() is walked twice: layout and one seeded sample of token rows, on which the centroids
    (train_centroids) and the buckets (train_buckets, on at most 2^24 / dp of its rows) are trained unless given; then every piece is
    assigned and encoded, and the inverted lists are built from tok_centroid."""
    corpus_len, device = int(corpus_len), torch.device(device)
    if not 0 < corpus_len < 2 ** 31:
        raise ValueError(f"corpus_len={corpus_len} out of range (1 .. 2^31 - 1)")
    if n_centroids is None and centroids is None:
        raise ValueError("quantizer='residual' needs n_centroids (or centroids)")
    kn = _default_kernels(kernels)
    unknown = sorted(set(train_kwargs) - {"train_size", "seed", "iters"})
    if unknown or (centroids is not None and buckets is not None and train_kwargs):
        raise TypeError(f"nothing to train with {unknown or sorted(train_kwargs)}")
    train_size, seed = int(train_kwargs.get("train_size", 65536)), int(train_kwargs.get("seed", 0))
    ids, lens, d, sample = _walk_parts(parts, centroids is None or buckets is None, train_size, torch.Generator().manual_seed(seed))
    dp = (max(d, 1) + 31) // 32 * 32
    nbits = _check_res_shape(nbits, dp)
    sample = _bf16_padded(sample.to(device), dp)
    if centroids is None:
        C = int(n_centroids)
        if not 1 <= C <= int(sample.shape[0]):
            raise ValueError(f"n_centroids={C} out of range (1 .. the sample's {int(sample.shape[0])} token rows)")
        cen = train_centroids(sample, C, iters=int(train_kwargs.get("iters", 10)), seed=seed, kernels=kn)
    else:
        cen = torch.as_tensor(centroids)
        C = int(cen.shape[0]) if n_centroids is None else int(n_centroids)
        if cen.dim() != 2 or cen.shape[0] != C or C < 1 or cen.shape[1] != d:
            raise ValueError(f"centroids {tuple(cen.shape)}; [{C}, {d}] expected")
        cen = _bf16_padded(cen.to(device), dp)
    cen = cen.contiguous()
    if buckets is None:
        if not sample.shape[0]:
            raise ValueError("no token row to train buckets on")
        pick = _sample(int(sample.shape[0]), QUANTILE_MAX // dp, seed)
        rows = sample if pick is None else sample[pick.to(device)]
        buckets = train_buckets(_residuals(rows, _nearest(kn, rows, cen, 1)[:, 0], cen)[:, :d], nbits)
    cutoffs, weights = _check_buckets(buckets, nbits, device)
    _, _, _, doc_blk = _layout(ids, lens, corpus_len, device)
    n_rows = int(doc_blk[-1]) * BLOCK
    res_code = torch.zeros((n_rows, dp * nbits // 8), dtype=torch.uint8, device=device)
    tok_centroid = torch.full((n_rows,), -1, dtype=torch.int32, device=device)
    for i, n, r in parts():
        r = torch.as_tensor(r)
        if r.shape[0]:
            dest = _dest_rows(doc_blk, torch.as_tensor(i).reshape(-1).to(device, torch.int64), torch.as_tensor(n).reshape(-1).to(device, torch.int64))
            rows = _bf16_padded(r.to(device), dp)
            tc = _nearest(kn, rows, cen, 1)[:, 0].to(torch.int32)
            res_code[dest] = kn.colbert_res_encode(rows, cutoffs, nbits, tc, cen)
            tok_centroid[dest] = tc
    return ColBERTResidualIndex.from_packed(res_code, tok_centroid, cen, cutoffs, weights, doc_blk, corpus_len, d, chunk=chunk, kernels=kn)


def _plain(quantizer, codebook, train_kwargs):
    """True for quantizer=None (with nothing to quantise with), False for "pq" and "residual"."""
    if quantizer in (None, "None"):
        if codebook is not None or train_kwargs:
            raise TypeError(f"quantizer=None takes no codebook and no training arguments {sorted(train_kwargs)}")
        return True
    if quantizer not in ("pq", "residual"):
        raise NotImplementedError(f"quantizer={quantizer!r}: None, 'pq' or 'residual'")
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

    def finish(self, chunk=None, quantizer=None, sub_vec_dim=8, codebook=None, nbits=2, n_centroids=None, centroids=None, buckets=None,
               **train_kwargs):
        """The index of the batches added so far.  quantizer="pq": a ColBERTPQIndex (sub_vec_dim in {2, 4, 8}; a codebook, or
        train_pq(**train_kwargs) on a seeded sample), encoded batch by batch -- the batches are never concatenated.
        quantizer="residual": a ColBERTResidualIndex (nbits in {1, 2, 4}; n_centroids trained on a seeded sample, or `centroids`;
        `buckets` or trained ones), assigned and encoded batch by batch."""
        if self.corpus_len is None:
            raise ValueError("corpus_len is needed to build the index")
        if not _plain(quantizer, codebook, _residual_args(quantizer, train_kwargs, n_centroids, centroids, buckets)):
            if not self.parts:
                raise ValueError("no context batch was added")
            device = self.parts[0][2].device if self.device is None else self.device
            if quantizer == "residual":
                return _build_residual(lambda: iter(self.parts), self.corpus_len, device, nbits, n_centroids, centroids, buckets, train_kwargs,
                                       chunk, self.kn)
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


def _residual_args(quantizer, train_kwargs, n_centroids, centroids, buckets):
    """train_kwargs as _plain judges them: with any other quantizer the residual build's arguments count as training arguments."""
    if quantizer == "residual":
        return train_kwargs
    given = {k: v for k, v in dict(n_centroids=n_centroids, centroids=centroids, buckets=buckets).items() if v is not None}
    if given and quantizer not in (None, "None"):
        raise TypeError(f"quantizer={quantizer!r} takes no {sorted(given)}")
    return dict(train_kwargs, **given)


def load_index(ctx_embeddings_dir, corpus_len, device=None, chunk=None, kernels=None, quantizer=None, sub_vec_dim=8, codebook=None,
               nbits=2, n_centroids=None, centroids=None, buckets=None, **train_kwargs):
    """Reads every `tokens_{rank:04}.pkl` under `ctx_embeddings_dir` and merges all ranks' passages by doc id into ONE index on `device`.

    quantizer="pq" (sub_vec_dim in {2, 4, 8}): a ColBERTPQIndex under `codebook`, or under train_pq(**train_kwargs) of a seeded sample
    of token rows taken across the files; the files are read one at a time (twice) and encoded one at a time, so the device never holds
    more than one file's dense rows.

    quantizer="residual" (nbits in {1, 2, 4}): a ColBERTResidualIndex over `n_centroids` centroids trained on
    a seeded sample of token rows taken across the files (train_size, seed, iters), or over `centroids`; the buckets are `buckets` or
    trained on the same sample.  The files are read one at a time (twice), assigned and encoded one at a time."""
    device = torch.device(device) if device is not None else torch.device("cuda", 0)
    if not _plain(quantizer, codebook, _residual_args(quantizer, train_kwargs, n_centroids, centroids, buckets)):
        files = _token_files(ctx_embeddings_dir)
        if quantizer == "residual":
            return _build_residual(lambda: (_read_token_file(path) for path in files), corpus_len, device, nbits, n_centroids, centroids,
                                   buckets, train_kwargs, chunk, kernels)
        return _build_pq(lambda: (_read_token_file(path) for path in files), corpus_len, device, sub_vec_dim, codebook, train_kwargs, chunk,
                         kernels)
    ids, lens, rows = read_tokens(ctx_embeddings_dir)
    return ColBERTIndex(ids, lens, rows, corpus_len, device, chunk=chunk, kernels=kernels)
