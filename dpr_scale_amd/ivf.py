"""Inverted-index retrieval for CITADEL and COIL -- the `index.search` that dpr_scale/task/citadel_retrieval_task.py:136 calls on
an `IVFGPUIndex` from dpr_scale/index/inverted_vector_index.py, a module the reference imports but does not ship.

    score(n, doc) = sum over entries (e, u) of query n of  max(0, max over postings (doc, v) of expert e of <u, v>)
                  + <cls_q[n], cls_doc[doc]>                                  (only when the index has CLS vectors)

On-disk index (what citadel_eval_task.py:76-120 writes): `expert_{rank:04}/{expert_id}.pkl`, each a pickled tuple
(ids int64 [n], weights fp32 [n], reprs fp32 [n, d]) with reprs = expert_weight * expert_repr, and `cls_{rank:04}.pkl`, a pickled
fp32 [n_docs_of_rank, dc] tensor.  Query side (citadel_retrieval_task.py:104-136): per query a dict {expert_id: [vector, ...]} of
weighted vectors (fp16 for CITADEL, fp32 for COIL), the same for the weights, and a [B, dc] tensor or an empty list of CLS vectors.

Precision: operands are rounded to bf16 once (round to nearest even) when the index and the query batch are packed; products are
exact in fp32 and accumulation is fp32 (csrc/ivf.h).  Scoring and top-k run in libdprhot.so (dprhot_ivf_search);
there is no torch fallback.

Not supported (NotImplementedError / out of scope): product quantisation, `portion` < 1, hnsw, expert parallelism across GPUs, ColBERT.
"""
import collections
import glob
import os
import pickle
import re
import time

import torch

_BF16 = torch.bfloat16
MAX_ENTRIES_PER_QUERY = 4096  # dprhot_ivf_search's limit
KNARROW = 4096                # largest k of dprhot_topk_update; beyond it the HBM-resident selection runs


def _pad_cols(x, mult):
    pad = (-x.shape[1]) % mult
    if pad:
        x = torch.cat([x, torch.zeros((x.shape[0], pad), dtype=x.dtype)], 1)
    return x


class QueryBatch:
    """One packed query batch (CPU tensors until .to(device)): entries sorted by (expert, query, slot)."""

    def __init__(self, nq, ent_vec, ent_q, bexp, boff, cls):
        self.nq, self.ent_vec, self.ent_q, self.bexp, self.boff, self.cls = nq, ent_vec, ent_q, bexp, boff, cls

    @property
    def n_entries(self):
        return int(self.ent_q.shape[0])

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device)
        return QueryBatch(self.nq, mv(self.ent_vec), mv(self.ent_q), mv(self.bexp), mv(self.boff), mv(self.cls))


def pack_queries(batch_cls, batch_embeddings, batch_weights=None, d=None):
    """Packs what CITADELRetrievalTask._eval_step hands to index.search.  `batch_weights` is accepted for the call's shape only: the
    vectors already carry their weights.  `d`: feature count when the batch has no entry at all."""
    nq = len(batch_embeddings)
    if nq == 0:
        raise ValueError("empty query batch")
    if batch_weights is not None and len(batch_weights) != nq:
        raise ValueError("batch_weights and batch_embeddings differ in length")
    keys, vecs = [], []
    for n, by_expert in enumerate(batch_embeddings):
        count = 0
        for e, lst in by_expert.items():
            for v in lst:
                keys.append((int(e), n))
                vecs.append(torch.as_tensor(v).detach().reshape(-1))
                count += 1
        if count > MAX_ENTRIES_PER_QUERY:
            raise ValueError(f"query {n} has {count} entries; at most {MAX_ENTRIES_PER_QUERY} are supported")
    if vecs:
        d = vecs[0].shape[0]
        # fp16 -> fp32 is exact, so the one rounding is the final one to bf16 (RNE)
        x = torch.stack([v.to("cpu", torch.float32) for v in vecs], 0)
        order = sorted(range(len(keys)), key=lambda i: keys[i])  # stable: the listed order survives inside (expert, query)
        x = _pad_cols(x[order], 32).to(_BF16).contiguous()
        ks = [keys[i] for i in order]
        ent_q = torch.tensor([k[1] for k in ks], dtype=torch.int32)
        bexp, boff = [], []
        for i, (e, _) in enumerate(ks):
            if not bexp or bexp[-1] != e:
                bexp.append(e)
                boff.append(i)
        boff.append(len(ks))
        if bexp[0] < 0 or bexp[-1] >= 2 ** 31:
            raise ValueError("expert ids must fit a non-negative int32")
    else:
        dp = (max(int(d or 32), 1) + 31) // 32 * 32
        x = torch.zeros((0, dp), dtype=_BF16)
        ent_q = torch.zeros(0, dtype=torch.int32)
        bexp, boff = [], [0]
    cls = None
    if torch.is_tensor(batch_cls) and batch_cls.numel() > 0:
        if batch_cls.shape[0] != nq:
            raise ValueError("batch_cls and batch_embeddings differ in length")
        cls = _pad_cols(batch_cls.detach().to("cpu", torch.float32), 8).to(_BF16).contiguous()
    return QueryBatch(nq, x, ent_q, torch.tensor(bexp, dtype=torch.int32), torch.tensor(boff, dtype=torch.int32), cls)


def _read_pickle(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def read_postings(ctx_embeddings_dir, corpus_len):
    """Reads and merges every shard directory.  Returns (expert int64 [P], doc int64 [P], vec fp32 [P, d], cls fp32 [corpus_len, dc]
    or None), postings in (shard directory, expert file, file order) order -- unsorted."""
    dirs = sorted(p for p in glob.glob(os.path.join(ctx_embeddings_dir, "expert_*")) if os.path.isdir(p))
    if not dirs:
        raise FileNotFoundError(f"no expert_* directory under {ctx_embeddings_dir}")
    cls_files = sorted(glob.glob(os.path.join(ctx_embeddings_dir, "cls_*.pkl")))
    cls_parts = [torch.as_tensor(_read_pickle(p)).float() for p in cls_files]
    bounds = None
    if cls_parts:
        tags = lambda paths: [re.search(r"_(\d+)(?:\.pkl)?$", os.path.basename(p)).group(1) for p in paths]
        if tags(cls_files) != tags(dirs):
            raise ValueError(f"CLS files {tags(cls_files)} and expert directories {tags(dirs)} do not belong to the same ranks")
        edges = [0]
        for c in cls_parts:
            edges.append(edges[-1] + c.shape[0])
        if edges[-1] != corpus_len:
            raise ValueError(f"the CLS files hold {edges[-1]} rows, the corpus has {corpus_len} passages: cannot map rows to doc ids")
        bounds = list(zip(edges[:-1], edges[1:]))
    experts, docs, vecs = [], [], []
    for r, dpath in enumerate(dirs):
        files = glob.glob(os.path.join(dpath, "*.pkl"))
        for path in sorted(files, key=lambda p: int(os.path.basename(p)[:-4])):
            e = int(os.path.basename(path)[:-4])
            ids, _weights, reprs = _read_pickle(path)
            ids, reprs = torch.as_tensor(ids).long().reshape(-1), torch.as_tensor(reprs).float()
            if reprs.dim() != 2 or reprs.shape[0] != ids.shape[0]:
                raise ValueError(f"{path}: ids {tuple(ids.shape)} and reprs {tuple(reprs.shape)} do not match")
            if ids.numel() == 0:
                continue
            lo, hi = bounds[r] if bounds else (0, corpus_len)
            if int(ids.min()) < lo or int(ids.max()) >= hi:
                raise ValueError(f"{path}: doc ids outside [{lo}, {hi})"
                                 + (": the ids are not the row numbers of the concatenated CLS files" if bounds else ""))
            experts.append(torch.full_like(ids, e))
            docs.append(ids)
            vecs.append(reprs)
    if not docs:
        raise ValueError(f"no posting under {ctx_embeddings_dir}")
    if len({v.shape[1] for v in vecs}) != 1:
        raise ValueError("posting vectors of different widths")
    return torch.cat(experts), torch.cat(docs), torch.cat(vecs, 0), (torch.cat(cls_parts, 0) if cls_parts else None)


class IVFIndex:
    """Device-resident inverted index; `search` stands where the reference's IVFGPUIndex.search stood."""

    def __init__(self, experts, docs, vecs, cls, corpus_len, device, chunk=None, kernels=None):
        """From unsorted CPU postings: expert int64 [P], doc int64 [P], vec fp32 [P, d], cls fp32 [corpus_len, dc] or None."""
        corpus_len = int(corpus_len)
        if not 0 < corpus_len < 2 ** 31:
            raise ValueError(f"corpus_len={corpus_len} out of range (1 .. 2^31 - 1)")
        if docs.numel() and (int(docs.min()) < 0 or int(docs.max()) >= corpus_len or int(experts.min()) < 0):
            raise ValueError("doc ids must lie in [0, corpus_len) and expert ids must be non-negative")
        if experts.numel() and int(experts.max()) >= 2 ** 31 - 1:
            raise ValueError("expert ids must fit int32")
        # (expert, doc) order; the stable sort keeps file order among the postings of one doc
        order = torch.sort(experts * corpus_len + docs, stable=True).indices
        device = torch.device(device)
        n_experts = int(experts.max()) + 1 if experts.numel() else 1
        counts = torch.bincount(experts, minlength=n_experts) if experts.numel() else torch.zeros(1, dtype=torch.int64)
        exp_off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
        cls_dev = None
        if cls is not None:
            if cls.shape[0] != corpus_len:
                raise ValueError(f"{cls.shape[0]} CLS rows for {corpus_len} passages")
            c = _pad_cols(cls.float(), 8).to(_BF16)
            # dprhot_ivf_search scores whole groups of 8 rows: zero rows behind the corpus
            cls_dev = torch.cat([c, torch.zeros((8, c.shape[1]), dtype=_BF16)], 0).contiguous().to(device)
        self._set(docs[order].to(torch.int32).contiguous().to(device), _pad_cols(vecs[order].float(), 32).to(_BF16).contiguous().to(device),
                  exp_off.contiguous().to(device), cls_dev, corpus_len, int(vecs.shape[1]), chunk, kernels)

    @classmethod
    def from_packed(cls, post_doc, post_vec, exp_off, cls_rows, corpus_len, d, chunk=None, kernels=None):
        """From tensors already in the device layout (csrc/ivf.h), on their device: post_doc int32 [P] sorted by (expert, doc), post_vec
        bf16 [P, dp], exp_off int64 [V + 1], cls_rows bf16 [>= corpus_len + 7, dc] with zero rows behind the corpus, or None."""
        self = cls.__new__(cls)
        self._set(post_doc, post_vec, exp_off, cls_rows, int(corpus_len), int(d), chunk, kernels)
        return self

    def _set(self, post_doc, post_vec, exp_off, cls_rows, corpus_len, d, chunk, kernels):
        assert post_doc.dtype == torch.int32 and post_vec.dtype == _BF16 and exp_off.dtype == torch.int64 and post_vec.shape[1] % 32 == 0
        self.device = post_doc.device
        self.corpus_len, self.d = corpus_len, d
        self.n_experts, self.n_postings = int(exp_off.shape[0]) - 1, int(post_doc.shape[0])
        self.post_doc, self.post_vec, self.exp_off = post_doc, post_vec, exp_off
        self.dp = int(post_vec.shape[1])
        self.cls, self.dc = cls_rows, (0 if cls_rows is None else int(cls_rows.shape[1]))
        self.chunk = None if chunk is None else int(chunk)
        self.kn = kernels
        self.latency = collections.defaultdict(float)
        self.latency["encode_time"] += 0.0  # test_epoch_end of the retrieval task pops this key

    def _kernels(self):
        if self.kn is None:
            from . import hotpath

            self.kn = hotpath.default_kernels()
        return self.kn

    def default_chunk(self, nq):
        """Doc ids per pass: the chunk's score buffer is nq x chunk fp32 (at most 8 MiB by default, at least 1024 ids)."""
        c = self.chunk if self.chunk is not None else max(1024, min(262144, (1 << 21) // max(nq, 1)))
        c = min(c, (self.corpus_len + 7) // 8 * 8)
        return max(8, c // 8 * 8)

    def search_packed(self, qb, topk, id_ranges=None, chunk=None):
        """(scores [nq, topk] fp32, ids [nq, topk] int64) for a packed batch on the index's device.  `id_ranges`: disjoint
        (begin, end) doc-id ranges folded into one result (default: the whole corpus)."""
        topk = int(topk)
        if not 1 <= topk <= self.corpus_len:
            raise ValueError(f"topk={topk} out of range (1 .. corpus_len={self.corpus_len})")
        if (qb.cls is None) != (self.cls is None):
            raise ValueError("CLS vectors on one side only: the index and the queries must both have them or both lack them")
        if qb.cls is not None and qb.cls.shape[1] != self.dc:
            raise ValueError(f"query CLS width {qb.cls.shape[1]} != index CLS width {self.dc}")
        if qb.n_entries and qb.ent_vec.shape[1] != self.dp:
            raise ValueError(f"query vectors of padded width {qb.ent_vec.shape[1]}, index of {self.dp}")
        kn = self._kernels()
        qb = qb.to(self.device)
        chunk = self.default_chunk(qb.nq) if chunk is None else int(chunk)
        values = torch.empty((qb.nq, topk), dtype=torch.float32, device=self.device)
        indices = torch.empty((qb.nq, topk), dtype=torch.int64, device=self.device)
        ws = kn.ivf_workspace(qb.nq, qb.n_entries, chunk, self.cls is not None, topk, self.post_doc)
        first = True
        for b, e in (id_ranges if id_ranges is not None else [(0, self.corpus_len)]):
            kn.ivf_search(self, qb, int(b), int(e), values, indices, first, chunk, ws)
            first = False
        return values, indices

    def search(self, batch_cls, batch_embeddings, batch_weights, topk, id_ranges=None, chunk=None):
        tic = time.perf_counter()
        qb = pack_queries(batch_cls, batch_embeddings, batch_weights, d=self.d)
        self.latency["encode_time"] += time.perf_counter() - tic
        tic = time.perf_counter()
        out = self.search_packed(qb, topk, id_ranges=id_ranges, chunk=chunk)
        self.latency["search_time"] += time.perf_counter() - tic
        return out


def load_index(ctx_embeddings_dir, corpus_len, device=None, chunk=None, kernels=None):
    """Reads every `expert_*/{id}.pkl` and `cls_*.pkl` under `ctx_embeddings_dir`, merges the shard directories into ONE index (a
    doc's score is a sum over experts: shards are never searched one by one) and places it on `device`.

    Doc ids are the corpus ids the writer stored.  With CLS files they must equal the row numbers of the CLS files concatenated in rank
    order (rank r's ids inside rank r's rows, all rows together = corpus_len); an index for which that does not hold raises."""
    device = torch.device(device) if device is not None else torch.device("cuda", 0)
    experts, docs, vecs, cls = read_postings(ctx_embeddings_dir, int(corpus_len))
    return IVFIndex(experts, docs, vecs, cls, corpus_len, device, chunk=chunk, kernels=kernels)
