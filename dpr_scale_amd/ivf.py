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

Building both sides on the device ("Building postings and query batches"): `pack_queries_device` makes the
packed query batch and `IndexBuilder` the postings -- the on-disk tree above or an IVFIndex -- straight from the encoders' repr tensors,
with the kept slots listed and the weighted vectors written by libdprhot.so (dprhot_ivf_compact / dprhot_ivf_gather) in the order and
with the roundings of the host loops they replace.

Product quantisation (the reference's quantizer="pq", sub_vec_dim): `IVFIndex.quantize` / `load_index(...,
quantizer="pq")` / `IndexBuilder.finish(quantizer="pq")` give an `IVFPQIndex` whose postings are 8-bit codes over sub-vectors of 2, 4
or 8 features and one bf16 codebook; its search returns, bit for bit, the dense search over the decoded rows (`IVFPQIndex.decode`).

Not supported (NotImplementedError / out of scope): per-expert codebooks, code widths other than 8 bits, a product-quantised index
for dp > 64 or on the CPU, `portion` < 1, hnsw, expert parallelism across GPUs.  ColBERT (no expert ids to index by) is searched by
dpr_scale_amd/colbert.py.
"""
import collections
import glob
import os
import pickle
import re
import time

import torch

from ._chunked import ChunkedIndex, _default_kernels

_BF16 = torch.bfloat16
MAX_ENTRIES_PER_QUERY = 4096  # dprhot_ivf_search's limit


def _pad_cols(x, mult):
    pad = (-x.shape[1]) % mult
    if pad:
        x = torch.cat([x, torch.zeros((x.shape[0], pad), dtype=x.dtype, device=x.device)], 1)
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


class IVFIndex(ChunkedIndex):
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

    def _set_frame(self, post_doc, exp_off, cls_rows, corpus_len, d, dp, chunk, kernels):
        """Everything but the posting rows themselves, which the dense and the product-quantised index hold in their own form."""
        assert post_doc.dtype == torch.int32 and exp_off.dtype == torch.int64
        self.device = post_doc.device
        self.corpus_len, self.d, self.dp = corpus_len, d, dp
        self.n_experts, self.n_postings = int(exp_off.shape[0]) - 1, int(post_doc.shape[0])
        self.post_doc, self.exp_off = post_doc, exp_off
        self.cls, self.dc = cls_rows, (0 if cls_rows is None else int(cls_rows.shape[1]))
        self._init_search(chunk, kernels)

    def _set(self, post_doc, post_vec, exp_off, cls_rows, corpus_len, d, chunk, kernels):
        assert post_vec.dtype == _BF16 and post_vec.shape[1] % 32 == 0
        self._set_frame(post_doc, exp_off, cls_rows, corpus_len, d, int(post_vec.shape[1]), chunk, kernels)
        self.post_vec = post_vec

    @property
    def nbytes(self):
        """Bytes of device memory the index holds (posting rows, doc ids, offsets, CLS rows)."""
        return sum(t.numel() * t.element_size() for t in (self.post_doc, self.post_vec, self.exp_off, self.cls) if t is not None)

    def _search_range(self, kn, qb, *tail):
        """One doc-id range through the index's search kernel (the product-quantised index has its own)."""
        kn.ivf_search(self, qb, *tail)

    def search_packed(self, qb, topk, id_ranges=None, chunk=None):
        """(scores [nq, topk] fp32, ids [nq, topk] int64) for a packed batch on the index's device.  `id_ranges`: disjoint
        (begin, end) doc-id ranges folded into one result (default: the whole corpus)."""
        topk = int(topk)
        if (qb.cls is None) != (self.cls is None):
            raise ValueError("CLS vectors on one side only: the index and the queries must both have them or both lack them")
        if qb.cls is not None and qb.cls.shape[1] != self.dc:
            raise ValueError(f"query CLS width {qb.cls.shape[1]} != index CLS width {self.dc}")
        if qb.n_entries and qb.ent_vec.shape[1] != self.dp:
            raise ValueError(f"query vectors of padded width {qb.ent_vec.shape[1]}, index of {self.dp}")
        kn = self._kernels()
        qb = qb.to(self.device)
        return self._fold(qb.nq, topk, id_ranges, chunk,
                          lambda chunk: kn.ivf_workspace(qb.nq, qb.n_entries, chunk, self.cls is not None, topk, self.post_doc),
                          lambda *tail: self._search_range(kn, qb, *tail))

    def search(self, batch_cls, batch_embeddings, batch_weights, topk, id_ranges=None, chunk=None):
        tic = time.perf_counter()
        qb = pack_queries(batch_cls, batch_embeddings, batch_weights, d=self.d)
        self.latency["encode_time"] += time.perf_counter() - tic
        tic = time.perf_counter()
        out = self.search_packed(qb, topk, id_ranges=id_ranges, chunk=chunk)
        self.latency["search_time"] += time.perf_counter() - tic
        return out

    def quantize(self, dsub=4, codebook=None, **train_kwargs):
        """The IVFPQIndex of this index: posting rows replaced by 8-bit codes over sub-vectors of `dsub` features (DESIGN.md section
        10.2).  Trains a codebook on the index's own rows (train_pq(**train_kwargs)) unless one is given; the result shares
        post_doc, exp_off and the CLS rows with this index and keeps no reference to the dense rows."""
        kn = self._kernels()
        if codebook is None:
            codebook = train_pq(self.post_vec, dsub=dsub, kernels=kn, **train_kwargs)
        elif train_kwargs:
            raise TypeError(f"a codebook was given: nothing to train with {sorted(train_kwargs)}")
        codebook = _check_codebook(codebook, self.dp, dsub).to(self.device).contiguous()
        codes = kn.pq_encode(self.post_vec, codebook)
        return IVFPQIndex.from_packed(self.post_doc, codes, codebook, self.exp_off, self.cls, self.corpus_len, self.d, chunk=self.chunk,
                                      kernels=kn)


# ---- product-quantised postings -----------------------------------------------------------------------------

PQ_SUB_VEC_DIMS = (2, 4, 8)  # whole sub-vectors inside the 8 consecutive bf16 values of an MFMA fragment
PQ_MAX_DP = 64               # dprhot_ivf_pq_score keeps the codebook (dp * 512 bytes) in LDS next to its 32 KiB table


def _check_pq_shape(dp, dsub, max_dp=PQ_MAX_DP):
    if dsub not in PQ_SUB_VEC_DIMS:
        raise ValueError(f"sub_vec_dim={dsub}: one of {PQ_SUB_VEC_DIMS}")
    if dp > max_dp:
        raise NotImplementedError(f"product quantisation of rows of padded width {dp}: at most {max_dp}")


def _check_codebook(codebook, dp, dsub, max_dp=PQ_MAX_DP):
    _check_pq_shape(dp, dsub, max_dp)
    if codebook.dtype != _BF16 or tuple(codebook.shape) != (dp // int(dsub), 256, int(dsub)):
        raise ValueError(f"codebook {codebook.dtype} {tuple(codebook.shape)}; bf16 {(dp // int(dsub), 256, int(dsub))} expected")
    return codebook


def pq_decode(codes, codebook):
    """bf16 [n, m * dsub]: row p holds codebook[j, codes[p, j], :] for j = 0 .. m - 1.  codes uint8 [n, m], codebook [m, 256, dsub]
    (any dtype); plain indexing, on whatever device the tensors live."""
    m, _, dsub = codebook.shape
    if codes.dim() != 2 or codes.shape[1] != m or codes.dtype != torch.uint8:
        raise ValueError(f"codes {codes.dtype} {tuple(codes.shape)} for a codebook of {m} subspaces")
    cols = torch.arange(m, device=codes.device).unsqueeze(0)
    parts = [codebook[cols, codes[lo:lo + (1 << 22)].long()].reshape(-1, m * dsub) for lo in range(0, codes.shape[0], 1 << 22)]
    return torch.cat(parts, 0) if parts else codebook.new_zeros((0, m * dsub))


def train_pq(post_vec, dsub=4, iters=10, train_size=65536, seed=0, kernels=None, on_iteration=None, *, max_dp=PQ_MAX_DP, encode=None):
    """Codebook bf16 [dp / dsub, 256, dsub] for the bf16 rows post_vec [P, dp] on a HIP device: Lloyd's k-means per subspace on a
    seeded sample of `train_size` rows (all of them when there are no more; rows with a non-finite value are left out).
      init      per subspace 256 distinct sub-vectors of the sample (a seeded choice among the distinct ones in sorted order); with
                fewer than 256 distinct ones all of them, the remaining slots zeros
      assign    dprhot_pq_encode -- the rule the index is encoded with, on the bf16 centroids search will see
      update    fp32 sum of a centroid's sub-vectors in sample order by ONE owner (a stable sort by (subspace, code), then
                torch.segment_reduce: no floating-point atomics), divided by the count in fp32, rounded to bf16 after every
                iteration; an empty centroid keeps its value
    Same inputs and seed: torch.equal codebooks.  `on_iteration(i, codebook)` sees the codebook before the first (i = 0) and after
    every iteration.  `max_dp` and `encode(rows, codebook) -> codes` (default: kernels.pq_encode) are for an index whose kernels take
    wider rows through an encode entry of their own (colbert.train_pq)."""
    kn = _default_kernels(kernels)
    if post_vec.dtype != _BF16 or post_vec.dim() != 2:
        raise ValueError(f"rows {post_vec.dtype} {tuple(post_vec.shape)}; bf16 [P, dp] expected")
    P, dp = int(post_vec.shape[0]), int(post_vec.shape[1])
    dsub, dev = int(dsub), post_vec.device
    _check_pq_shape(dp, dsub, max_dp)
    encode = kn.pq_encode if encode is None else encode
    m = dp // dsub
    gen = torch.Generator().manual_seed(int(seed))
    if P > int(train_size):
        x = post_vec[torch.randperm(P, generator=gen)[: int(train_size)].sort().values.to(dev)]
    else:
        x = post_vec
    x = x[torch.isfinite(x.float()).all(1)].contiguous()
    ns = int(x.shape[0])
    sub = x.view(ns, m, dsub)
    codebook = torch.zeros((m, 256, dsub), dtype=_BF16, device=dev)
    for j in range(m):
        u = torch.unique(sub[:, j].float() + 0.0, dim=0)  # sorted rows; + 0.0: one zero, not two
        if u.shape[0] > 256:
            u = u[torch.randperm(u.shape[0], generator=gen)[:256].sort().values.to(dev)]
        codebook[j, : u.shape[0]] = u.to(_BF16)
    if on_iteration is not None:
        on_iteration(0, codebook.clone())
    base = (torch.arange(m, device=dev) * 256).unsqueeze(0)
    flat = sub.reshape(ns * m, dsub).float()
    for it in range(int(iters) if ns else 0):
        key = (encode(x, codebook).long() + base).reshape(-1)
        order = torch.sort(key, stable=True).indices  # sample order survives inside a centroid
        counts = torch.bincount(key, minlength=m * 256)
        sums = torch.segment_reduce(flat[order], "sum", lengths=counts, axis=0, unsafe=True)
        mean = (sums / counts.clamp(min=1).to(torch.float32).unsqueeze(1)).to(_BF16).view(m, 256, dsub)
        codebook = torch.where((counts > 0).view(m, 256, 1), mean, codebook)
        if on_iteration is not None:
            on_iteration(it + 1, codebook.clone())
    return codebook


class IVFPQIndex(IVFIndex):
    """IVFIndex with product-quantised postings: post_code uint8 [P, m] and ONE codebook bf16 [m, 256, dsub] instead of post_vec.
    `search` / `search_packed` return, bit for bit, what `decode()` -- the IVFIndex over the decoded rows -- returns."""

    def __init__(self, *args, **kwargs):
        raise TypeError("an IVFPQIndex comes from IVFIndex.quantize, IVFPQIndex.from_packed or load_pq_index")

    @classmethod
    def from_packed(cls, post_doc, post_code, codebook, exp_off, cls_rows, corpus_len, d, chunk=None, kernels=None):
        """From tensors in the device layout (csrc/ivf_pq.h), on their device: post_doc int32 [P] sorted by (expert, doc), post_code
        uint8 [P, m] in the same order, codebook bf16 [m, 256, dsub], exp_off int64 [V + 1], cls_rows as for IVFIndex.from_packed."""
        self = cls.__new__(cls)
        m, _, dsub = codebook.shape
        _check_codebook(codebook, m * dsub, dsub)
        assert post_code.dtype == torch.uint8
        assert post_code.shape == (post_doc.shape[0], m) and post_code.is_contiguous() and codebook.is_contiguous()
        self._set_frame(post_doc, exp_off, cls_rows, int(corpus_len), int(d), int(m * dsub), chunk, kernels)
        self.post_code, self.codebook, self.dsub = post_code, codebook, int(dsub)
        return self

    def _search_range(self, kn, qb, *tail):
        kn.ivf_pq_search(self, qb, *tail)

    def _tensors(self):
        return dict(post_doc=self.post_doc, post_code=self.post_code, codebook=self.codebook, exp_off=self.exp_off, cls=self.cls)

    @property
    def nbytes(self):
        """Bytes of device memory the index holds (codes, doc ids, offsets, codebook, CLS rows)."""
        return sum(t.numel() * t.element_size() for t in self._tensors().values() if t is not None)

    def decode(self):
        """The IVFIndex whose post_vec rows are pq_decode(post_code, codebook): the index this one searches, by definition."""
        return IVFIndex.from_packed(self.post_doc, pq_decode(self.post_code, self.codebook), self.exp_off, self.cls, self.corpus_len, self.d,
                                    chunk=self.chunk, kernels=self.kn)

    def quantize(self, *args, **kwargs):
        raise TypeError("the index is quantised already")

    def save(self, path):
        """One torch.save of the tensors (on the CPU) and sizes; load_pq_index reads it back."""
        blob = {k: (None if t is None else t.cpu()) for k, t in self._tensors().items()}
        blob.update(format="dpr_scale_amd.ivf_pq/1", corpus_len=self.corpus_len, d=self.d, dsub=self.dsub)
        torch.save(blob, path)
        return path


def load_pq_index(path, device=None, chunk=None, kernels=None):
    """The IVFPQIndex that IVFPQIndex.save wrote, placed on `device`."""
    device = torch.device(device) if device is not None else torch.device("cuda", 0)
    blob = torch.load(path, map_location="cpu", weights_only=True)
    if blob.get("format") != "dpr_scale_amd.ivf_pq/1":
        raise ValueError(f"{path}: not a product-quantised index file")
    mv = lambda t: None if t is None else t.contiguous().to(device)
    return IVFPQIndex.from_packed(mv(blob["post_doc"]), mv(blob["post_code"]), mv(blob["codebook"]), mv(blob["exp_off"]), mv(blob["cls"]),
                                  blob["corpus_len"], blob["d"], chunk=chunk, kernels=kernels)


def _quantized(index, quantizer, sub_vec_dim, train_kwargs):
    if quantizer in (None, "None"):
        if train_kwargs:
            raise TypeError(f"unexpected arguments {sorted(train_kwargs)}")
        return index
    if quantizer != "pq":
        raise NotImplementedError(f"quantizer={quantizer!r}: None or 'pq'")
    return index.quantize(dsub=sub_vec_dim, **train_kwargs)


def load_index(ctx_embeddings_dir, corpus_len, device=None, chunk=None, kernels=None, quantizer=None, sub_vec_dim=4, **train_kwargs):
    """Reads every `expert_*/{id}.pkl` and `cls_*.pkl` under `ctx_embeddings_dir`, merges the shard directories into ONE index (a
    doc's score is a sum over experts: shards are never searched one by one) and places it on `device`.

    Doc ids are the corpus ids the writer stored.  With CLS files they must equal the row numbers of the CLS files concatenated in rank
    order (rank r's ids inside rank r's rows, all rows together = corpus_len); an index for which that does not hold raises.

    quantizer="pq" (the reference's option; sub_vec_dim in {2, 4, 8}): the index is quantised on the device once it is built
    (IVFIndex.quantize; `train_kwargs` go to train_pq) and an IVFPQIndex comes back."""
    device = torch.device(device) if device is not None else torch.device("cuda", 0)
    experts, docs, vecs, cls = read_postings(ctx_embeddings_dir, int(corpus_len))
    return _quantized(IVFIndex(experts, docs, vecs, cls, corpus_len, device, chunk=chunk, kernels=kernels), quantizer, sub_vec_dim,
                      train_kwargs)


# ---- both sides from the encoders' repr tensors, on the device ----------------------------------------------------------------------

def query_dicts(queries_repr, n):
    """The query side of the reference's retrieval step (citadel_retrieval_task.py:104-125) on the host: per query a dict
    {expert_id: [weighted vector, ...]} and the same for the weights (fp32 for COIL, fp16 and zero weights dropped for CITADEL)."""
    coil = queries_repr["expert_ids"].dim() == 2
    # one transfer instead of one per token: the per-token work below is host work on small tensors
    reprs, ids, wts, att = (queries_repr[k].cpu() for k in ("expert_repr", "expert_ids", "expert_weights", "attention_mask"))
    batch_embeddings, batch_weights = [], []
    for b in range(n):
        embeddings, weights = collections.defaultdict(list), collections.defaultdict(list)
        for x, e, w, a in zip(reprs[b], ids[b], wts[b], att[b]):
            if a > 0:
                if coil:  # fp32 entries (:116-117)
                    embeddings[e.item()].append((w * x).to(torch.float32))
                    weights[e.item()].append(w.to(torch.float32))
                else:  # CITADEL: fp16 entries, zero weights dropped (:119-122)
                    for ek, wk in zip(e, w):
                        if wk > 0:
                            embeddings[ek.item()].append((wk * x).to(torch.float16))
                            weights[ek.item()].append(wk.to(torch.float16))
        batch_embeddings.append(embeddings)
        batch_weights.append(weights)
    return batch_embeddings, batch_weights


def _slots(repr_, n=None):
    """(expert_repr [n, L, d], expert_ids [n, L, K], expert_weights [n, L, K], attention_mask [n, L], coil) of a repr dict."""
    x, ids, w, att = (repr_[k].detach() for k in ("expert_repr", "expert_ids", "expert_weights", "attention_mask"))
    if n is not None:
        x, ids, w, att = x[:n], ids[:n], w[:n], att[:n]
    coil = ids.dim() == 2
    if coil:
        ids, w = ids.unsqueeze(-1), w.unsqueeze(-1)
    if ids.dim() != 3 or w.shape != ids.shape or x.shape[:2] != ids.shape[:2] or att.shape != ids.shape[:2]:
        raise ValueError(f"repr dict: expert_repr {tuple(x.shape)}, expert_ids {tuple(ids.shape)}, expert_weights {tuple(w.shape)}, "
                         f"attention_mask {tuple(att.shape)} do not belong together")
    return x, ids, w, att, coil


def query_entries(queries_repr, n=None, kernels=None):
    """The entries of a query batch as the reference's query writer lists them (citadel_eval_task.py:153-170), on the device of the
    repr tensors and in emission order (query, token, slot): (expert int32 [E], query row int32 [E], weight fp32 [E], vec fp32 [E, d])
    with vec = weight * expert_repr in expert_repr's dtype, widened.  COIL keeps every attended token, CITADEL every attended
    slot of weight > 0."""
    kn = _default_kernels(kernels)
    x, ids, w, att, coil = _slots(queries_repr, n)
    rows = torch.arange(ids.shape[0], dtype=torch.int32, device=ids.device)
    _, _, _, expert, row, slot, weight = kn.ivf_compact(ids, w, att, rows, not coil, 0.0)
    return expert, row, weight, kn.ivf_gather(x, w, slot, None, ids.shape[2], False, torch.float32, None)


def pack_queries_device(queries_repr, batch_cls, n=None, kernels=None):
    """What pack_queries(batch_cls, *query_dicts(queries_repr, n)).to(device) returns, tensor for tensor, built on the device of the
    repr tensors: the kept slots come from dprhot_ivf_compact in (query, token, slot) order, a stable sort by expert makes that
    (expert, query, listed order), and dprhot_ivf_gather writes the bf16 entries through the host path's roundings (product in the
    token rows' dtype; CITADEL: then fp16; then bf16)."""
    kn = _default_kernels(kernels)
    x, ids, w, att, coil = _slots(queries_repr, n)
    nq, d, dev = int(ids.shape[0]), int(x.shape[-1]), x.device
    if nq == 0:
        raise ValueError("empty query batch")
    rows = torch.arange(nq, dtype=torch.int32, device=dev)
    E, most, seq_off, expert, row, slot, _ = kn.ivf_compact(ids, w, att, rows, not coil, 0.0)
    if most > MAX_ENTRIES_PER_QUERY:
        q = int(torch.nonzero(seq_off[1:] - seq_off[:-1] > MAX_ENTRIES_PER_QUERY)[0])
        raise ValueError(f"query {q} has {int(seq_off[q + 1] - seq_off[q])} entries; at most {MAX_ENTRIES_PER_QUERY} are supported")
    dp = (d + 31) // 32 * 32
    if E:
        key, order = torch.sort(expert.long(), stable=True)  # stable: (query, token, slot) survives inside an expert
        ent_vec = kn.ivf_gather(x, w, slot, order.contiguous(), ids.shape[2], not coil, _BF16, dp)
        ent_q = row[order].contiguous()
        bexp, counts = torch.unique_consecutive(key, return_counts=True)
        boff = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)]).to(torch.int32)
        bexp = bexp.to(torch.int32)
    else:
        ent_vec = torch.zeros((0, dp), dtype=_BF16, device=dev)
        ent_q = torch.zeros(0, dtype=torch.int32, device=dev)
        bexp, boff = torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    cls = None
    if torch.is_tensor(batch_cls) and batch_cls.numel() > 0:
        if batch_cls.shape[0] != nq:
            raise ValueError("batch_cls and batch_embeddings differ in length")
        cls = _pad_cols(batch_cls.detach().to(dev, torch.float32), 8).to(_BF16).contiguous()
    return QueryBatch(nq, ent_vec, ent_q, bexp, boff, cls)


def postings_from_repr(contexts_repr, corpus_ids, weight_threshold=0.0, kernels=None):
    """The postings of one context batch as the reference's index writer lists them (citadel_eval_task.py:51-69), on the device of the
    repr tensors and in emission order (passage, token, slot): (expert int32 [P], doc int32 [P], weight fp32 [P], slot int32 [P],
    vec fp32 [P, d]) with vec = weight * expert_repr in expert_repr's dtype, widened.  COIL (2-D ids) keeps weights > 0,
    CITADEL weights > weight_threshold (strictly)."""
    kn = _default_kernels(kernels)
    x, ids, w, att, coil = _slots(contexts_repr)
    docs = torch.as_tensor(corpus_ids).to(x.device)
    thr = 0.0 if coil else float(weight_threshold)
    if w.is_floating_point():  # torch compares a tensor with a Python number in the tensor's dtype
        thr = float(torch.tensor(thr, dtype=torch.float64).to(w.dtype))
    _, _, _, expert, doc, slot, weight = kn.ivf_compact(ids, w, att, docs, True, thr)
    vec = kn.ivf_gather(x, w, slot, None, ids.shape[2], False, torch.float32, None)
    return expert, doc, weight, slot, vec


class IndexBuilder:
    """Collects the postings of context batches on the device and turns them into the reference's on-disk index (`write`) or straight
    into an IVFIndex (`finish`), which equals load_index of the tree `write` produces.  `corpus_len` is needed by `finish` only."""

    def __init__(self, corpus_len, device=None, kernels=None):
        self.corpus_len = None if corpus_len is None else int(corpus_len)
        self.device = None if device is None else torch.device(device)
        self.kn = kernels
        self.parts, self.cls_parts = [], []

    def add(self, contexts_repr, corpus_ids, weight_threshold=0.0, context_ids=None):
        """One context batch.  `context_ids` [B, L] (CITADEL only: the writer's add_context_id): every attended slot is kept whatever
        its weight and the third column of the files is the slot's token id instead of its vector."""
        self.kn = _default_kernels(self.kn)
        if context_ids is not None and contexts_repr["expert_ids"].dim() == 3:
            x, ids, w, att, _ = _slots(contexts_repr)
            docs = torch.as_tensor(corpus_ids).to(x.device)
            _, _, _, expert, doc, slot, weight = self.kn.ivf_compact(ids, w, att, docs, False, 0.0)
            tok = context_ids.detach().to(x.device)[:, : ids.shape[1]].reshape(-1)
            vec = tok[(slot // ids.shape[2]).long()].to(torch.float32)
        else:
            expert, doc, weight, slot, vec = postings_from_repr(contexts_repr, corpus_ids, weight_threshold, self.kn)
        self.parts.append((expert, doc, weight, vec))
        if "cls_repr" in contexts_repr:
            self.cls_parts.append(contexts_repr["cls_repr"].detach().to(torch.float32))
        return int(expert.shape[0])

    def _cat(self):
        if not self.parts:
            raise ValueError("no context batch was added")
        return tuple(torch.cat([p[i] for p in self.parts], 0) for i in range(4))

    def by_expert(self):
        """Host tensors of everything added, stably sorted by expert: (expert ids [V'], their posting counts [V'], doc int64 [P],
        weight fp32 [P], vec fp32 [P, d]) -- what `write` cuts into files."""
        expert, doc, weight, vec = self._cat()
        key, order = torch.sort(expert.long(), stable=True)
        ids, counts = torch.unique_consecutive(key, return_counts=True)
        return ids.cpu(), counts.cpu(), doc[order].long().cpu(), weight[order].cpu(), vec[order].cpu()

    def write(self, ctx_embeddings_dir, rank=0):
        """expert_{rank:04}/{id}.pkl = (ids int64, weights fp32, reprs fp32) in emission order per expert, cls_{rank:04}.pkl fp32 [docs,
        dc] when the batches carried cls_repr: the files of citadel_eval_task.py:75-117, pickle protocol 4."""
        ids, counts, doc, weight, vec = self.by_expert()
        if self.cls_parts:
            with open(os.path.join(ctx_embeddings_dir, f"cls_{rank:04}.pkl"), "wb") as f:
                pickle.dump(torch.cat(self.cls_parts, 0).cpu(), f, protocol=4)
        out_dir = os.path.join(ctx_embeddings_dir, f"expert_{rank:04}")
        os.makedirs(out_dir, exist_ok=True)
        lo = 0
        for e, c in zip(ids.tolist(), counts.tolist()):
            with open(os.path.join(out_dir, f"{e}.pkl"), "wb") as f:  # clones: a pickled view would carry the whole storage
                pickle.dump((doc[lo:lo + c].clone(), weight[lo:lo + c].clone(), vec[lo:lo + c].clone()), f, protocol=4)
            lo += c
        return ctx_embeddings_dir

    def finish(self, chunk=None, quantizer=None, sub_vec_dim=4, **train_kwargs):
        """The IVFIndex of everything added: postings stably sorted by (expert, doc), vectors rounded to bf16 and padded to a multiple
        of 32 columns by dprhot_ivf_gather, CLS rows with their zero tail.  quantizer="pq": its quantize(sub_vec_dim, **train_kwargs)."""
        if self.corpus_len is None or not 0 < self.corpus_len < 2 ** 31:
            raise ValueError(f"corpus_len={self.corpus_len} out of range (1 .. 2^31 - 1)")
        expert, doc, _, vec = self._cat()
        if vec.dim() != 2:
            raise ValueError("postings that carry token ids (add_context_id) make no index")
        P, d = int(vec.shape[0]), int(vec.shape[1])
        if P == 0:
            raise ValueError("no posting was added")
        lo_hi = torch.stack([doc.min(), doc.max(), expert.min(), expert.max()]).tolist()
        if lo_hi[0] < 0 or lo_hi[1] >= self.corpus_len or lo_hi[2] < 0:
            raise ValueError("doc ids must lie in [0, corpus_len) and expert ids must be non-negative")
        if lo_hi[3] >= 2 ** 31 - 1:
            raise ValueError("expert ids must fit int32")
        dev = vec.device
        order = torch.sort(expert.long() * self.corpus_len + doc.long(), stable=True).indices.contiguous()
        counts = torch.bincount(expert.long(), minlength=lo_hi[3] + 1)
        exp_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)]).contiguous()
        slot = torch.arange(P, dtype=torch.int32, device=dev)
        post_vec = self.kn.ivf_gather(vec, None, slot, order, 1, False, _BF16, (d + 31) // 32 * 32)
        post_doc = doc[order].to(torch.int32).contiguous()
        cls_rows = None
        if self.cls_parts:
            cls = torch.cat(self.cls_parts, 0)
            if cls.shape[0] != self.corpus_len:
                raise ValueError(f"{cls.shape[0]} CLS rows for {self.corpus_len} passages")
            c = _pad_cols(cls, 8).to(_BF16)
            cls_rows = torch.cat([c, torch.zeros((8, c.shape[1]), dtype=_BF16, device=dev)], 0).contiguous()
        out = [post_doc, post_vec, exp_off, cls_rows]
        if self.device is not None and self.device != dev:
            out = [None if t is None else t.to(self.device) for t in out]
        return _quantized(IVFIndex.from_packed(*out, self.corpus_len, d, chunk=chunk, kernels=self.kn), quantizer, sub_vec_dim, train_kwargs)
