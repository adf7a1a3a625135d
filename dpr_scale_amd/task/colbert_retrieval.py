"""End-to-end retrieval tasks for ColBERT.  The reference has none: its index writer keys every posting by
`expert_ids`, which a ColBERT encoder does not produce.  These two are the ColBERT counterparts of task/citadel_eval.py's index writer
and task/citadel_retrieval.py's retrieval task over dpr_scale_amd.colbert -- a packed token index searched exhaustively by
libdprhot.so (dprhot_colbert_search), with the score of training and reranking (hotpath.expert_sim_score on a ColBERT repr dict).

GenerateColBERTEmbeddingsTask   GenerateMultiVecEmbeddingsTask (its constructor kwargs, hooks and barrier) with its own step; writes
                                `tokens_{rank:04}.pkl` = (ids int64, lengths int32, reprs bfloat16), the attended tokens of every passage.
                                `add_context_id` and `weight_threshold` are accepted and have no meaning without experts.
ColBERTRetrievalTask            CITADELRetrievalTask's constructor, refusals, merge_trec_results / merge_qa_results and output files;
                                the index is colbert.load_index and a query batch is searched as the dense [B, LQ, d] block the
                                encoder returns (padded query tokens are zero rows), with `query_pool` and `topk`.
ColBERTPQRetrievalTask          ColBERTRetrievalTask over a product-quantised token index (colbert.ColBERTPQIndex, DESIGN.md section
                                12.1): the same kwargs plus `sub_vec_dim` (8) and `save_quantized` (False).
ColBERTPrunedRetrievalTask      ColBERTRetrievalTask with centroid pruning: the same kwargs plus `nprobe` and
                                `n_centroids`; with both set the index gets centroids and queries go through search_pruned, with
                                `ndocs` (None: every candidate is scored exactly) as its centroid-interaction stage (section 12.3).
                                The three are class attributes of ColBERTRetrievalTask (None: exhaustive), whose constructor stays
                                CITADELRetrievalTask's.  Over a product-quantised index pruning is refused (dense rows only).
ColBERTResidualRetrievalTask    ColBERTRetrievalTask over a residual-compressed token index (colbert.ColBERTResidualIndex, DESIGN.md
                                section 12.4), always with centroid pruning: the same kwargs plus `nbits` (2), `nprobe` and
                                `n_centroids` (both required), `ndocs` and `save_compressed` (False).
`kernels` (default: the HIP kernels) is the kernel object colbert.py takes.
"""
import os
import time

import torch

from .. import colbert, ivf
from .citadel_eval import GenerateMultiVecEmbeddingsTask
from .citadel_retrieval import CITADELRetrievalTask


class GenerateColBERTEmbeddingsTask(GenerateMultiVecEmbeddingsTask):
    def _eval_step(self, batch, batch_idx):
        contexts_ids = batch["contexts_ids"]
        contexts_repr = {k: v.detach() for k, v in self(contexts_ids).items()}
        if "expert_ids" in contexts_repr:
            raise NotImplementedError("an encoder with expert_ids (COIL / CITADEL) is indexed by GenerateMultiVecEmbeddingsTask")
        if self.builder is None:
            self.builder = colbert.TokenIndexBuilder(None, kernels=self.kernels)
        corpus_ids = torch.tensor([int(c) for c in batch["corpus_ids"]], dtype=torch.int64)
        return self.builder.add(contexts_repr, contexts_ids["attention_mask"][:, 1:], corpus_ids)

    def _index_file(self):
        return f"tokens_{self.global_rank:04}.pkl"


class ColBERTRetrievalTask(CITADELRetrievalTask):
    kernels = None
    # centroid pruning: with BOTH set, `setup` gives the index centroids -- `centroids.pkl` beside the token
    # files when present (ColBERTIndex.load_centroids), else build_centroids(n_centroids) -- and the task retrieves with search_pruned;
    # with either None it is the exhaustive task.  The constructor is CITADELRetrievalTask's: ColBERTPrunedRetrievalTask takes the two
    # as keyword arguments.
    nprobe = None
    n_centroids = None
    ndocs = None  # with pruning on: search_pruned keeps the best ndocs candidates per query by approximate score
    CENTROID_FILE = "centroids.pkl"

    def _pruned(self):
        return self.nprobe is not None and self.n_centroids is not None

    def _load_index(self, device):
        index = colbert.load_index(self.ctx_embeddings_dir, len(self.ctxs), device, kernels=self.kernels)
        if self._pruned():
            path = os.path.join(self.ctx_embeddings_dir, self.CENTROID_FILE)
            if os.path.exists(path):
                index.load_centroids(path)
            else:
                index.build_centroids(int(self.n_centroids))
        return index

    def _search(self, queries_repr, n, tic):
        if "expert_ids" in queries_repr:
            raise NotImplementedError("an encoder with expert_ids (COIL / CITADEL) is searched by CITADELRetrievalTask")
        self.latency["encode_time"] += time.perf_counter() - tic
        if self._pruned():
            stage = {} if self.ndocs is None else dict(ndocs=int(self.ndocs))
            return self.index.search_pruned(queries_repr["expert_repr"][:n], self.topk, int(self.nprobe), query_pool=self.query_pool, **stage)
        return self.index.search(queries_repr["expert_repr"][:n], self.topk, query_pool=self.query_pool)


class ColBERTPrunedRetrievalTask(ColBERTRetrievalTask):
    """ColBERTRetrievalTask with `nprobe`, `n_centroids` and `ndocs` as constructor kwargs (the first two None: the exhaustive task)."""

    def __init__(self, *args, nprobe=None, n_centroids=None, ndocs=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.nprobe, self.n_centroids, self.ndocs = nprobe, n_centroids, ndocs


class ColBERTPQRetrievalTask(ColBERTRetrievalTask):
    """ColBERTRetrievalTask over 8-bit codes of sub-vectors of `sub_vec_dim` in {2, 4, 8} features.  `setup` loads
    `ctx_embeddings_dir/colbert_pq.pt` when that file exists (colbert.load_pq_index); otherwise it trains a codebook on a sample of
    the token files and encodes them one at a time (colbert.load_index(..., quantizer="pq")) -- the dense index is never built -- and
    writes the file when `save_quantized` is set, so that a large index is not retrained at every start."""

    PQ_FILE = "colbert_pq.pt"

    def __init__(self, *args, quantizer="pq", sub_vec_dim=8, save_quantized=False, **kwargs):
        if quantizer != "pq":
            raise NotImplementedError(f'quantizer={quantizer!r}: ColBERTPQRetrievalTask is the quantizer="pq" task '
                                      f"(ColBERTRetrievalTask takes the plain index)")
        if sub_vec_dim not in ivf.PQ_SUB_VEC_DIMS:
            raise NotImplementedError(f"sub_vec_dim={sub_vec_dim}: sub-vectors of {ivf.PQ_SUB_VEC_DIMS} features")
        super().__init__(*args, quantizer=None, sub_vec_dim=sub_vec_dim, **kwargs)  # refuses what the plain task refuses
        self.quantizer = "pq"
        self.save_quantized = bool(save_quantized)

    def _load_index(self, device):
        path = os.path.join(self.ctx_embeddings_dir, self.PQ_FILE)
        if os.path.exists(path):
            index = colbert.load_pq_index(path, device, kernels=self.kernels)
            if index.corpus_len != len(self.ctxs) or index.dsub != self.sub_vec_dim:
                raise ValueError(f"{path}: an index of {index.corpus_len} passages with sub_vec_dim={index.dsub}; "
                                 f"{len(self.ctxs)} passages and sub_vec_dim={self.sub_vec_dim} were asked for")
            return index
        index = colbert.load_index(self.ctx_embeddings_dir, len(self.ctxs), device, kernels=self.kernels, quantizer="pq",
                                   sub_vec_dim=self.sub_vec_dim)
        if self.save_quantized:
            index.save(path)
        return index


class ColBERTResidualRetrievalTask(ColBERTRetrievalTask):
    """ColBERTRetrievalTask over centroid ids plus `nbits` in {1, 2, 4} bits per feature of the residual, searched with search_pruned
    (`nprobe`, `ndocs`).  `setup` loads `ctx_embeddings_dir/colbert_res.pt` when that file exists (colbert.load_residual_index);
    otherwise it trains `n_centroids` centroids and the buckets on a sample of the token files and encodes them one at a time
    (colbert.load_index(..., quantizer="residual")) -- the dense index is never built -- and writes the file when `save_compressed`
    is set, so that a large index is not retrained at every start."""

    RES_FILE = "colbert_res.pt"

    def __init__(self, *args, nbits=2, nprobe=None, n_centroids=None, ndocs=None, save_compressed=False, **kwargs):
        if nbits not in colbert.RES_NBITS:
            raise NotImplementedError(f"nbits={nbits}: {colbert.RES_NBITS} bits per feature")
        if nprobe is None or n_centroids is None:
            raise ValueError("the residual index is searched with centroid pruning only: nprobe and n_centroids are required")
        super().__init__(*args, **kwargs)  # refuses what the plain task refuses
        self.nbits, self.nprobe, self.n_centroids, self.ndocs = int(nbits), nprobe, n_centroids, ndocs
        self.save_compressed = bool(save_compressed)

    def _load_index(self, device):
        path = os.path.join(self.ctx_embeddings_dir, self.RES_FILE)
        if os.path.exists(path):
            index = colbert.load_residual_index(path, device, kernels=self.kernels)
            if index.corpus_len != len(self.ctxs) or index.nbits != self.nbits:
                raise ValueError(f"{path}: an index of {index.corpus_len} passages with nbits={index.nbits}; "
                                 f"{len(self.ctxs)} passages and nbits={self.nbits} were asked for")
            return index
        index = colbert.load_index(self.ctx_embeddings_dir, len(self.ctxs), device, kernels=self.kernels, quantizer="residual",
                                   nbits=self.nbits, n_centroids=int(self.n_centroids))
        if self.save_compressed:
            index.save(path)
        return index
