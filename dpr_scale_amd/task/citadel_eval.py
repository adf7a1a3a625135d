"""Drop-ins for dpr_scale.task.citadel_eval_task.GenerateMultiVecEmbeddingsTask and GenerateMultiVecQueryEmbeddingsTask (reference:
dpr_scale/task/citadel_eval_task.py:16-213): the index writer and the query-embedding writer of CITADEL / COIL.

Same constructor kwargs and defaults, same hooks, same files: `expert_{rank:04}/{expert_id}.pkl` = (ids int64, weights fp32, reprs
fp32) and `cls_{rank:04}.pkl` for the index (what dpr_scale_amd.ivf.load_index reads); `query_id.pkl`, `query_repr.pkl`,
`query_weight.pkl` and `query_cls.pkl` for the queries.  The reference walks every token slot in Python, one `.item()` each; here the
kept slots are listed and their weighted vectors written by libdprhot.so (dprhot_ivf_compact / dprhot_ivf_gather through
dpr_scale_amd.ivf), in the reference's order and with its roundings, and only finished arrays reach the host.  `self.kernels` (default:
the HIP kernels) is the kernel object ivf.py takes.

Scope: ColBERT (encoders without `expert_ids`) is not covered here: task/colbert_retrieval.py holds its writer and retrieval task.  RerankMultiVecRetrieverTask of the same reference file: task/rerank.py.
"""
import collections
import os
import pathlib
import pickle

import torch

from .. import ivf
from .citadel_task import MultiVecRetrieverTask


def _barrier():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()  # make sure rank 0 waits for all to complete


class GenerateMultiVecEmbeddingsTask(MultiVecRetrieverTask):
    kernels = None  # what dpr_scale_amd.ivf takes as `kernels` (None: hotpath.default_kernels())

    def __init__(self, ctx_embeddings_dir, checkpoint_path, add_context_id, weight_threshold=0.0, **kwargs):
        super().__init__(**kwargs)
        self.ctx_embeddings_dir = ctx_embeddings_dir
        self.checkpoint_path = checkpoint_path
        self.add_context_id = add_context_id  # for token/expert distribution analysis
        self.weight_threshold = weight_threshold  # for on-the-fly pruning
        self.builder = None
        pathlib.Path(ctx_embeddings_dir).mkdir(parents=True, exist_ok=True)

    def setup(self, stage: str):
        super().setup("train")
        print(f"Loading checkpoint from {self.checkpoint_path}")
        checkpoint = torch.load(self.checkpoint_path, map_location="cpu", weights_only=False)
        self.load_state_dict(checkpoint["state_dict"])

    def forward(self, contexts_ids):
        return self.encode_contexts(contexts_ids)

    def _eval_step(self, batch, batch_idx):
        contexts_ids = batch["contexts_ids"]
        contexts_repr = {k: v.detach() for k, v in self(contexts_ids).items()}
        if "expert_ids" not in contexts_repr:
            raise NotImplementedError("ColBERT (an encoder without expert_ids) is not covered by the index writer: "
                                      "task/colbert_retrieval.py GenerateColBERTEmbeddingsTask writes its token index")
        if self.builder is None:
            self.builder = ivf.IndexBuilder(None, kernels=self.kernels)
        corpus_ids = torch.tensor([int(c) for c in batch["corpus_ids"]], dtype=torch.int64)
        tokens = contexts_ids["input_ids"][:, 1:] if self.add_context_id else None
        return self.builder.add(contexts_repr, corpus_ids, self.weight_threshold, context_ids=tokens)

    def test_step(self, batch, batch_idx):
        return self._eval_step(batch, batch_idx)

    def _index_file(self):
        """What `builder.write` leaves under ctx_embeddings_dir for this rank."""
        return f"expert_{self.global_rank:04}"

    def test_epoch_end(self, contexts_reprs):
        if not self.ctx_embeddings_dir:
            self.ctx_embeddings_dir = self.trainer.weights_save_path
        if self.builder is not None:
            print(f"\nWriting tensors to {os.path.join(self.ctx_embeddings_dir, self._index_file())}")
            self.builder.write(self.ctx_embeddings_dir, self.global_rank)
            self.builder = None
        _barrier()


class GenerateMultiVecQueryEmbeddingsTask(GenerateMultiVecEmbeddingsTask):
    def __init__(
        self,
        hnsw_index=False,
        output_path="/tmp/results.jsonl",
        query_emb_output_dir=None,
        passages="",
        **kwargs,
    ):
        super().__init__(**kwargs)
        self.hnsw_index = hnsw_index
        self.output_path = output_path
        self.query_emb_output_dir = query_emb_output_dir

    def forward(self, query_ids):
        return self.encode_queries(query_ids)

    def _eval_step(self, batch, batch_idx):
        query_ids = batch["query_ids"]
        topic_ids = batch["topic_ids"]  # add question topic id
        queries_repr = {k: v.detach() for k, v in self(query_ids).items()}
        if "expert_ids" not in queries_repr:
            raise NotImplementedError("ColBERT (an encoder without expert_ids) is not covered by the query writer: "
                                      "task/colbert_retrieval.py ColBERTRetrievalTask searches its queries as they leave the encoder")
        batch_cls = queries_repr["cls_repr"].cpu() if "cls_repr" in queries_repr else []
        n = len(topic_ids)
        expert, row, weight, vec = (t.cpu() for t in ivf.query_entries(queries_repr, n, kernels=self.kernels))
        batch_embeddings = [collections.defaultdict(list) for _ in range(n)]
        batch_weights = [collections.defaultdict(list) for _ in range(n)]
        # finished fp32 arrays on the host: the clones keep every pickled tensor from carrying the whole batch's storage
        for e, q, w, v in zip(expert.tolist(), row.tolist(), weight, vec):
            batch_embeddings[q][e].append(v.clone())
            batch_weights[q][e].append(w.clone())
        return batch_embeddings, batch_weights, topic_ids, batch_cls

    def test_step(self, batch, batch_idx):
        return self._eval_step(batch, batch_idx)

    def test_epoch_end(self, queries_reprs):
        embeddings, weights, topic_ids, cls_embeddings = [], [], [], []
        for batch_queries_repr, batch_weights, batch_topic_ids, batch_cls in queries_reprs:
            if len(batch_cls) > 0:
                cls_embeddings.append(batch_cls)
            embeddings.extend(batch_queries_repr)
            weights.extend(batch_weights)
            topic_ids.extend(batch_topic_ids)
        pathlib.Path(self.query_emb_output_dir).mkdir(parents=True, exist_ok=True)
        files = [("query_id.pkl", topic_ids), ("query_repr.pkl", embeddings), ("query_weight.pkl", weights)]
        if len(cls_embeddings) > 0:
            files.append(("query_cls.pkl", torch.cat(cls_embeddings, 0)))
        for name, obj in files:
            path = os.path.join(self.query_emb_output_dir, name)
            print(f"\nWriting tensors to {path}")
            with open(path, "wb") as f:
                pickle.dump(obj, f, protocol=4)
