"""End-to-end retrieval tasks for ColBERT.  The reference has none: its index writer keys every posting by
`expert_ids`, which a ColBERT encoder does not produce.  These two are the ColBERT counterparts of task/citadel_eval.py's index writer
and task/citadel_retrieval.py's retrieval task over dpr_scale_amd.colbert -- a packed token index searched exhaustively by
libdprhot.so (dprhot_colbert_search), with the score of training and reranking (hotpath.expert_sim_score on a ColBERT repr dict).

GenerateColBERTEmbeddingsTask   the constructor kwargs, hooks and barrier of GenerateMultiVecEmbeddingsTask; writes
                                `tokens_{rank:04}.pkl` = (ids int64, lengths int32, reprs bfloat16), the attended tokens of every passage.
                                `add_context_id` and `weight_threshold` are accepted and have no meaning without experts.
ColBERTRetrievalTask            CITADELRetrievalTask's constructor, refusals, merge_trec_results / merge_qa_results and output files;
                                the index is colbert.load_index and a query batch is searched as the dense [B, LQ, d] block the
                                encoder returns (padded query tokens are zero rows), with `query_pool` and `topk`.
`kernels` (default: the HIP kernels) is the kernel object colbert.py takes.
"""
import os
import pathlib
import time

import torch

from .. import colbert
from .citadel_eval import _barrier
from .citadel_retrieval import CITADELRetrievalTask
from .citadel_task import MultiVecRetrieverTask


class GenerateColBERTEmbeddingsTask(MultiVecRetrieverTask):
    kernels = None  # what dpr_scale_amd.colbert takes as `kernels` (None: hotpath.default_kernels())

    def __init__(self, ctx_embeddings_dir, checkpoint_path, add_context_id, weight_threshold=0.0, **kwargs):
        super().__init__(**kwargs)
        self.ctx_embeddings_dir = ctx_embeddings_dir
        self.checkpoint_path = checkpoint_path
        self.add_context_id = add_context_id
        self.weight_threshold = weight_threshold
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
        if "expert_ids" in contexts_repr:
            raise NotImplementedError("an encoder with expert_ids (COIL / CITADEL) is indexed by GenerateMultiVecEmbeddingsTask")
        if self.builder is None:
            self.builder = colbert.TokenIndexBuilder(None, kernels=self.kernels)
        corpus_ids = torch.tensor([int(c) for c in batch["corpus_ids"]], dtype=torch.int64)
        return self.builder.add(contexts_repr, contexts_ids["attention_mask"][:, 1:], corpus_ids)

    def test_step(self, batch, batch_idx):
        return self._eval_step(batch, batch_idx)

    def test_epoch_end(self, contexts_reprs):
        if not self.ctx_embeddings_dir:
            self.ctx_embeddings_dir = self.trainer.weights_save_path
        if self.builder is not None:
            print(f"\nWriting tensors to {os.path.join(self.ctx_embeddings_dir, f'tokens_{self.global_rank:04}.pkl')}")
            self.builder.write(self.ctx_embeddings_dir, self.global_rank)
            self.builder = None
        _barrier()


class ColBERTRetrievalTask(CITADELRetrievalTask):
    kernels = None

    def _load_index(self, device):
        return colbert.load_index(self.ctx_embeddings_dir, len(self.ctxs), device, kernels=self.kernels)

    def _eval_step(self, batch, batch_idx):
        tic = time.perf_counter()
        query_ids = batch["query_ids"]
        topic_ids = batch["topic_ids"] if "topic_ids" in batch else []
        answers = batch["answers"] if "answers" in batch else []
        questions = batch["question"] if "question" in batch else []
        queries_repr = {k: v.detach() for k, v in self(query_ids).items()}
        if "expert_ids" in queries_repr:
            raise NotImplementedError("an encoder with expert_ids (COIL / CITADEL) is searched by CITADELRetrievalTask")
        n = len(topic_ids) if len(topic_ids) > 0 else len(query_ids["input_ids"])
        self.latency["encode_time"] += time.perf_counter() - tic
        batch_top_scores, batch_top_ids = self.index.search(queries_repr["expert_repr"][:n], self.topk, query_pool=self.query_pool)
        return batch_top_scores.cpu().tolist(), batch_top_ids.cpu().tolist(), topic_ids, questions, answers
