"""Drop-ins for the reference's two rerank tasks: dpr_scale.task.citadel_eval_task.RerankMultiVecRetrieverTask
(dpr_scale/task/citadel_eval_task.py:215-313, conf/task/multivec_rerank.yaml) and dpr_scale.task.dpr_rerank_task.RerankDenseRetrieverTask
(dpr_scale/task/dpr_rerank_task.py, conf/task/dpr_rerank.yaml) -- the stage between retrieval and the metric scripts.

Same constructor kwargs, same hooks, same files: `scores_{rank:04}.pkl` (one fp32 tensor), `qids_{rank:04}.pkl` and
`ctx_ids_{rank:04}.pkl` (lists), pickle protocol 4.  A rerank batch is B aligned (query, passage) pairs.  The multi-vector score is
hotpath.rerank_score: the pairwise MaxSim of ColBERT / COIL / CITADEL from one score-only launch that keeps no tables
(csrc/maxsim.h ms_score_kernel), plus the CLS dot product when the encoders return `cls_repr`; the dense score
is hotpath.pairwise_score.  `self.kernels` (default: the HIP kernels) is the kernel object both take.

Scope: the cross-encoder rerank task and the rerank datamodule (the reference's DenseRetrieverRerankDataModule is used as is) are not
covered.
"""
import os
import pickle

import torch

from .. import hotpath
from .citadel_eval import _barrier
from .citadel_task import MultiVecRetrieverTask
from .dpr_task import DenseRetrieverTask


class _RerankTask:
    """What the two tasks share: the checkpoint, the batch plumbing and the three output files."""

    def __init__(self, checkpoint_path, output_dir, **kwargs):
        super().__init__(**kwargs)
        self.checkpoint_path = checkpoint_path
        self.output_dir = output_dir
        os.makedirs(output_dir, exist_ok=True)

    def setup(self, stage: str):
        super().setup("train")
        print(f"Loading checkpoint from {self.checkpoint_path}")
        checkpoint = torch.load(self.checkpoint_path, map_location="cpu", weights_only=False)
        self.load_state_dict(checkpoint["state_dict"])

    def forward(self, query_ids, ctx_ids):
        return self.encode_queries(query_ids), self.encode_contexts(ctx_ids)

    def _pair_scores(self, q_repr, ctx_repr):
        raise NotImplementedError

    def _eval_step(self, batch, batch_idx):
        q_repr, ctx_repr = self(batch["query_ids"], batch["contexts_ids"])
        scores = self._pair_scores(q_repr, ctx_repr)
        return [batch["qid"], batch["ctx_id"], scores.cpu()]

    def test_step(self, batch, batch_idx):
        return self._eval_step(batch, batch_idx)

    def test_epoch_end(self, test_outputs):
        qids, ctx_ids, scores = [], [], []
        for b_qids, b_ctx_ids, b_scores in test_outputs:
            qids.extend(b_qids)
            ctx_ids.extend(b_ctx_ids)
            scores.append(b_scores)
        scores = torch.cat(scores, dim=0)
        print(f"\nWriting scores to {os.path.join(self.output_dir, f'scores_{self.global_rank:04}.pkl')}")
        for name, obj in (("scores", scores), ("qids", qids), ("ctx_ids", ctx_ids)):
            with open(os.path.join(self.output_dir, f"{name}_{self.global_rank:04}.pkl"), "wb") as f:
                pickle.dump(obj, f, protocol=4)
        _barrier()


class RerankMultiVecRetrieverTask(_RerankTask, MultiVecRetrieverTask):
    def __init__(self, checkpoint_path, output_dir, **kwargs):
        super().__init__(checkpoint_path, output_dir, **kwargs)

    def _pair_scores(self, q_repr, ctx_repr):
        q_repr = {k: v.detach() for k, v in q_repr.items()}
        ctx_repr = {k: v.detach() for k, v in ctx_repr.items()}
        return hotpath.rerank_score(q_repr, ctx_repr, self.query_pool, self.kernels)


class RerankDenseRetrieverTask(_RerankTask, DenseRetrieverTask):
    def __init__(self, checkpoint_path, output_dir, **kwargs):
        super().__init__(checkpoint_path, output_dir, **kwargs)

    def _pair_scores(self, q_repr, ctx_repr):
        return hotpath.pairwise_score(q_repr.detach(), ctx_repr.detach(), None, self.kernels)[:, 0]
