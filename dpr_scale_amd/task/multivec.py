"""CITADEL / ColBERT / COIL expert loss on the MI355X hot path: the late-interaction half of dpr_scale/task/citadel_task.py.

  citadel_task.py:155-238  colbert_score / coil_score / citadel_score / expert_sim_score  -> ExpertScoring.expert_sim_score
  citadel_task.py:264-281  expert_loss                                                  -> ExpertScoring.expert_loss

The reference materialises the token-level score tensor [Nq, LQ*KQ, Nc, LD*KD] before it takes max and sum; here one HIP launch
keeps only a running max / argmax per query slot (hotpath.expert_sim_score, csrc/maxsim.h) and the backward works from the argmax.
`ExpertScoring` is a mix-in next to citadel_router.RouterScoring; task/citadel_task.py combines both into the drop-in task.
"""
import torch

from .. import hotpath
from .citadel_router import distilled_loss


class ExpertScoring:
    """Mix-in: expects `self.loss`, `self.kernels`, `self.in_batch`, `self.query_pool`, `self.teacher_coef`, `self.tau`, `self.log`
    and `self.sim_score` (RouterScoring's) as the reference's MultiVecRetrieverTask has them."""

    def expert_sim_score(self, query_repr, context_repr, mask=None, pairwise=False):
        """citadel_task.py:215-238: [Nq, Nc] (or [B, M] pairwise), masked contexts -inf; differentiable in the token vectors and,
        for CITADEL, in the expert weights."""
        return hotpath.expert_sim_score(query_repr, context_repr, mask, pairwise, getattr(self, "query_pool", "sum"),
                                        getattr(self, "kernels", None))

    def expert_loss(self, query_repr, context_repr, mask, pos_ctx_indices, teacher_scores):
        """citadel_task.py:264-281."""
        expert_loss = 0.0
        if 1 - self.teacher_coef > 0:
            expert_scores = 0.0
            if "cls_repr" in context_repr:
                expert_scores += self.sim_score(query_repr["cls_repr"], context_repr["cls_repr"], mask)
            expert_scores += self.expert_sim_score(query_repr, context_repr, mask, pairwise=not self.in_batch)
            if not self.in_batch:
                pos_ctx_indices = torch.zeros(len(expert_scores), dtype=torch.int64, device=expert_scores.device)
            expert_loss = self.loss(expert_scores, pos_ctx_indices)
        if self.teacher_coef > 0:
            pairwise_expert_scores = self.expert_sim_score(query_repr, context_repr, mask, pairwise=True)
            expert_loss = (1 - self.teacher_coef) * expert_loss + self.teacher_coef * distilled_loss(
                pairwise_expert_scores / self.tau, teacher_scores / self.tau)
        self.log("train_expert_loss", expert_loss, prog_bar=True)
        return expert_loss
