"""Drop-in for dpr_scale.task.citadel_task.MultiVecRetrieverTask (reference: dpr_scale/task/citadel_task.py:8-391).

Same constructor kwargs (:9-24), same hooks and metric names.  The router loss comes from citadel_router.RouterScoring, the
expert (late-interaction) loss from multivec.ExpertScoring; both run on libdprhot.so.  The regularisers and the metric logging
stay plain torch, as in the reference.  The repr dicts this task consumes come from the encoders of dpr_scale_amd/models/
(citadel_model.CITADELEncoder, splade_model.SPLADEEncoder: the reference's kwargs, keys and shapes), whose head behind the MLM logits is
hotpath.router_head -- HIP kernels that keep no [B, T, V] tensor (csrc/router_head.h).
"""
import torch

from .citadel_router import RouterScoring, distributed_gather
from .dpr_task import DDPShardedStrategy, DDPStrategy, DenseRetrieverTask
from .multivec import ExpertScoring


class MultiVecRetrieverTask(RouterScoring, ExpertScoring, DenseRetrieverTask):
    def __init__(
        self,
        add_cls: bool = False,
        query_topk: int = 1,
        context_topk: int = 1,
        query_expert_load_loss_coef: float = 0,
        context_expert_load_loss_coef: float = 0,
        query_router_marg_load_loss_coef: float = 0,
        context_router_marg_load_loss_coef: float = 0,
        cross_batch: bool = True,
        in_batch: bool = True,
        query_pool: str = "sum",
        anneal_factor: float = 0.0,
        teacher_coef: float = 0.0,
        tau: float = 1.0,
        **kwargs,
    ):
        super().__init__(**kwargs)
        self.query_kwargs = dict(topk=query_topk, add_cls=add_cls)
        self.context_kwargs = dict(topk=context_topk, add_cls=add_cls)
        self.query_expert_load_loss_coef = query_expert_load_loss_coef
        self.context_expert_load_loss_coef = context_expert_load_loss_coef
        self.query_router_marg_load_loss_coef = query_router_marg_load_loss_coef
        self.context_router_marg_load_loss_coef = context_router_marg_load_loss_coef
        self.cross_batch = cross_batch
        self.in_batch = in_batch
        self.query_pool = query_pool
        self.epoch = 0
        self.anneal_factor = anneal_factor
        self.teacher_coef = teacher_coef
        self.tau = tau

    def anneal_func(self, loss):
        """:48-52."""
        coef = min(1, (self.epoch / self.trainer.max_epochs) ** self.anneal_factor)
        loss = coef * loss
        self.log("train_anneal_coef", coef)
        return loss

    def _encode_sequence(self, token_ids, encoder_model, **kwargs):
        return encoder_model(token_ids, **kwargs)

    def encode_queries(self, query_ids):
        return self._encode_sequence(query_ids, self.query_encoder, **self.query_kwargs)

    def encode_contexts(self, contexts_ids):
        return self._encode_sequence(contexts_ids, self.context_encoder, **self.context_kwargs)

    def distributed_gather(self, query_repr, context_repr, mask, pos_ctx_indices, teacher_scores):
        """:97-135 (ragged all-gather of the repr dicts, this rank's own tensors spliced in)."""
        return distributed_gather(query_repr, context_repr, mask, pos_ctx_indices, teacher_scores, self.global_rank)

    def _load_loss(self, coef, value, name):
        aux_loss = coef * value
        aux_loss = self.anneal_func(aux_loss) if self.anneal_factor else aux_loss
        self.log(name, aux_loss, prog_bar=True)
        return aux_loss

    def compute_loss(self, query_repr, context_repr, mask, pos_ctx_indices, teacher_scores):
        """:283-328."""
        loss = 0.0
        if "router_repr" in context_repr:
            loss += self.router_loss(query_repr, context_repr, mask, pos_ctx_indices, teacher_scores)
        if "expert_repr" in context_repr:
            loss += self.expert_loss(query_repr, context_repr, mask, pos_ctx_indices, teacher_scores)
        if self.query_router_marg_load_loss_coef > 0:
            marg = (query_repr["router_mask"].mean(0) * query_repr["router_softmax_repr"].mean(0)).sum()
            loss += self._load_loss(self.query_router_marg_load_loss_coef, marg, "train_query_router_marg_load_loss")
        if self.context_router_marg_load_loss_coef > 0:
            marg = (context_repr["router_mask"].mean(0) * context_repr["router_softmax_repr"].mean(0)).sum()
            loss += self._load_loss(self.context_router_marg_load_loss_coef, marg, "train_context_router_marg_load_loss")
        if self.context_expert_load_loss_coef > 0:
            loss += self._load_loss(self.context_expert_load_loss_coef, context_repr["expert_weights"].sum(1).sum(1).mean(0),
                                    "train_context_expert_load_loss")
        if self.query_expert_load_loss_coef > 0:
            loss += self._load_loss(self.query_expert_load_loss_coef, query_repr["expert_weights"].sum(1).sum(1).mean(0),
                                    "train_query_expert_load_loss")
        for side, repr_ in (("context", context_repr), ("query", query_repr)):
            for kind in ("cond", "marg"):
                if f"avg_{kind}_num_experts" in repr_:
                    self.log(f"train_avg_{side}_{kind}_num_experts", repr_[f"avg_{kind}_num_experts"].mean(), prog_bar=True)
        return loss

    def training_step(self, batch, batch_idx):
        """:330-344."""
        mask = batch["ctx_mask"]
        pos_ctx_indices = batch["pos_ctx_indices"]
        teacher_scores = batch["scores"]
        query_repr, context_repr = self(batch["query_ids"], batch["contexts_ids"])
        if self.cross_batch and isinstance(self.trainer.strategy, (DDPStrategy, DDPShardedStrategy)):
            query_repr, context_repr, mask, pos_ctx_indices, teacher_scores = self.distributed_gather(
                query_repr, context_repr, mask, pos_ctx_indices, teacher_scores)
        return self.compute_loss(query_repr, context_repr, mask, pos_ctx_indices, teacher_scores)

    def _eval_step(self, batch, batch_idx):
        """:346-365."""
        pos_ctx_indices = batch["pos_ctx_indices"]
        mask = batch["ctx_mask"]
        query_repr, contexts_repr = self(batch["query_ids"], batch["contexts_ids"])
        pred_context_scores = self.expert_sim_score(query_repr, contexts_repr, mask)
        if "cls_repr" in query_repr:
            pred_context_scores += self.sim_score(query_repr["cls_repr"], contexts_repr["cls_repr"], mask)
        loss = self.loss(pred_context_scores, pos_ctx_indices)
        return (self.compute_rank_metrics(pred_context_scores, pos_ctx_indices), query_repr, contexts_repr, pos_ctx_indices, mask,
                loss)

    def _eval_epoch_end(self, outputs, log_prefix="valid"):
        """:367-391."""
        self.epoch += 1
        total_avg_rank, total_ctx_count, total_count, total_mrr, total_loss, total_score = 0, 0, 0, 0, 0, 0
        for metrics, query_repr, contexts_repr, _, mask, loss in outputs:
            rank, mrr, score = metrics
            total_avg_rank += rank
            total_mrr += mrr
            total_score += score
            total_ctx_count += contexts_repr["expert_repr"].size(0) - torch.sum(mask)
            total_count += query_repr["expert_repr"].size(0)
            total_loss += loss
        total_ctx_count = total_ctx_count / len(outputs)
        total_loss = total_loss / len(outputs)
        metrics = {
            log_prefix + "_avg_rank": total_avg_rank / total_count,
            log_prefix + "_mrr": total_mrr / total_count,
            log_prefix + f"_accuracy@{self.k}": total_score / total_count,
            log_prefix + "_ctx_count": total_ctx_count,
            log_prefix + "_expert_loss": total_loss,
        }
        self.log_dict(metrics, on_epoch=True, sync_dist=True)
