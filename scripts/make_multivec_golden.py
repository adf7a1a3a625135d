#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/multivec_*.npz from the reference's own citadel_task.py.

Run where the reference tree is present:   python scripts/make_multivec_golden.py
Every expected number below comes from the reference's MultiVecRetrieverTask, imported unmodified through
oracle.ref_shim.make_reference_citadel_task (fp32, CPU); only `query_pool` (and, for the step case, the regulariser
coefficients) are set on the instance.  Inputs come from tests/_multivec_oracle.make_inputs (grid values: every score is exact in
fp32) and are stored in the fixture as well, so the tests never regenerate them.

Cases
  multivec_{colbert,coil,citadel11,citadel23}_{inbatch,pairwise}_{sum,max}
        expert_sim_score (:215-238) with a masked context, the argmax of the token tensor (the reference's own colbert_score /
        coil_score / citadel_score, then .max(-1)), and expert_loss (:264-281) with the gradient into every expert_repr /
        expert_weights leaf.  citadel11: KQ = KD = 1; citadel23: KQ = 2, KD = 3.
  multivec_teacher   expert_loss with teacher_coef = 0.5, tau = 2 (distilled_loss on the pairwise scores, :240-247)
  multivec_step      training_step (:330-344 -> compute_loss :283-328) with the two expert-load regularisers and distillation:
                     loss, gradients, logged metric names
  multivec_eval      _eval_step (:346-365) + _eval_epoch_end (:367-391): rank metrics, loss, logged metrics
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402
import _multivec_oracle as MO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
KINDS = {"colbert": ("colbert", 1, 1), "coil": ("coil", 1, 1), "citadel11": ("citadel", 1, 1), "citadel23": ("citadel", 2, 3)}
B, LQ, M, LD, D = 3, 5, 2, 7, 12
POS = [0, 2, 4]     # in-batch labels (never masked)
MASKED = (5,)       # query 2's second context (pairwise: never the positive)


def save(name, meta, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def inputs(kind, KQ, KD, seed):
    return MO.make_inputs(seed, kind, B=B, LQ=LQ, Nc=B * M, LD=LD, d=D, KQ=KQ, KD=KD, masked=MASKED)


def leaves(r):
    out = {}
    for k, t in r.items():
        t = t.detach().clone()
        if k == "expert_repr" or (k == "expert_weights" and t.is_floating_point()):
            t = t.float().requires_grad_(True)
        out[k] = t
    return out


def flat(prefix, r):
    return {f"{prefix}_{k}": v.detach().numpy() for k, v in r.items()}


def grads(prefix, r):
    return {f"{prefix}_{k}_grad": v.grad.numpy() for k, v in r.items() if v.requires_grad}


def ref_argmax(task, qr, cr, pairwise):
    """The reference's own token tensor (:155-213), reduced with .max(-1).indices: [B, LQ*KQ, Y]."""
    s = task.colbert_score(qr, cr, pairwise)
    if "expert_ids" in qr:
        s = (task.coil_score if qr["expert_ids"].dim() == 2 else task.citadel_score)(s, qr, cr, pairwise)
    return s.max(-1).indices


class ToyEncoder(torch.nn.Module):
    """Returns fixed repr leaves (what an encoder head hands the task)."""

    def __init__(self, r):
        super().__init__()
        self.r = r

    def forward(self, ids, **kw):
        return dict(self.r)


def main():
    torch.manual_seed(0)
    seed = 100
    for tag, (kind, KQ, KD) in KINDS.items():
        for mode in ("inbatch", "pairwise"):
            for pool in ("sum", "max"):
                seed += 1
                qr, cr, mask = inputs(kind, KQ, KD, seed)
                pairwise = mode == "pairwise"
                task = ref_shim.make_reference_citadel_task(in_batch=not pairwise)
                task.query_pool = pool
                with torch.no_grad():
                    S = task.expert_sim_score(leaves(qr), leaves(cr), mask.clone(), pairwise=pairwise)
                    arg = ref_argmax(task, leaves(qr), leaves(cr), pairwise)
                lq, lc = leaves(qr), leaves(cr)
                loss = task.expert_loss(lq, lc, mask.clone(), torch.tensor(POS), torch.zeros(B, M))
                loss.backward()
                meta = dict(case=f"{tag}_{mode}_{pool}", kind=kind, KQ=KQ, KD=KD, pairwise=pairwise, pool=pool, seed=seed, B=B, LQ=LQ,
                            M=M, LD=LD, d=D, logged=sorted(task.logged))
                save(f"multivec_{tag}_{mode}_{pool}", meta, mask=mask.numpy(), pos=np.array(POS), scores=S.numpy(),
                     argmax=arg.numpy(), loss=np.float32(loss.item()), **flat("q", qr), **flat("c", cr), **grads("q", lq),
                     **grads("c", lc))

    # distillation: in-batch CE + teacher term on the pairwise scores
    qr, cr, mask = inputs("citadel", 2, 3, 201)
    teacher = torch.from_numpy(np.random.default_rng(201).standard_normal((B, M)).astype(np.float32))
    task = ref_shim.make_reference_citadel_task(in_batch=True, teacher_coef=0.5, tau=2.0)
    lq, lc = leaves(qr), leaves(cr)
    loss = task.expert_loss(lq, lc, mask.clone(), torch.tensor(POS), teacher.clone())
    loss.backward()
    save("multivec_teacher", dict(case="teacher", kind="citadel", KQ=2, KD=3, teacher_coef=0.5, tau=2.0, pool="sum", in_batch=True,
                                  logged=sorted(task.logged)),
         mask=mask.numpy(), pos=np.array(POS), teacher=teacher.numpy(), loss=np.float32(loss.item()), **flat("q", qr), **flat("c", cr),
         **grads("q", lq), **grads("c", lc))

    # the training step with regularisers and distillation
    qr, cr, mask = inputs("citadel", 2, 3, 202)
    teacher = torch.from_numpy(np.random.default_rng(202).standard_normal((B, M)).astype(np.float32))
    task = ref_shim.make_reference_citadel_task(in_batch=True, teacher_coef=0.25, tau=1.0)
    task.query_expert_load_loss_coef, task.context_expert_load_loss_coef = 0.1, 0.2
    lq, lc = leaves(qr), leaves(cr)
    task.query_encoder, task.context_encoder = ToyEncoder(lq), ToyEncoder(lc)
    batch = {"query_ids": None, "contexts_ids": None, "pos_ctx_indices": torch.tensor(POS), "ctx_mask": mask.clone(),
             "scores": teacher.clone()}
    loss = task.training_step(batch, 0)
    loss.backward()
    save("multivec_step", dict(case="step", kind="citadel", KQ=2, KD=3, teacher_coef=0.25, tau=1.0, pool="sum", in_batch=True,
                               query_expert_load_loss_coef=0.1, context_expert_load_loss_coef=0.2, logged=sorted(task.logged)),
         mask=mask.numpy(), pos=np.array(POS), teacher=teacher.numpy(), loss=np.float32(loss.item()), **flat("q", qr), **flat("c", cr),
         **grads("q", lq), **grads("c", lc))

    # evaluation: _eval_step + _eval_epoch_end
    qr, cr, mask = inputs("colbert", 1, 1, 203)
    task = ref_shim.make_reference_citadel_task(in_batch=True)
    task.query_encoder, task.context_encoder = ToyEncoder(leaves(qr)), ToyEncoder(leaves(cr))
    batch = {"query_ids": None, "contexts_ids": None, "pos_ctx_indices": torch.tensor(POS), "ctx_mask": mask.clone(),
             "scores": torch.zeros(B, M)}
    with torch.no_grad():
        out = task._eval_step(batch, 0)
        task._eval_epoch_end([out])
    (rank, mrr, score), loss = out[0], out[-1]
    logged = {k: float(v) for k, v in task.logged.items()}
    save("multivec_eval", dict(case="eval", kind="colbert", KQ=1, KD=1, pool="sum", logged=logged),
         mask=mask.numpy(), pos=np.array(POS), metrics=np.array([rank, mrr, score], np.float64), loss=np.float32(loss.item()),
         **flat("q", qr), **flat("c", cr))


if __name__ == "__main__":
    main()
