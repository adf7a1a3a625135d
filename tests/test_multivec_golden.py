"""The late-interaction expert score pinned to tests/golden/multivec_*.npz, which scripts/make_multivec_golden.py wrote by running the
reference's own dpr_scale/task/citadel_task.py (MultiVecRetrieverTask: expert_sim_score :215-238, expert_loss :264-281, training_step
/ compute_loss :283-344, _eval_step / _eval_epoch_end :346-391) unmodified.  Nothing expected here is computed by the product.

CPU: the float64 oracle (tests/_multivec_oracle.py) against the fixtures, and the drop-in MultiVecRetrieverTask on the CPU stand-in
kernels against the reference task's loss, gradients and logged metric names.  GPU: the same through the HIP kernels."""
import numpy as np
import pytest
import torch

import _multivec_oracle as MO
from conftest import golden_names, load_golden

SCORE_CASES = [n for n in golden_names("multivec_") if n.split("_")[-1] in ("sum", "max")]


def _reprs(z, dev, grad=True):
    qr, cr = {}, {}
    for side, out in (("q", qr), ("c", cr)):
        for k in ("expert_repr", "expert_ids", "expert_weights"):
            key = f"{side}_{k}"
            if key in z:
                t = torch.from_numpy(z[key]).to(dev)
                if grad and (k == "expert_repr" or (k == "expert_weights" and t.is_floating_point())):
                    t = t.clone().requires_grad_(True)
                out[k] = t
    return qr, cr


def _check_grads(z, qr, cr, tol):
    n = 0
    for side, r in (("q", qr), ("c", cr)):
        for k, t in r.items():
            key = f"{side}_{k}_grad"
            if key in z:
                ref = z[key].astype(np.float64)
                got = t.grad.detach().double().cpu().numpy()
                assert np.abs(got - ref).max() <= tol * max(np.abs(ref).max(), 1e-30), key
                n += 1
    assert n >= 2


def _task(meta, kernels, dev):
    from test_multivec import make_task

    kw = {k: meta[k] for k in ("query_expert_load_loss_coef", "context_expert_load_loss_coef") if k in meta}
    return make_task(in_batch=meta.get("in_batch", not meta.get("pairwise", False)), query_pool=meta["pool"],
                     teacher_coef=meta.get("teacher_coef", 0.0), tau=meta.get("tau", 1.0), kernels=kernels, **kw)


class _Enc(torch.nn.Module):
    def __init__(self, r):
        super().__init__()
        self.r = r

    def forward(self, ids, **kw):
        return dict(self.r)


def _task_for(meta, kernels, dev, torch_ce):
    task = _task(meta, kernels, dev)
    if torch_ce:  # the reference's own loss, fp32 (isolates the expert score from the task's default loss)
        task.loss = torch.nn.CrossEntropyLoss()
    return task


# Gradient bars: with torch's fp32 cross-entropy the expert score's own bar (1e-3 of max |grad| on the GPU).  The task's default
# loss (HotCrossEntropyLoss) hands back bf16 dScores, as the DPR step does: its bar is the suite's 1e-2 for that rounding.
GRAD_TOL = {True: 1e-3, False: 1e-2}


def _run_expert_loss(name, kernels, dev, torch_ce=True):
    meta, z = load_golden(name)
    qr, cr = _reprs(z, dev)
    task = _task_for(meta, kernels, dev, torch_ce)
    mask = torch.from_numpy(z["mask"]).to(dev)
    loss = task.expert_loss(qr, cr, mask, torch.from_numpy(z["pos"]).to(dev), torch.from_numpy(z.get("teacher", np.zeros((3, 2), np.float32))).to(dev))
    loss.backward()
    return meta, z, task, loss, qr, cr


def _run_step(kernels, dev, torch_ce=True):
    meta, z = load_golden("multivec_step")
    qr, cr = _reprs(z, dev)
    task = _task_for(meta, kernels, dev, torch_ce)
    task.query_encoder, task.context_encoder = _Enc(qr), _Enc(cr)
    batch = {"query_ids": None, "contexts_ids": None, "pos_ctx_indices": torch.from_numpy(z["pos"]).to(dev),
             "ctx_mask": torch.from_numpy(z["mask"]).to(dev), "scores": torch.from_numpy(z["teacher"]).to(dev)}
    loss = task.training_step(batch, 0)
    loss.backward()
    return meta, z, task, loss, qr, cr


def _run_eval(kernels, dev):
    meta, z = load_golden("multivec_eval")
    qr, cr = _reprs(z, dev, grad=False)
    task = _task(meta, kernels, dev)
    task.query_encoder, task.context_encoder = _Enc(qr), _Enc(cr)
    batch = {"query_ids": None, "contexts_ids": None, "pos_ctx_indices": torch.from_numpy(z["pos"]).to(dev),
             "ctx_mask": torch.from_numpy(z["mask"]).to(dev), "scores": None}
    with torch.no_grad():
        out = task._eval_step(batch, 0)
        task._eval_epoch_end([out])
    return meta, z, task, out


def _check_loss(got, ref, tol):
    assert abs(float(got) - float(ref)) <= tol * max(1.0, abs(float(ref))), (float(got), float(ref))


# ---- CPU: the oracle and the drop-in's orchestration ----------------------------------------------------------------------------
def test_every_fixture_is_present():
    assert len(SCORE_CASES) == 16
    for n in ("multivec_teacher", "multivec_step", "multivec_eval"):
        assert n in golden_names("multivec_")


@pytest.mark.parametrize("name", SCORE_CASES)
def test_oracle_pinned_to_fixture(name):
    meta, z = load_golden(name)
    qr, cr = _reprs(z, "cpu", grad=False)
    mask = torch.from_numpy(z["mask"])
    S, arg, _ = MO.expert_sim_score(qr, cr, mask, meta["pairwise"], meta["pool"], return_argmax=True)
    assert np.array_equal(S.numpy(), z["scores"].astype(np.float64))  # grid inputs: exact in fp32 as in fp64
    assert np.array_equal(arg.numpy(), z["argmax"])


@pytest.fixture
def standin():
    from _multivec_standin import MultiVecKernels

    return MultiVecKernels()


@pytest.mark.parametrize("torch_ce", [True, False])
@pytest.mark.parametrize("name", SCORE_CASES + ["multivec_teacher"])
def test_dropin_expert_loss_matches_reference_on_standin(name, torch_ce, standin):
    meta, z, task, loss, qr, cr = _run_expert_loss(name, standin, "cpu", torch_ce)
    _check_loss(loss.item(), z["loss"], 1e-5)
    _check_grads(z, qr, cr, 1e-4 if torch_ce else GRAD_TOL[False])
    assert sorted(task.logged) == meta["logged"]


@pytest.mark.parametrize("torch_ce", [True, False])
def test_dropin_training_step_matches_reference_on_standin(torch_ce, standin):
    meta, z, task, loss, qr, cr = _run_step(standin, "cpu", torch_ce)
    _check_loss(loss.item(), z["loss"], 1e-5)
    _check_grads(z, qr, cr, 1e-4 if torch_ce else GRAD_TOL[False])
    assert sorted(task.logged) == meta["logged"]


def test_dropin_eval_matches_reference_on_standin(standin):
    meta, z, task, out = _run_eval(standin, "cpu")
    assert np.allclose(np.array(out[0], np.float64), z["metrics"], rtol=1e-6)
    _check_loss(out[-1], z["loss"], 1e-5)
    assert set(task.logged) == set(meta["logged"])
    for k, v in meta["logged"].items():
        assert abs(float(task.logged[k]) - v) <= 1e-5 * max(1.0, abs(v)), k


# ---- GPU: the HIP path -------------------------------------------------------------------------------------------------------------
DEV = torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORE_CASES)
def test_hip_scores_and_argmax_pinned_to_fixture(name):
    from dpr_scale_amd import hotpath

    meta, z = load_golden(name)
    qr, cr = _reprs(z, DEV, grad=False)
    S = hotpath.expert_sim_score(qr, cr, torch.from_numpy(z["mask"]).to(DEV), meta["pairwise"], meta["pool"])
    assert np.array_equal(S.cpu().numpy(), z["scores"])
    # the argmax tables the backward reads (workspace layout of include/dprhot.h: value table, then argmax table)
    kn = hotpath.default_kernels()
    KQ, KD = meta["KQ"], meta["KD"]
    pad = (-meta["d"]) % 32
    Qb = torch.nn.functional.pad(qr["expert_repr"], (0, pad)).to(torch.bfloat16).contiguous()
    Cb = torch.nn.functional.pad(cr["expert_repr"], (0, pad)).to(torch.bfloat16).contiguous()
    ids = [qr[k].to(torch.int32).contiguous() if k in qr else None for k in ("expert_ids",)] + \
          [cr["expert_ids"].to(torch.int32).contiguous() if "expert_ids" in cr else None]
    w = [qr["expert_weights"].float().contiguous() if "expert_weights" in qr else None,
         cr["expert_weights"].float().contiguous() if "expert_weights" in cr else None]
    M = meta["M"] if meta["pairwise"] else 0
    _, state = kn.maxsim_fwd(Qb, Cb, ids[0], ids[1], w[0], w[1], KQ, KD, 0 if meta["pool"] == "sum" else 1, M, None)
    Bq, Y = z["argmax"].shape[0], z["argmax"].shape[2]
    tab = Y * Bq * meta["LQ"] * KQ * 4
    off = (tab + 255) // 256 * 256
    arg = state[off:off + tab].view(torch.int32).view(Y, -1).cpu().numpy()
    assert np.array_equal(arg, z["argmax"].transpose(2, 0, 1).reshape(Y, -1))


@pytest.mark.gpu
@pytest.mark.parametrize("torch_ce", [True, False])
@pytest.mark.parametrize("name", SCORE_CASES + ["multivec_teacher"])
def test_hip_dropin_expert_loss_matches_reference(name, torch_ce):
    meta, z, task, loss, qr, cr = _run_expert_loss(name, None, DEV, torch_ce)
    _check_loss(loss.item(), z["loss"], 1e-4)
    _check_grads(z, qr, cr, GRAD_TOL[torch_ce])
    assert sorted(task.logged) == meta["logged"]


@pytest.mark.gpu
@pytest.mark.parametrize("torch_ce", [True, False])
def test_hip_dropin_training_step_and_eval_match_reference(torch_ce):
    meta, z, task, loss, qr, cr = _run_step(None, DEV, torch_ce)
    _check_loss(loss.item(), z["loss"], 1e-4)
    _check_grads(z, qr, cr, GRAD_TOL[torch_ce])
    assert sorted(task.logged) == meta["logged"]
    meta, z, task, out = _run_eval(None, DEV)
    assert np.allclose(np.array(out[0], np.float64), z["metrics"], rtol=1e-6)
    _check_loss(out[-1], z["loss"], 1e-4)
    assert set(task.logged) == set(meta["logged"])
