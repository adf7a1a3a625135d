"""CPU side of the late-interaction expert score (hotpath.expert_sim_score, task/multivec.py, task/citadel_task.py): the float64
oracle against the reference's own citadel_task.py where that tree is present, the drop-in task's orchestration on the CPU stand-in
kernels, host-side validation of the new C-ABI entry points and the compiler's resource report of the new kernels."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _multivec_oracle as MO
from conftest import ROOT
from oracle import ref_shim

SHAPES = {"colbert": dict(KQ=1, KD=1), "coil": dict(KQ=1, KD=1), "citadel": dict(KQ=2, KD=3)}
needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference tree not present")


def make_task(in_batch=True, query_pool="sum", teacher_coef=0.0, kernels=None, **kw):
    from dpr_scale_amd.task.citadel_task import MultiVecRetrieverTask

    task = MultiVecRetrieverTask(in_batch=in_batch, query_pool=query_pool, teacher_coef=teacher_coef, transform=None, model=None,
                                 datamodule=None, optim=None, **kw)
    task.kernels = kernels
    task.loss.kernels = kernels  # (HotCrossEntropyLoss carries its own)
    from types import SimpleNamespace

    task.trainer = SimpleNamespace(strategy=object(), max_epochs=1)
    return task


class _ToyEncoder(torch.nn.Module):
    """Returns a repr dict the way the reference's encoder heads do, from fixed tensors scaled by one trainable parameter."""

    def __init__(self, repr_):
        super().__init__()
        self.repr = repr_
        self.scale = torch.nn.Parameter(torch.ones(()))

    def forward(self, ids, **kw):
        out = dict(self.repr)
        out["expert_repr"] = self.repr["expert_repr"] * self.scale
        return out


def toy_batch(seed, kind, dev=torch.device("cpu")):
    qr, cr, mask = MO.make_inputs(seed, kind, B=3, LQ=6, Nc=6, LD=9, d=16, masked=(5,), **SHAPES[kind])
    batch = {"query_ids": None, "contexts_ids": None, "pos_ctx_indices": torch.tensor([0, 2, 4], device=dev),
             "ctx_mask": mask.to(dev), "scores": torch.zeros(3, 2, device=dev)}
    return batch, qr, cr


def _attach(task, qr, cr, dev):
    to = lambda r: {k: v.to(dev) for k, v in r.items()}
    task.query_encoder, task.context_encoder = _ToyEncoder(to(qr)).to(dev), _ToyEncoder(to(cr)).to(dev)
    return task


@pytest.fixture
def standin():
    from _multivec_standin import MultiVecKernels

    return MultiVecKernels()


@needs_reference
@pytest.mark.parametrize("kind", MO.KINDS)
@pytest.mark.parametrize("pairwise", [False, True])
@pytest.mark.parametrize("pool", ["sum", "max"])
def test_oracle_equals_reference(kind, pairwise, pool):
    qr, cr, mask = MO.make_inputs(5, kind, B=3, LQ=5, Nc=6, LD=7, d=8, masked=(1,), **SHAPES[kind])
    ref = ref_shim.make_reference_citadel_task()
    ref.query_pool = pool
    f64 = lambda r: {k: (v.double() if v.is_floating_point() else v) for k, v in r.items()}
    want = ref.expert_sim_score(f64(qr), f64(cr), mask.clone(), pairwise=pairwise)
    got = MO.expert_sim_score(qr, cr, mask, pairwise, pool)
    assert torch.equal(got, want)


@needs_reference
def test_constructor_signature_equals_reference():
    from dpr_scale_amd.task.citadel_task import MultiVecRetrieverTask

    ref = ref_shim.load_reference_citadel_class()
    assert str(inspect.signature(MultiVecRetrieverTask.__init__)) == str(inspect.signature(ref.__init__))


def test_constructor_signature():
    from dpr_scale_amd.task.citadel_task import MultiVecRetrieverTask

    names = list(inspect.signature(MultiVecRetrieverTask.__init__).parameters)
    assert names == ["self", "add_cls", "query_topk", "context_topk", "query_expert_load_loss_coef", "context_expert_load_loss_coef",
                     "query_router_marg_load_loss_coef", "context_router_marg_load_loss_coef", "cross_batch", "in_batch", "query_pool",
                     "anneal_factor", "teacher_coef", "tau", "kwargs"]


def test_oracle_grid_inputs_are_exact_in_fp32():
    qr, cr, mask = MO.make_inputs(1, "citadel", B=2, LQ=4, Nc=4, LD=6, d=32, KQ=2, KD=2)
    f32 = {k: (v.float() if v.is_floating_point() else v) for k, v in qr.items()}
    c32 = {k: (v.float() if v.is_floating_point() else v) for k, v in cr.items()}
    s64 = MO.expert_sim_score(qr, cr, mask)
    bf = lambda r: {k: (v.to(torch.bfloat16).float() if k == "expert_repr" else v) for k, v in r.items()}
    assert torch.equal(MO.expert_sim_score(bf(f32), bf(c32), mask), s64)


@pytest.mark.parametrize("kind", MO.KINDS)
@pytest.mark.parametrize("in_batch", [True, False])
@pytest.mark.parametrize("pool", ["sum", "max"])
def test_expert_score_orchestration_on_standin(kind, in_batch, pool, standin):
    from dpr_scale_amd import hotpath

    qr, cr, mask = MO.make_inputs(8, kind, B=3, LQ=5, Nc=6, LD=7, d=20, masked=(3,), **SHAPES[kind])
    lq, lc = MO.leaf(qr), MO.leaf(cr)
    gq = {k: (v.float().detach().requires_grad_(v.requires_grad) if v.is_floating_point() else v) for k, v in lq.items()}
    gc = {k: (v.float().detach().requires_grad_(v.requires_grad) if v.is_floating_point() else v) for k, v in lc.items()}
    S = hotpath.expert_sim_score(gq, gc, mask, not in_batch, pool, standin)
    S0 = MO.expert_sim_score(lq, lc, mask, not in_batch, pool)
    assert torch.equal(S.double(), S0.detach())
    dS = torch.randn(S.shape, generator=torch.Generator().manual_seed(0))
    fin = torch.isfinite(S0)
    (S.masked_fill(~fin, 0) * dS).sum().backward()
    (S0.masked_fill(~fin, 0) * dS.double()).sum().backward()
    for a, b in ((gq, lq), (gc, lc)):
        for k in ("expert_repr", "expert_weights"):
            if k in b and b[k].requires_grad:
                assert torch.allclose(a[k].grad.double(), b[k].grad, atol=1e-5), k


def test_expert_score_rejects_too_many_slots(standin):
    from dpr_scale_amd import hotpath

    qr, cr, _ = MO.make_inputs(1, "citadel", B=1, LQ=2, Nc=2, LD=2, d=8, KQ=1, KD=9, n_experts=12)
    with pytest.raises(ValueError, match="1..8"):
        hotpath.expert_sim_score(qr, cr, None, False, "sum", standin)
    with pytest.raises(NotImplementedError):
        hotpath.expert_sim_score(qr, cr, None, False, "mean", standin)


@pytest.mark.parametrize("kind", MO.KINDS)
@pytest.mark.parametrize("in_batch", [True, False])
def test_dropin_training_and_eval_step_on_standin(kind, in_batch, standin):
    batch, qr, cr = toy_batch(3, kind)
    task = _attach(make_task(in_batch=in_batch, kernels=standin), qr, cr, torch.device("cpu"))
    task.loss = torch.nn.CrossEntropyLoss()
    loss = task.training_step(batch, 0)
    loss.backward()
    S0 = MO.expert_sim_score(qr, cr, batch["ctx_mask"], not in_batch).float()
    labels = batch["pos_ctx_indices"] if in_batch else torch.zeros(3, dtype=torch.int64)
    ref = torch.nn.functional.cross_entropy(S0, labels)
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    assert set(task.logged) == {"train_expert_loss"}
    assert task.query_encoder.scale.grad is not None and torch.isfinite(task.query_encoder.scale.grad)
    if in_batch:
        with torch.no_grad():  # (Lightning runs the eval hooks without grad)
            metrics, *_, eval_loss = task._eval_step(batch, 0)
            outputs = [task._eval_step(batch, 0)]
        assert abs(float(eval_loss) - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
        task._eval_epoch_end(outputs)
        assert {"valid_avg_rank", "valid_mrr", "valid_accuracy@1", "valid_ctx_count", "valid_expert_loss"} <= set(task.logged)


def test_dropin_teacher_distillation_and_regularisers_on_standin(standin):
    batch, qr, cr = toy_batch(4, "citadel")
    task = _attach(make_task(teacher_coef=0.5, kernels=standin, query_expert_load_loss_coef=0.1,
                             context_expert_load_loss_coef=0.2), qr, cr, torch.device("cpu"))
    task.loss = torch.nn.CrossEntropyLoss()
    batch["scores"] = torch.randn(3, 2, generator=torch.Generator().manual_seed(2))
    loss = task.training_step(batch, 0)
    from dpr_scale_amd.task.citadel_router import distilled_loss

    S0 = MO.expert_sim_score(qr, cr, batch["ctx_mask"]).float()
    P0 = MO.expert_sim_score(qr, cr, batch["ctx_mask"], pairwise=True).float()
    ref = 0.5 * torch.nn.functional.cross_entropy(S0, batch["pos_ctx_indices"]) + 0.5 * distilled_loss(P0, batch["scores"])
    ref = ref + 0.1 * qr["expert_weights"].sum(1).sum(1).mean(0) + 0.2 * cr["expert_weights"].sum(1).sum(1).mean(0)
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    assert {"train_expert_loss", "train_query_expert_load_loss", "train_context_expert_load_loss"} <= set(task.logged)


def test_maxsim_argument_validation_is_host_side():
    from dpr_scale_amd import _lib

    lib = _lib.lib
    out = ctypes.c_size_t(0)
    assert lib.dprhot_maxsim_workspace_bytes(4, 32, 2, 64, 1, ctypes.byref(out)) == 0 and out.value >= 3 * 4 * 32 * 2 * 64 * 4
    assert lib.dprhot_maxsim_workspace_bytes(4, 32, 9, 64, 1, ctypes.byref(out)) == -1
    assert b"KQ=9" in lib.dprhot_last_error()
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: validation fails first
    ws = ctypes.c_void_p(1 << 21)
    args = lambda **kw: dict(dict(Nq=2, LQ=4, Nc=4, LD=8, dp=32, KQ=1, KD=1, pool=0, M=0, ids=None, w=None, nbytes=1 << 30), **kw)

    def fwd(a):
        return lib.dprhot_maxsim_fwd(fake, fake, a["Nq"], a["LQ"], a["Nc"], a["LD"], a["dp"], a["ids"], a["ids"], a["w"], a["w"],
                                     a["KQ"], a["KD"], a["pool"], a["M"], None, fake, ws, a["nbytes"], None)

    assert fwd(args(dp=40)) == -1 and b"multiple of 32" in lib.dprhot_last_error()
    assert fwd(args(LD=513)) == -1 and b"limited" in lib.dprhot_last_error()
    assert fwd(args(KD=2)) == -1 and b"without expert ids" in lib.dprhot_last_error()
    assert fwd(args(ids=fake, KD=9)) == -1 and b"1..8" in lib.dprhot_last_error()
    assert fwd(args(pool=2)) == -1 and b"pool" in lib.dprhot_last_error()
    assert fwd(args(M=3)) == -1 and b"pairwise" in lib.dprhot_last_error()
    assert fwd(args(nbytes=16)) == -1 and b"workspace" in lib.dprhot_last_error()
    assert lib.dprhot_maxsim_fwd(None, fake, 2, 4, 4, 8, 32, None, None, None, None, 1, 1, 0, 0, None, fake, ws, 1 << 30, None) == -1
    assert lib.dprhot_maxsim_bwd(None, fake, fake, 2, 4, 4, 8, 32, None, None, None, None, 1, 1, 0, 0, None, ws, 1 << 30, fake, fake,
                                 None, None, None) == -1
    assert b"dS" in lib.dprhot_last_error()


REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")


@pytest.mark.skipif(not os.path.isfile(REPORT), reason="no resource report next to the library (built without the Makefile)")
def test_maxsim_kernels_never_spill():
    cur, rows = None, {}
    for ln in open(REPORT, errors="replace"):
        m = re.search(r" Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", ln)
        if m and cur:
            rows[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    ms = {k: v for k, v in rows.items() if re.search(r"dprhot\d+ms_(fwd|pool|dq|dc)_kernel", k)}
    assert len(ms) >= 16 + 1 + 4 + 4, sorted(ms)
    for name, r in ms.items():
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)
