#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/rerank_*.npz from the reference's own rerank tasks.

Run where the reference tree is present:   python scripts/make_rerank_golden.py

For every case the script imports RerankMultiVecRetrieverTask (citadel_eval_task.py:215-313) or RerankDenseRetrieverTask
(dpr_rerank_task.py) unmodified and
  1. runs its expert_sim_score (multi-vector) on B aligned (query, passage) pairs in fp32;
  2. runs _eval_step on two batches (the pairs split 3 + 2) through stand-in encoders that return fixed reprs;
  3. runs test_epoch_end and unpickles scores_0000.pkl, qids_0000.pkl and ctx_ids_0000.pkl.
Inputs come from tests/_multivec_oracle.make_inputs: grid values (exact in bf16, every sum exact in fp32), Nc = B, the last passage
all padding.  Cases: ColBERT, COIL, CITADEL at (KQ, KD) = (1, 1) and (2, 3), each with `sum` and `max` pooling; CITADEL (2, 3) with
cls_repr; one dense case.  Import stand-ins installed here, next to oracle.ref_shim's: pytorch_lightning.utilities.cloud_io
(checkpoint loading is never reached) and tqdm when it is missing.  A single-process gloo group serves test_epoch_end's barrier.
"""
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402
import _multivec_oracle as MO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
KINDS = {"colbert": ("colbert", 1, 1), "coil": ("coil", 1, 1), "citadel11": ("citadel", 1, 1), "citadel23": ("citadel", 2, 3)}
B, LQ, LD, D, DC, NEXP, SPLIT = 5, 9, 21, 40, 16, 6, 3
NOTES = []


def install_stubs():
    ref_shim.load_reference_citadel_class()  # installs the pytorch_lightning / hydra stand-ins, puts the reference on sys.path
    pl = sys.modules["pytorch_lightning"]
    util = types.ModuleType("pytorch_lightning.utilities")
    cloud = types.ModuleType("pytorch_lightning.utilities.cloud_io")
    cloud.load = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("checkpoint loading is not part of the fixture run"))
    util.cloud_io = cloud
    pl.utilities = util
    sys.modules["pytorch_lightning.utilities"] = util
    sys.modules["pytorch_lightning.utilities.cloud_io"] = cloud
    try:
        import tqdm  # noqa: F401
    except ImportError:
        t = types.ModuleType("tqdm")
        t.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = t
        NOTES.append("tqdm replaced by the identity")


class ToyEncoder(torch.nn.Module):
    """Returns rows [lo, hi) of fixed reprs (a dict, or a tensor for the dense task)."""

    def __init__(self, r):
        super().__init__()
        self.r, self.rows = r, slice(None)

    def forward(self, ids, **kw):
        if isinstance(self.r, dict):
            return {k: v[self.rows].clone() for k, v in self.r.items()}
        return self.r[self.rows].clone()


def grid(seed, n, d):
    g = np.random.default_rng(seed)
    return torch.from_numpy(g.integers(-4, 5, size=(n, d)).astype(np.float32) / 4.0)


def f32(r):
    return {k: (v.float() if v.is_floating_point() else v) for k, v in r.items()}


def run_task(task, q, c, qids, ctx_ids, tmp):
    """_eval_step on the two batches, test_epoch_end, and what the three files hold."""
    task.global_rank = 0
    task.query_encoder, task.context_encoder = ToyEncoder(q), ToyEncoder(c)
    outs = []
    for lo, hi in ((0, SPLIT), (SPLIT, B)):
        task.query_encoder.rows = task.context_encoder.rows = slice(lo, hi)
        with torch.no_grad():
            outs.append(task._eval_step({"query_ids": None, "contexts_ids": None, "qid": qids[lo:hi], "ctx_id": ctx_ids[lo:hi]}, 0))
    step_scores = torch.cat([o[2] for o in outs]).numpy()
    task.test_epoch_end(outs)
    assert sorted(os.listdir(tmp)) == ["ctx_ids_0000.pkl", "qids_0000.pkl", "scores_0000.pkl"], os.listdir(tmp)
    files = {}
    for name in ("scores", "qids", "ctx_ids"):
        with open(os.path.join(tmp, f"{name}_0000.pkl"), "rb") as f:
            files[name] = pickle.load(f)
    assert isinstance(files["scores"], torch.Tensor) and files["scores"].dtype == torch.float32 and files["scores"].shape == (B,)
    assert type(files["qids"]) is list and type(files["ctx_ids"]) is list
    assert np.array_equal(files["scores"].numpy(), step_scores)
    return step_scores, files


def save(name, meta, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    size = os.path.getsize(path)
    assert size < 16 * 1024, size
    print(f"{name}: {size / 1024:.1f} KiB")


def main():
    install_stubs()
    from dpr_scale.task.citadel_eval_task import RerankMultiVecRetrieverTask
    from dpr_scale.task.dpr_rerank_task import RerankDenseRetrieverTask
    import torch.distributed as dist

    store = tempfile.mkdtemp()
    dist.init_process_group("gloo", init_method=f"file://{store}/pg", rank=0, world_size=1)
    base = dict(transform=None, model=None, datamodule=None, optim=None)
    qids = [100 + b for b in range(B)]           # the reference's datamodule yields int query ids for numeric ones
    ctx_ids = [f"d{7 * b + 3}" for b in range(B)]  # and passage ids as read (strings)
    common = dict(B=B, LQ=LQ, LD=LD, d=D, split=SPLIT, qids=qids, ctx_ids=ctx_ids, file_types={"scores": "torch.float32 tensor [B]",
                  "qids": "list", "ctx_ids": "list"}, pickle_protocol=4)
    seed = 500
    cases = [(tag, pool, False) for tag in KINDS for pool in ("sum", "max")] + [("citadel23", "sum", True)]
    for tag, pool, with_cls in cases:
        seed += 1
        kind, KQ, KD = KINDS[tag]
        qr, cr, _ = MO.make_inputs(seed, kind, B=B, LQ=LQ, Nc=B, LD=LD, d=D, KQ=KQ, KD=KD, n_experts=NEXP, all_pad=(B - 1,))
        qr, cr = f32(qr), f32(cr)
        if with_cls:
            qr["cls_repr"], cr["cls_repr"] = grid(seed, B, DC), grid(seed + 1000, B, DC)
        tmp = tempfile.mkdtemp()
        task = RerankMultiVecRetrieverTask(checkpoint_path="", output_dir=tmp, query_pool=pool, **base)
        with torch.no_grad():
            expert = task.expert_sim_score({k: v.clone() for k, v in qr.items()}, {k: v.clone() for k, v in cr.items()})
        assert expert.dtype == torch.float32 and expert.shape == (B,)
        step_scores, files = run_task(task, qr, cr, qids, ctx_ids, tmp)
        if not with_cls:
            assert np.array_equal(step_scores, expert.numpy())
        assert files["qids"] == qids and files["ctx_ids"] == ctx_ids
        arrays = {f"{side}_{k}": v.numpy() for side, r in (("q", qr), ("c", cr)) for k, v in r.items()}
        name = f"rerank_{tag}_{pool}" + ("_cls" if with_cls else "")
        meta = dict(common, case=name, kind=kind, KQ=KQ, KD=KD, pool=pool, seed=seed, cls=with_cls, shim_notes=NOTES,
                    reference_methods=["RerankMultiVecRetrieverTask.expert_sim_score", "RerankMultiVecRetrieverTask._eval_step",
                                       "RerankMultiVecRetrieverTask.test_epoch_end"])
        save(name, meta, expert_scores=expert.numpy(), scores=step_scores, file_scores=files["scores"].numpy(), **arrays)

    seed += 1
    q, c = grid(seed, B, D), grid(seed + 1000, B, D)
    tmp = tempfile.mkdtemp()
    task = RerankDenseRetrieverTask(checkpoint_path="", output_dir=tmp, **base)
    step_scores, files = run_task(task, q, c, qids, ctx_ids, tmp)
    assert files["qids"] == qids and files["ctx_ids"] == ctx_ids
    meta = dict(common, case="rerank_dense", kind="dense", seed=seed, shim_notes=NOTES,
                reference_methods=["RerankDenseRetrieverTask._eval_step", "RerankDenseRetrieverTask.test_epoch_end"])
    save("rerank_dense", meta, q=q.numpy(), c=c.numpy(), scores=step_scores, file_scores=files["scores"].numpy())
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
