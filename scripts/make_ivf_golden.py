#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/ivf_{coil,citadel11,citadel23}[_cls].npz from the reference's own tasks.

Run where the reference tree is present:   python scripts/make_ivf_golden.py

For every case the script
  1. runs the reference's GenerateMultiVecEmbeddingsTask._eval_step and test_epoch_end (citadel_eval_task.py:44-120), imported
     unmodified, on a stand-in context encoder that returns the repr dicts of tests/_multivec_oracle.make_inputs, and reads the index
     files it wrote (expert_0000/{id}.pkl, cls_0000.pkl);
  2. runs the reference's CITADELRetrievalTask._eval_step (citadel_retrieval_task.py:84-140) against a recording stand-in for the
     index module the reference does not ship, and captures (batch_cls, batch_embeddings, batch_weights, topk);
  3. computes the expected scores with the reference's MultiVecRetrieverTask.expert_sim_score (query_pool = "sum",
     citadel_task.py:215-238) plus sim_score on cls_repr (:137-153), asserts for every passage that a padded slot exists (so that the
     reference's max over slots sees a 0 and equals max(0, .)), and takes the top-k in (score descending, lower id first) order after
     checking it against torch.topk;
  4. formats the result with the reference's merge_trec_results (:179-201).
Import stand-ins installed here, next to oracle.ref_shim's: pytorch_lightning.utilities.cloud_io (checkpoint loading is never
reached), dpr_scale.index.inverted_vector_index (absent from the reference), dpr_scale.datamodule.citadel when its own imports are
missing (only setup() uses it; setup() is not run).  A single-process gloo group serves test_epoch_end's barrier.
Inputs are grid values (exact in bf16, every sum exact in fp32), the last token of every query and passage is padding.
"""
import glob
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
CASES = {"coil": ("coil", 1, 1), "citadel11": ("citadel", 1, 1), "citadel23": ("citadel", 2, 3)}
NQ, LQ, NDOC, LD, D, DC, TOPK, NEXP = 4, 6, 20, 7, 32, 16, 8, 6
NOTES = []


class Recorder:
    """Stands where IVFGPUIndex stood: records the arguments of search() and answers with the expected result."""

    def __init__(self, answer):
        self.answer, self.calls = answer, []

    def search(self, batch_cls, batch_embeddings, batch_weights, topk):
        self.calls.append((batch_cls, batch_embeddings, batch_weights, topk))
        return self.answer


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
    index = types.ModuleType("dpr_scale.index.inverted_vector_index")
    for name in ("IVFGPUIndex", "IVFCPUIndex", "IVFPQGPUIndex", "IVFPQCPUIndex"):
        setattr(index, name, Recorder)
    pkg = types.ModuleType("dpr_scale.index")
    pkg.__path__ = []
    sys.modules.setdefault("dpr_scale.index", pkg)
    sys.modules["dpr_scale.index.inverted_vector_index"] = index
    try:
        import dpr_scale.datamodule.citadel  # noqa: F401
    except Exception as exc:  # its own imports (tokenizers, ujson ...) are not needed by the methods run here
        mod = types.ModuleType("dpr_scale.datamodule.citadel")
        mod.IDCSVDataset = object
        sys.modules["dpr_scale.datamodule.citadel"] = mod
        NOTES.append(f"dpr_scale.datamodule.citadel replaced by a stand-in ({type(exc).__name__})")


class ToyEncoder(torch.nn.Module):
    def __init__(self, r):
        super().__init__()
        self.r = r

    def forward(self, ids, **kw):
        return dict(self.r)


def pad_last(r):
    """The last token of every sequence becomes padding: zero vector, weight 0."""
    r = {k: v.clone() for k, v in r.items()}
    r["expert_repr"][:, -1] = 0
    r["expert_weights"][:, -1] = 0
    w = r["expert_weights"]
    r["attention_mask"] = (w.reshape(w.shape[0], w.shape[1], -1).sum(-1) > 0).long()
    return r


def grid_cls(seed, n):
    g = np.random.default_rng(seed)
    return torch.from_numpy(g.integers(-4, 5, size=(n, DC)).astype(np.float32) / 4.0)


def base_kwargs():
    return dict(transform=None, model=None, datamodule=None, optim=None)


def main():
    install_stubs()
    from dpr_scale.task.citadel_eval_task import GenerateMultiVecEmbeddingsTask
    from dpr_scale.task.citadel_retrieval_task import CITADELRetrievalTask
    import torch.distributed as dist

    store = tempfile.mkdtemp()
    dist.init_process_group("gloo", init_method=f"file://{store}/pg", rank=0, world_size=1)
    seed = 300
    for tag, (kind, KQ, KD) in CASES.items():
        for with_cls in (False, True):
            seed += 1
            qr, cr, _ = MO.make_inputs(seed, kind, B=NQ, LQ=LQ, Nc=NDOC, LD=LD, d=D, KQ=KQ, KD=KD, n_experts=NEXP)
            qr, cr = pad_last(qr), pad_last(cr)
            if with_cls:
                qr["cls_repr"], cr["cls_repr"] = grid_cls(seed, NQ), grid_cls(seed + 1000, NDOC)
            assert bool((cr["attention_mask"] == 0).any(1).all()) and bool((qr["attention_mask"] == 0).any(1).all())
            cw = cr["expert_weights"].reshape(NDOC, -1)
            assert bool((cw == 0).any(1).all()), "every passage needs a slot of weight 0: the reference's max then equals max(0, .)"

            # 3. expected scores from the reference's training score
            score_task = ref_shim.make_reference_citadel_task(in_batch=True)
            score_task.query_pool = "sum"
            nomask = torch.zeros(NDOC, dtype=torch.bool)
            sq = {k: v for k, v in qr.items() if k.startswith("expert")}
            sc = {k: v for k, v in cr.items() if k.startswith("expert")}
            if kind == "citadel":
                sq["expert_weights"], sc["expert_weights"] = sq["expert_weights"].float(), sc["expert_weights"].float()
            with torch.no_grad():
                S = score_task.expert_sim_score(sq, sc, nomask.clone(), pairwise=False).float()
                if with_cls:
                    S = S + score_task.sim_score(qr["cls_repr"], cr["cls_repr"], nomask.clone(), pairwise=False)
            S = S.numpy().astype(np.float32)
            ids = np.stack([np.lexsort((np.arange(NDOC), -row))[:TOPK] for row in S])
            top = np.take_along_axis(S, ids, 1)
            assert np.array_equal(top, torch.topk(torch.from_numpy(S), TOPK, dim=1).values.numpy())

            # 1. the reference's index writer
            tmp = tempfile.mkdtemp()
            gen = GenerateMultiVecEmbeddingsTask(ctx_embeddings_dir=tmp, checkpoint_path="", add_context_id=False, **base_kwargs())
            gen.global_rank = 0
            half = NDOC // 2
            outs = []
            for lo, hi in ((0, half), (half, NDOC)):
                gen.context_encoder = ToyEncoder({k: v[lo:hi] for k, v in cr.items()})
                batch = {"contexts_ids": {"input_ids": torch.zeros((hi - lo, LD + 1), dtype=torch.long)}, "corpus_ids": list(range(lo, hi))}
                with torch.no_grad():
                    outs.append(gen._eval_step(batch, 0))
            gen.test_epoch_end(outs)
            pe, pd, pw, pv = [], [], [], []
            for path in sorted(glob.glob(os.path.join(tmp, "expert_0000", "*.pkl")), key=lambda p: int(os.path.basename(p)[:-4])):
                with open(path, "rb") as f:
                    i_, w_, r_ = pickle.load(f)
                assert i_.dtype == torch.int64 and w_.dtype == torch.float32 and r_.dtype == torch.float32
                pe.append(np.full(len(i_), int(os.path.basename(path)[:-4]), np.int64))
                pd.append(i_.numpy()), pw.append(w_.numpy()), pv.append(r_.numpy())
            arrays = dict(post_expert=np.concatenate(pe), post_doc=np.concatenate(pd), post_weight=np.concatenate(pw),
                          post_vec=np.concatenate(pv))
            if with_cls:
                with open(os.path.join(tmp, "cls_0000.pkl"), "rb") as f:
                    arrays["cls_doc"] = pickle.load(f).numpy()
                assert np.array_equal(arrays["cls_doc"], cr["cls_repr"].numpy())

            # 2. the reference's query side against the recording index
            ret = CITADELRetrievalTask(ctx_embeddings_dir=tmp, checkpoint_path="", topk=TOPK, **base_kwargs())
            ret.global_rank = 0
            ret.query_encoder = ToyEncoder(qr)
            ret.index = Recorder((torch.from_numpy(top), torch.from_numpy(ids)))
            topics = [f"t{n}" for n in range(NQ)]
            with torch.no_grad():
                out = ret._eval_step({"query_ids": {"input_ids": torch.zeros((NQ, LQ), dtype=torch.long)}, "topic_ids": topics}, 0)
            (b_cls, b_emb, b_w, k), = ret.index.calls
            assert k == TOPK
            eq, ee, ev, ew, dtypes = [], [], [], [], set()
            for n, (by_e, by_w) in enumerate(zip(b_emb, b_w)):
                for e, lst in by_e.items():
                    for v, w in zip(lst, by_w[e]):
                        dtypes.add(str(v.dtype))
                        eq.append(n), ee.append(int(e)), ev.append(v.float().numpy()), ew.append(float(w))
            arrays.update(ent_query=np.array(eq, np.int64), ent_expert=np.array(ee, np.int64), ent_vec=np.stack(ev).astype(np.float32),
                          ent_weight=np.array(ew, np.float32))
            if with_cls:
                arrays["cls_q"] = b_cls.float().numpy()
            trec = ret.merge_trec_results(out[2], out[1], out[0])
            name = f"ivf_{tag}{'_cls' if with_cls else ''}"
            meta = dict(case=name, kind=kind, KQ=KQ, KD=KD, seed=seed, nq=NQ, corpus_len=NDOC, d=D, topk=TOPK, entry_dtype=sorted(dtypes),
                        topics=topics, trec=trec, shim_notes=NOTES,
                        reference_methods=["GenerateMultiVecEmbeddingsTask._eval_step", "GenerateMultiVecEmbeddingsTask.test_epoch_end",
                                           "CITADELRetrievalTask._eval_step", "CITADELRetrievalTask.merge_trec_results",
                                           "MultiVecRetrieverTask.expert_sim_score", "MultiVecRetrieverTask.sim_score"])
            path = os.path.join(OUT, name + ".npz")
            np.savez_compressed(path, meta=np.array(json.dumps(meta)), scores=S, top_scores=top, top_ids=ids.astype(np.int64), **arrays)
            size = os.path.getsize(path)
            assert size < 64 * 1024, size
            print(f"{name}: {size / 1024:.1f} KiB, {len(arrays['post_doc'])} postings, {len(eq)} entries, dtypes {sorted(dtypes)}")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
