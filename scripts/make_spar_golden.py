#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/spar_{concat,sum,mean}.npz and tests/golden/spar_task.npz from the reference's own
spar/spar_retrieval.py and dpr_scale/task/spar_task.py.

Run where the reference tree is present:   python scripts/make_spar_golden.py

Retrieval.  spar/spar_retrieval.py is imported from the reference tree, unmodified.  It imports `faiss`, which is not installed: a numpy
stand-in for the one class it uses, faiss.IndexFlatIP, is placed in sys.modules -- add() stacks fp32 rows, search() takes fp32 inner
products and orders them descending with a stable sort (ties: the lower row first).  run_spar_retrieval then runs on the files
tests/_spar_fixture.py writes: 300 passages, d1 = d2 = 32, two datasets of 5 queries with weights 1 and 3, topk 20, once per pooling.
Every feature is a multiple of 1/8 in [-1, 1] (tests/_spar_oracle.grid): with these weights the pooled vectors and every inner product
are exact in fp32 in any order ((q1 + 3 q2) / 4 and (p1 + p2) / 2 included), so the recorded scores are THE scores, not one rounding of
them.  The fixture holds the inputs and, per dataset, the scores and passage rows (id - 1) of the reference's output records.

Task.  SalientPhraseAwareDenseRetrieverTask is imported from the reference tree through oracle/ref_shim.py, used as it is.  Its setup()
(two load_from_checkpoint calls of pytorch-lightning) is not run: dense_model and lexical_model are two reference DenseRetrieverTask
objects whose encoders are torch.nn.EmbeddingBag(mode='sum') tables with grid weights.  The fixture holds the four tables, the token
ids, lexical_weight and what the reference's encode_queries / encode_contexts returned.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402
import _spar_fixture as SF  # noqa: E402
import _spar_oracle as SO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
N, D, NQ, TOPK, WEIGHTS = 300, 32, 5, 20, [1.0, 3.0]


class IndexFlatIP:
    def __init__(self, d):
        self.d, self.rows = d, []

    def add(self, x):
        x = np.asarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[1] == self.d
        self.rows.append(x)

    def search(self, q, k):
        S = np.asarray(q, dtype=np.float32) @ np.concatenate(self.rows, 0).T
        assert S.dtype == np.float32
        order = np.argsort(-S, axis=1, kind="stable")[:, :k]
        return np.take_along_axis(S, order, axis=1), order


def load_reference_spar_retrieval():
    faiss = types.ModuleType("faiss")
    faiss.IndexFlatIP = IndexFlatIP
    sys.modules["faiss"] = faiss
    path = os.path.join(ref_shim.REFERENCE_ROOT, "spar", "spar_retrieval.py")
    spec = importlib.util.spec_from_file_location("reference_spar_retrieval", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def retrieval_fixtures():
    ref = load_reference_spar_retrieval()
    for seed, pooling in ((401, "concat"), (402, "sum"), (403, "mean")):
        rng = np.random.default_rng(seed)
        p1, p2 = SO.grid(rng, N, D), SO.grid(rng, N, D)
        q1s, q2s = [SO.grid(rng, NQ, D) for _ in WEIGHTS], [SO.grid(rng, NQ, D) for _ in WEIGHTS]
        with tempfile.TemporaryDirectory() as tmp:
            kw = SF.write_inputs(tmp, p1, p2, q1s, q2s)
            out = os.path.join(tmp, "out")
            ref.run_spar_retrieval(output_dir=out, weights=list(WEIGHTS), save_embeddings=False, topk=TOPK, pooling=pooling, **kw)
            results = SF.read_outputs(out, kw["output_filenames"])
        scores = np.array([[[c["score"] for c in rec["ctxs"]] for rec in recs] for recs in results], dtype=np.float64)
        rows = np.array([[[int(c["id"]) - 1 for c in rec["ctxs"]] for rec in recs] for recs in results], dtype=np.int64)
        assert scores.shape == rows.shape == (len(WEIGHTS), NQ, TOPK)
        assert np.array_equal(scores.astype(np.float32).astype(np.float64), scores)
        qids = [[rec["id"] for rec in recs] for recs in results]
        meta = dict(case=f"spar_{pooling}", pooling=pooling, seed=seed, n=N, d1=D, d2=D, nq=NQ, topk=TOPK, weights=WEIGHTS, question_ids=qids)
        path = os.path.join(OUT, f"spar_{pooling}.npz")
        np.savez_compressed(path, meta=np.array(json.dumps(meta)), p1=p1, p2=p2, q1=np.stack(q1s), q2=np.stack(q2s),
                            scores=scores.astype(np.float32), rows=rows)
        print(f"spar_{pooling}: {os.path.getsize(path) / 1024:.1f} KiB")


def task_fixture():
    ref_shim.load_reference_task_class()
    from dpr_scale.task.spar_task import SalientPhraseAwareDenseRetrieverTask  # noqa: E402  (the reference's file)

    assert os.path.realpath(sys.modules["dpr_scale.task.spar_task"].__file__).startswith(os.path.realpath(ref_shim.REFERENCE_ROOT))
    rng = np.random.default_rng(404)
    vocab, d_dense, d_lex, lexical_weight = 16, 8, 12, 2.0
    tables = {name: SO.grid(rng, vocab, d) for name, d in (("dense_q", d_dense), ("dense_c", d_dense), ("lex_q", d_lex), ("lex_c", d_lex))}
    query_ids = rng.integers(0, vocab, size=(3, 5))
    contexts_ids = rng.integers(0, vocab, size=(6, 7))

    def bag(w):
        m = torch.nn.EmbeddingBag(w.shape[0], w.shape[1], mode="sum")
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(w))
        return m

    def model(prefix):
        t = ref_shim.make_reference_task(False)
        t.query_encoder, t.context_encoder = bag(tables[prefix + "_q"]), bag(tables[prefix + "_c"])
        return t

    task = SalientPhraseAwareDenseRetrieverTask(pretrained_checkpoint_path="", lexical_model_checkpoint_path="", lexical_weight=lexical_weight,
                                                transform=None, model=None, datamodule=None, optim=None)
    task.dense_model, task.lexical_model = model("dense"), model("lex")
    with torch.no_grad():
        qr = task.encode_queries(torch.from_numpy(query_ids))
        cr = task.encode_contexts(torch.from_numpy(contexts_ids))
    assert qr.shape == (3, d_dense + d_lex) and cr.shape == (6, d_dense + d_lex)
    meta = dict(case="spar_task", vocab=vocab, d_dense=d_dense, d_lex=d_lex, lexical_weight=lexical_weight)
    path = os.path.join(OUT, "spar_task.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), query_ids=query_ids, contexts_ids=contexts_ids, query_repr=qr.numpy(),
                        context_repr=cr.numpy(), **tables)
    print(f"spar_task: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    retrieval_fixtures()
    task_fixture()
