"""SPAR retrieval without a GPU: the Python layer (dpr_scale_amd/spar.py, task/spar_task.py) on the CPU stand-in of
tests/_spar_standin.py, the oracle against the reference's own scripts (tests/golden/spar_*.npz, scripts/make_spar_golden.py), the C ABI's
host-side validation and the compiler's resource report for the new kernels."""
import ctypes
import json
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _spar_fixture as SF  # noqa: E402
import _spar_oracle as SO  # noqa: E402
from _spar_standin import SparKernels  # noqa: E402
from dpr_scale_amd import spar  # noqa: E402

POOLINGS = ["concat", "sum", "mean"]


# ---------------------------------------------------------------- oracle vs the reference ------------------------------------------------
@pytest.mark.parametrize("pooling", POOLINGS)
def test_run_spar_retrieval_reproduces_the_reference(pooling, tmp_path):
    meta, z = load_golden(f"spar_{pooling}")
    kw = SF.write_inputs(tmp_path, z["p1"], z["p2"], list(z["q1"]), list(z["q2"]))
    out = tmp_path / "out"
    spar.run_spar_retrieval(output_dir=str(out), weights=meta["weights"], topk=meta["topk"], pooling=pooling, device="cpu", kernels=SparKernels(),
                            **kw)
    results = SF.read_outputs(out, kw["output_filenames"])
    passages = spar.load_passages_tsv(kw["tsv_passages_path"])
    for s, recs in enumerate(results):
        assert [r["id"] for r in recs] == meta["question_ids"][s] and [r["question"] for r in recs] == [f"question {s}-{i}" for i in range(meta["nq"])]
        assert all(r["answers"] == [f"answer {i}"] for i, r in enumerate(recs))
        for r in recs:
            assert len(r["ctxs"]) == meta["topk"] and all(set(c) == {"id", "title", "text", "score"} for c in r["ctxs"])
            assert all(c["title"] == passages[int(c["id"]) - 1]["title"] and c["text"] == passages[int(c["id"]) - 1]["text"] for c in r["ctxs"])
        SF.same_ranking([[c["score"] for c in r["ctxs"]] for r in recs], [[int(c["id"]) - 1 for c in r["ctxs"]] for r in recs],
                     z["scores"][s], z["rows"][s])


def test_the_oracle_is_the_references_concat_score():
    meta, z = load_golden("spar_concat")
    for s, w in enumerate(meta["weights"]):
        S = SO.score(z["q1"][s], z["q2"][s], z["p1"], z["p2"], [w])[0]
        v, i = SO.topk(S.astype(np.float32), meta["topk"])
        SF.same_ranking(v, i, z["scores"][s], z["rows"][s])


def test_save_embeddings_writes_what_the_reference_writes(tmp_path):
    meta, z = load_golden("spar_concat")
    kw = SF.write_inputs(tmp_path, z["p1"], z["p2"], list(z["q1"]), list(z["q2"]))
    out = tmp_path / "out"
    spar.run_spar_retrieval(output_dir=str(out), weights=meta["weights"], topk=5, save_embeddings=True, device="cpu", kernels=SparKernels(), **kw)
    shards = [pickle.load(open(out / f"reps_000{i}.pkl", "rb")) for i in range(8)]
    assert torch.equal(torch.cat(shards), torch.from_numpy(np.concatenate([z["p1"], z["p2"]], 1)))
    assert [len(s) for s in shards] == [38] * 7 + [34]  # n // 8 + 1 rows per shard
    for s, name in enumerate(kw["query_emb_names"]):
        assert torch.equal(pickle.load(open(out / name, "rb")), torch.from_numpy(np.concatenate([z["q1"][s], meta["weights"][s] * z["q2"][s]], 1)))


# ---------------------------------------------------------------- SparIndex --------------------------------------------------------------
def _case(seed=0, n=70, nq=4, d1=24, d2=40):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(SO.grid(rng, *s)) for s in ((nq, d1), (nq, d2), (n, d1), (n, d2))]


def test_from_dirs_round_trips_through_pickles_and_pads_to_32(tmp_path):
    q1, q2, p1, p2 = _case()
    kw = SF.write_inputs(tmp_path, p1.numpy(), p2.numpy(), [q1.numpy()], [q2.numpy()])
    index = spar.SparIndex.from_dirs(kw["ctx_embeddings_dir_1"], kw["ctx_embeddings_dir_2"], "cpu", kernels=SparKernels())
    assert (index.corpus_len, index.d1, index.d2, index.dp1, index.dp2) == (70, 24, 40, 32, 64)
    assert index.c1.dtype == torch.bfloat16 and index.c1.shape == (70, 32) and index.c2.shape == (70, 64)
    assert torch.equal(index.c1[:, :24].float(), p1) and not index.c1[:, 24:].any()
    assert torch.equal(index.c2[:, :40].float(), p2) and not index.c2[:, 40:].any()
    direct = spar.SparIndex(p1, p2, "cpu", kernels=SparKernels())
    assert torch.equal(direct.c1, index.c1) and torch.equal(direct.c2, index.c2)
    v, i = index.search(q1, q2, [0.5, 2.0], 10)
    assert v.shape == (2, 4, 10) and v.dtype == torch.float32 and i.dtype == torch.int64
    tv, ti = SO.topk(SO.score(q1, q2, p1, p2, [0.5, 2.0]).astype(np.float32), 10)
    assert np.array_equal(v.numpy(), tv) and np.array_equal(i.numpy(), ti)


def test_weights_as_scalar_list_and_more_than_32():
    q1, q2, p1, p2 = _case(1)
    kn = SparKernels()
    index = spar.SparIndex(p1, p2, "cpu", kernels=kn)
    ws = [0.25 * (j + 1) for j in range(40)]
    v, i = index.search(q1, q2, ws, 7)
    assert v.shape == (40, 4, 7) and kn.calls == [("search", 32), ("search", 8)]  # groups of at most 32, one pass each
    tv, ti = SO.topk(SO.score(q1, q2, p1, p2, ws).astype(np.float32), 7)
    assert np.array_equal(v.numpy(), tv) and np.array_equal(i.numpy(), ti)
    v1, i1 = index.search(q1, q2, 0.75, 7)
    assert v1.shape == (1, 4, 7) and torch.equal(v1[0], v[2]) and torch.equal(i1[0], i[2])
    vl, il = index.search(q1, q2, [0.75], 7)
    assert torch.equal(vl, v1) and torch.equal(il, i1)
    S = index.score(q1, q2, ws, 3, 20)
    assert S.shape == (40, 4, 20) and np.array_equal(S.numpy().astype(np.float64), SO.score(q1, q2, p1[3:23], p2[3:23], ws))


def test_id_range_folds_equal_one_search():
    q1, q2, p1, p2 = _case(2)
    index = spar.SparIndex(p1, p2, "cpu", kernels=SparKernels())
    v, i = index.search(q1, q2, [0.5, 1.0, 4.0], 30)
    for ranges, chunk in (([(0, 70)], 8), ([(0, 33), (33, 70)], 16), ([(41, 70), (0, 9), (9, 41)], None)):
        v2, i2 = index.search(q1, q2, [0.5, 1.0, 4.0], 30, id_ranges=ranges, chunk=chunk)
        assert torch.equal(v, v2) and torch.equal(i, i2), ranges
    v3, i3 = index.search(q1, q2, [1.0], 30, id_ranges=[(10, 25)])  # fewer candidates than topk: the tail stays unfilled
    assert bool((i3[:, :, 15:] == -1).all()) and bool(torch.isinf(v3[:, :, 15:]).all()) and bool((i3[:, :, :15] >= 10).all())


def test_partial_scores_are_the_two_summands():
    q1, q2, p1, p2 = _case(3)
    index = spar.SparIndex(p1, p2, "cpu", kernels=SparKernels())
    ws = list(SO.GRID_LAMS)
    v, i = index.search(q1, q2, ws, 12)
    s1, s2 = index.partial_scores(q1, q2, i)
    assert s1.shape == s2.shape == v.shape
    assert torch.equal(v, s1 + torch.tensor(ws).view(-1, 1, 1) * s2)  # grid inputs: exact
    assert torch.equal(s1[0], torch.gather(q1 @ p1.T, 1, i[0]))


def test_refusals(tmp_path):
    q1, q2, p1, p2 = _case(4)
    with pytest.raises(ValueError, match="same passages"):
        spar.SparIndex(p1, p2[:-1], "cpu", kernels=SparKernels())
    index = spar.SparIndex(p1, p2, "cpu", kernels=SparKernels())
    for k in (0, 71):
        with pytest.raises(ValueError, match="topk"):
            index.search(q1, q2, 1.0, k)
    with pytest.raises(ValueError, match="do not fit"):
        index.search(q1, q2[:, :8], 1.0, 5)
    with pytest.raises(ValueError, match="no weights"):
        index.search(q1, q2, [], 5)
    kw = SF.write_inputs(tmp_path, p1.numpy(), p2.numpy(), [q1.numpy()], [q2.numpy()])
    with pytest.raises(ValueError, match="widths 24 and 40 differ"):
        spar.run_spar_retrieval(output_dir=str(tmp_path / "o"), pooling="sum", topk=5, device="cpu", kernels=SparKernels(), **kw)
    with pytest.raises(ValueError):
        spar.run_spar_retrieval(output_dir=str(tmp_path / "o"), pooling="product", topk=5, device="cpu", kernels=SparKernels(), **kw)


# ---------------------------------------------------------------- grid_search_weights ----------------------------------------------------
def test_grid_search_weights_writes_one_exact_file_per_weight(tmp_path):
    rng = np.random.default_rng(6)
    n, nq, d = 60, 3, 32
    p1, p2, q1, q2 = SO.grid(rng, n, d), SO.grid(rng, n, d), SO.grid(rng, nq, d), SO.grid(rng, nq, d)
    kw = SF.write_inputs(tmp_path, p1, p2, [q1], [q2])
    d1, d2, qname = kw["ctx_embeddings_dir_1"], kw["ctx_embeddings_dir_2"], kw["query_emb_names"][0]
    kn = SparKernels()
    spar.run_spar_retrieval(output_dir=d1, weights=[0.0], topk=10, device="cpu", kernels=kn,  # model 1's own predictions, as the reference's input
                            **{**kw, "output_filenames": ["dev.json"]})
    ws = list(SO.GRID_LAMS)
    seen = []

    def evaluate(path, ks, regex):
        seen.append((os.path.basename(path), tuple(ks), regex))
        w = float(re.match(r"weight([0-9.]+)_", os.path.basename(path)).group(1))
        return {k: [1.0 - abs(w - 2.0) / 10, 1.0] for k in ks}  # best at w = 2

    kn.calls.clear()
    out = tmp_path / "tuned"
    best = spar.grid_search_weights(d1, d2, "dev.json", qname, weights=ws, output_dir=str(out), eval_on_ks=[1, 5], valid_on_k=5,
                                    evaluate_retrieval=evaluate, topk_out=15, device="cpu", kernels=kn, tsv_passages_path=kw["tsv_passages_path"])
    assert kn.calls == [("search", len(ws))]  # ONE pass for the whole grid
    assert best[0] == 2.0 and seen == [(f"weight{w}_dev.json", (1, 5), False) for w in ws]
    assert "The best weight for dev.json is 2.0" in open(out / "dev.json.log").read()
    want = SO.score(q1, q2, p1, p2, ws)
    tv, ti = SO.topk(want.astype(np.float32), 15)
    for j, w in enumerate(ws):
        recs = json.load(open(out / f"weight{w}_dev.json"))
        assert [r["question"] for r in recs] == [f"question 0-{i}" for i in range(nq)]
        for i, r in enumerate(recs):
            assert [int(c["id"]) - 1 for c in r["ctxs"]] == ti[j, i].tolist() and [c["score"] for c in r["ctxs"]] == tv[j, i].tolist()
            for c in r["ctxs"]:
                row = int(c["id"]) - 1
                assert (c["title"], c["text"]) == (f"title {row}", f"passage text {row}")
                assert c["score"] == c["score_1"] + w * c["score_2"]  # grid inputs: exact
                assert c["score_1"] == float(q1[i].astype(np.float64) @ p1[row]) and c["score_2"] == float(q2[i].astype(np.float64) @ p2[row])
    assert spar.grid_search_weights.__defaults__[0] == [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.25, 1.43, 1.67, 2, 2.5, 3.33, 5.0, 10.0]
    assert "exact" in spar.grid_search_weights.__doc__.lower() and "joint pool" in spar.grid_search_weights.__doc__


def test_grid_search_weights_gives_every_winner_its_text(tmp_path):
    """The evaluation decides a hit by the passage text.  The exact winners of a large weight are the lexical model's finds, which lie
    outside model 1's own lists: they must come out with their text, from the corpus TSV or from model 2's prediction file, or not at
    all -- a record with an empty text would count every such find as a miss and bias the tuned weight against the lexical half."""
    rng = np.random.default_rng(8)
    n, nq, d, ws = 60, 3, 32, [0.25, 4.0]
    p1, p2, q1 = SO.grid(rng, n, d), SO.grid(rng, n, d), SO.grid(rng, nq, d)
    own = SO.topk(SO.score(q1, q1, p1, p1, [0.0])[0].astype(np.float32), n)[1]  # model 1's own ranking
    gold = [int(own[i, -1]) for i in range(nq)]  # the passage model 1 ranks last ...
    p2[gold] = np.where(p2[gold] >= 0, 1.0, -1.0).astype(np.float32)
    q2 = p2[gold].copy()  # ... is the lexical model's clear first
    top = SO.topk(SO.score(q1, q2, p1, p2, ws).astype(np.float32), 3)[1]
    assert [int(top[1, i, 0]) for i in range(nq)] == gold and all(gold[i] not in top[0, i] for i in range(nq))
    kw = SF.write_inputs(tmp_path, p1, p2, [q1], [q2])
    d1, d2, qname, kn = kw["ctx_embeddings_dir_1"], kw["ctx_embeddings_dir_2"], kw["query_emb_names"][0], SparKernels()
    spar.run_spar_retrieval(output_dir=d1, weights=[0.0], topk=5, device="cpu", kernels=kn, **{**kw, "output_filenames": ["dev.json"]})
    assert all(str(gold[i] + 1) not in [c["id"] for c in r["ctxs"]] for i, r in enumerate(json.load(open(os.path.join(d1, "dev.json")))))

    def evaluate(path, ks, regex):  # a hit: the gold passage's TEXT among the first k, as the reference's evaluation matches answers in text
        recs = json.load(open(path))
        return {k: [float(f"passage text {gold[i]}" in [c["text"] for c in r["ctxs"][:k]]) for i, r in enumerate(recs)] for k in ks}

    common = dict(weights=ws, eval_on_ks=[1], valid_on_k=1, evaluate_retrieval=evaluate, topk_out=3, device="cpu", kernels=kn)
    assert spar.grid_search_weights(d1, d2, "dev.json", qname, output_dir=str(tmp_path / "a"), tsv_passages_path=kw["tsv_passages_path"],
                                    **common) == (4.0, 1.0)
    assert "accuracy for weight 0.25 is 0.0" in open(tmp_path / "a" / "dev.json.log").read()
    with pytest.raises(LookupError, match="tsv_passages_path"):  # only model 1's lists to take texts from: refused, nothing empty written
        spar.grid_search_weights(d1, d2, "dev.json", qname, output_dir=str(tmp_path / "b"), **common)
    with pytest.raises(LookupError, match="tsv_passages_path"):
        spar.grid_search_weights(d1, d2, "dev.json", qname, output_dir=str(tmp_path / "b2"), **{**common, "evaluate_retrieval": None})
    assert not os.path.exists(tmp_path / "b" / "weight4.0_dev.json")
    # model 2's prediction file, as the reference reads it: its lists hold the lexical finds
    spar.run_spar_retrieval(output_dir=d2, weights=[64.0], topk=5, device="cpu", kernels=kn, **{**kw, "output_filenames": ["dev.json"]})
    with pytest.raises(LookupError):  # still not every winner: at weight 0.25 ranks 2 and 3 may be in neither list
        spar.grid_search_weights(d1, d2, "dev.json", qname, output_dir=str(tmp_path / "c"), **common)
    assert spar.grid_search_weights(d1, d2, "dev.json", qname, output_dir=str(tmp_path / "c1"), **{**common, "topk_out": 1}) == (4.0, 1.0)
    with pytest.raises(ValueError, match="passages"):
        short = tmp_path / "short.tsv"
        short.write_text("id\ttext\ttitle\n1\tx\ty\n")
        spar.grid_search_weights(d1, d2, "dev.json", qname, output_dir=str(tmp_path / "d"), tsv_passages_path=str(short), **common)


# ---------------------------------------------------------------- the task ---------------------------------------------------------------
def test_task_vectors_equal_the_reference_classes(tmp_path):
    from dpr_scale_amd.task.dpr_task import DenseRetrieverTask
    from dpr_scale_amd.task.spar_task import SalientPhraseAwareDenseRetrieverTask

    meta, z = load_golden("spar_task")
    paths = {}
    for name, d in (("dense", meta["d_dense"]), ("lex", meta["d_lex"])):
        conf = {"_target_": "torch.nn.EmbeddingBag", "num_embeddings": meta["vocab"], "embedding_dim": d, "mode": "sum"}
        state = {"query_encoder.weight": torch.from_numpy(z[name + "_q"]), "context_encoder.weight": torch.from_numpy(z[name + "_c"])}
        paths[name] = str(tmp_path / f"{name}.ckpt")
        torch.save({"state_dict": state, "hyper_parameters": dict(transform=None, model=conf, datamodule=None, optim=None, shared_model=False)},
                   paths[name])
    task = SalientPhraseAwareDenseRetrieverTask(pretrained_checkpoint_path=paths["dense"], lexical_model_checkpoint_path=paths["lex"],
                                                lexical_weight=meta["lexical_weight"], transform=None, model=None, datamodule=None, optim=None)
    task.setup("fit")
    assert isinstance(task.dense_model, DenseRetrieverTask) and isinstance(task.lexical_model, DenseRetrieverTask) and task.setup_done
    with torch.no_grad():
        qr = task.encode_queries(torch.from_numpy(z["query_ids"]))
        cr = task.encode_contexts(torch.from_numpy(z["contexts_ids"]))
    assert np.array_equal(qr.numpy(), z["query_repr"]) and np.array_equal(cr.numpy(), z["context_repr"])
    kept = task.dense_model
    task.setup("test")  # a second setup for the test stage keeps the restored models
    assert task.dense_model is kept


# ---------------------------------------------------------------- ABI --------------------------------------------------------------------
_ONE = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch
_LAM2 = (ctypes.c_float * 2)(0.5, 2.0)
_GOOD = dict(Q1=_ONE, Q2=_ONE, nq=2, d1=32, d2=64, C1=_ONE, C2=_ONE, n=100, lam=_LAM2, W=2, b=0, e=100, k=5, chunk=64, vals=_ONE, idx=_ONE, first=1,
             ws=_ONE, wsb=1 << 20, st=None)
_BAD = [  # (what is wrong, code, a word of the error text)
    (dict(Q1=None), -1, b"NULL"), (dict(C2=None), -1, b"NULL"), (dict(lam=None), -1, b"NULL"), (dict(vals=None), -1, b"NULL"),
    (dict(idx=None), -1, b"NULL"),
    (dict(Q2=ctypes.c_void_p(264)), -1, b"aligned"), (dict(C1=ctypes.c_void_p(260)), -1, b"aligned"), (dict(ws=ctypes.c_void_p(264)), -1, b"aligned"),
    (dict(d1=48), -1, b"multiples of 32"), (dict(d2=0), -1, b"multiples of 32"),
    (dict(W=0), -1, b"weights"), (dict(W=33, lam=(ctypes.c_float * 33)()), -1, b"weights"),
    (dict(lam=(ctypes.c_float * 2)(1.0, float("inf"))), -1, b"finite"), (dict(lam=(ctypes.c_float * 2)(float("nan"), 1.0)), -1, b"finite"),
    (dict(nq=0), -1, b"state rows"), (dict(nq=1 << 30), -1, b"state rows"),
    (dict(nq=1 << 20, W=2, chunk=1 << 20), -1, b"candidate slots"),
    (dict(n=0), -1, b"n_ctx"), (dict(n=1 << 31, e=1 << 31), -1, b"n_ctx"),
    (dict(k=0), -1, b"topk"), (dict(k=101), -1, b"topk"),
    (dict(b=50, e=40), -1, b"range"), (dict(b=7, e=7), -1, b"range"), (dict(e=101), -1, b"range"), (dict(b=-1), -1, b"range"),
    (dict(chunk=12), -1, b"chunk"), (dict(chunk=0), -1, b"chunk"),
    (dict(ws=None), -4, b"workspace"), (dict(wsb=16), -4, b"workspace"),
    (dict(n=6000, e=6000, k=5000, wsb=4 * 64 * 8 + 256), -4, b"workspace"),  # k > 4096: the wide selection's state is missing
]


def test_abi_exports_binds_and_validates_on_the_host():
    from dpr_scale_amd import _lib

    lib = _lib.lib
    for s in ("dprhot_spar_workspace_bytes", "dprhot_spar_score", "dprhot_spar_search"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert _lib.spar_workspace_bytes(2, 2, 64) == 4 * 64 * 8 + 256 == _lib.search_workspace_bytes(4, 64)
    out = ctypes.c_size_t(0)
    for args, word in (((2, 0, 64), b"weights"), ((2, 33, 64), b"weights"), ((0, 1, 64), b"state rows"), ((2, 2, 12), b"chunk")):
        assert lib.dprhot_spar_workspace_bytes(*args, ctypes.byref(out)) == -1 and word in lib.dprhot_last_error(), args
    for bad, code, word in _BAD:
        assert set(bad) <= set(_GOOD), bad
        rc = lib.dprhot_spar_search(*[bad.get(k, v) for k, v in _GOOD.items()])
        err = lib.dprhot_last_error()
        assert rc == code and word in err, (bad, rc, err)
        if code == -4:
            assert b"spar_search needs" in err and b"dprhot_spar_workspace_bytes" in err, err
            assert (b"dprhot_topk_wide_workspace_bytes" in err) == ("k" in bad), err
    S = dict(Q1=_ONE, Q2=_ONE, nq=2, d1=32, d2=64, C1=_ONE, C2=_ONE, n=100, lam=_LAM2, W=2, db=0, cols=10, S=_ONE, ld=16, st=None)
    for bad, word in ((dict(S=None), b"NULL"), (dict(cols=0), b"cols"), (dict(ld=8), b"ld"), (dict(ld=12), b"multiple of 8"), (dict(db=95), b"corpus"),
                      (dict(S=ctypes.c_void_p(260)), b"aligned"), (dict(d1=40), b"multiples of 32")):
        rc = lib.dprhot_spar_score(*[bad.get(k, v) for k, v in S.items()])
        assert rc == -1 and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())


# ---------------------------------------------------------------- resources --------------------------------------------------------------
def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    report = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
    assert os.path.isfile(report), "the library's Makefile writes the compiler's resource report next to it"
    cur, rows = None, {}
    for ln in open(report, errors="replace"):
        m = re.search(r" Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)", ln)
        if m and cur:
            rows[cur][m.group(1)] = int(m.group(2))
    mine = {k: v for k, v in rows.items() if "11spar_kernel" in k}
    assert len(mine) == 2, sorted(mine)  # the store and the filter epilogue
    for name, r in mine.items():
        assert r == {"ScratchSize [bytes/lane]": 0, "SGPRs Spill": 0, "VGPRs Spill": 0}, (name, r)
