"""Inverted-index retrieval for CITADEL / COIL on the CPU: the fp64 oracle against the fixtures the reference's tasks produced
(scripts/make_ivf_golden.py), the index loader and the query packer, IVFIndex.search and the drop-in CITADELRetrievalTask driven
through the test-only stand-in kernels, the ABI surface and the compiler's resource report of the new kernel."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ivf_fixture as F  # noqa: E402
import _ivf_oracle as O  # noqa: E402
from _ivf_standin import IvfKernels  # noqa: E402
from dpr_scale_amd import ivf  # noqa: E402

REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")


@pytest.mark.parametrize("name", F.NAMES)
def test_oracle_reproduces_the_reference(name):
    meta, z = F.load(name)
    cls_q, emb, _ = F.queries(meta, z)
    for bf16 in (False, True):  # grid inputs: the bf16 rounding changes nothing
        S = O.score_matrix(F.postings(z), emb, meta["corpus_len"], cls_q if len(cls_q) else None, z.get("cls_doc"), bf16=bf16)
        assert np.array_equal(S.astype(np.float32), z["scores"])
        v, i = O.topk(S, meta["topk"])
        assert np.array_equal(v.astype(np.float32), z["top_scores"]) and np.array_equal(i, z["top_ids"])


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("name", ["ivf_coil_cls", "ivf_citadel23", "ivf_citadel23_cls"])
def test_load_index_layout(name, splits, tmp_path):
    meta, z = F.load(name)
    index = ivf.load_index(F.write_tree(str(tmp_path), z, splits), meta["corpus_len"], "cpu", kernels=IvfKernels())
    # expected: (expert, doc) order, file order kept inside a doc (the fixture's arrays are in file order per expert)
    order = np.lexsort((np.arange(len(z["post_doc"])), z["post_doc"], z["post_expert"]))
    assert np.array_equal(index.post_doc.numpy(), z["post_doc"][order].astype(np.int32))
    assert np.array_equal(index.post_vec[:, : meta["d"]].float().numpy(), z["post_vec"][order])
    assert index.dp % 32 == 0 and not index.post_vec[:, meta["d"]:].float().any()
    counts = np.bincount(z["post_expert"], minlength=index.n_experts)
    assert np.array_equal(index.exp_off.numpy(), np.concatenate([[0], np.cumsum(counts)]))
    assert index.exp_off.dtype == torch.int64 and index.post_doc.dtype == torch.int32 and index.post_vec.dtype == torch.bfloat16
    if "cls_doc" in z:
        assert np.array_equal(index.cls[: meta["corpus_len"], : z["cls_doc"].shape[1]].float().numpy(), z["cls_doc"])
        assert index.cls.shape[0] >= meta["corpus_len"] + 7 and not index.cls[meta["corpus_len"]:].float().any()
    else:
        assert index.cls is None
    assert "encode_time" in index.latency


def test_load_index_refuses_ids_that_are_not_cls_rows(tmp_path):
    meta, z = F.load("ivf_coil_cls")
    root = F.write_tree(str(tmp_path / "a"), z, 2)
    for a, b in (("expert_0000", "x"), ("expert_0001", "expert_0000"), ("x", "expert_0001")):  # rank 0's files now name rank 1's rows
        os.rename(os.path.join(root, a), os.path.join(root, b))
    with pytest.raises(ValueError, match="doc ids outside"):
        ivf.load_index(root, meta["corpus_len"], "cpu", kernels=IvfKernels())
    meta, z = F.load("ivf_coil_cls")
    with pytest.raises(ValueError, match="CLS files hold"):
        ivf.load_index(F.write_tree(str(tmp_path / "b"), z, 1), meta["corpus_len"] + 1, "cpu", kernels=IvfKernels())


def test_pack_queries_order_and_single_rounding():
    meta, z = F.load("ivf_citadel23")
    cls_q, emb, wts = F.queries(meta, z)
    qb = ivf.pack_queries(cls_q, emb, wts)
    # expected order: (expert, query, listed order)
    order = np.lexsort((np.arange(len(z["ent_query"])), z["ent_query"], z["ent_expert"]))
    assert np.array_equal(qb.ent_q.numpy(), z["ent_query"][order].astype(np.int32))
    assert np.array_equal(qb.ent_vec[:, : meta["d"]].float().numpy(), z["ent_vec"][order])
    ex = z["ent_expert"][order]
    assert np.array_equal(qb.bexp.numpy(), np.unique(ex))
    assert np.array_equal(qb.boff.numpy(), np.concatenate([np.searchsorted(ex, np.unique(ex)), [len(ex)]]))
    # fp16 and fp32 inputs of equal value give the same bf16 entries, also where fp16 -> bf16 rounds: the only rounding is the last
    g = np.random.default_rng(5)
    h = torch.from_numpy(g.standard_normal((6, 32)).astype(np.float32)).to(torch.float16)
    a = ivf.pack_queries([], [{3: [h[0], h[1]], 1: [h[2]]}, {1: [h[3], h[4]], 7: [h[5]]}], None)
    b = ivf.pack_queries([], [{3: [h[0].float(), h[1].float()], 1: [h[2].float()]}, {1: [h[3].float(), h[4].float()], 7: [h[5].float()]}], None)
    assert torch.equal(a.ent_vec.view(torch.int16), b.ent_vec.view(torch.int16)) and torch.equal(a.ent_q, b.ent_q)
    assert torch.equal(a.ent_vec, h[[2, 3, 4, 0, 1, 5]].float().to(torch.bfloat16))
    assert a.ent_q.tolist() == [0, 1, 1, 0, 0, 1] and a.bexp.tolist() == [1, 3, 7] and a.boff.tolist() == [0, 3, 5, 6]
    with pytest.raises(ValueError, match="at most 4096"):
        ivf.pack_queries([], [{0: [h[0]] * 4097}], None)
    empty = ivf.pack_queries([], [{}], None, d=20)
    assert empty.n_entries == 0 and empty.ent_vec.shape == (0, 32)


@pytest.mark.parametrize("name", F.NAMES)
def test_search_through_the_standin(name, tmp_path):
    meta, z = F.load(name)
    kn = IvfKernels()
    index = ivf.load_index(F.write_tree(str(tmp_path), z, 2), meta["corpus_len"], "cpu", kernels=kn)
    cls_q, emb, wts = F.queries(meta, z)
    v, i = index.search(cls_q, emb, wts, meta["topk"], chunk=8)
    assert v.dtype == torch.float32 and i.dtype == torch.int64
    assert np.array_equal(v.numpy(), z["top_scores"]) and np.array_equal(i.numpy(), z["top_ids"])
    assert kn.calls == [(0, 8), (8, 16), (16, 20)]
    # disjoint doc-id ranges, in any order, fold into the same result
    v2, i2 = index.search(cls_q, emb, wts, meta["topk"], id_ranges=[(13, 20), (0, 5), (5, 13)], chunk=16)
    assert torch.equal(v, v2) and torch.equal(i, i2)
    with pytest.raises(ValueError, match="topk"):
        index.search(cls_q, emb, wts, meta["corpus_len"] + 1)
    assert index.latency["encode_time"] > 0


def _toy_task(meta, z, tmp_path, **kw):
    from dpr_scale_amd.task.citadel_retrieval import CITADELRetrievalTask

    task = CITADELRetrievalTask(ctx_embeddings_dir=str(tmp_path), checkpoint_path="", topk=meta["topk"], transform=None, model=None,
                                datamodule=None, optim=None, **kw)
    return task


@pytest.mark.parametrize("name", ["ivf_coil_cls", "ivf_citadel23", "ivf_citadel23_cls"])
def test_dropin_eval_step_and_trec_lines(name, tmp_path):
    """The drop-in's _eval_step on an encoder stand-in that returns repr tensors rebuilt from the fixture's entries: one token per
    entry (CITADEL: the entry is weight * repr with weight 1 in slot 0, the other slots weight 0)."""
    meta, z = F.load(name)
    task = _toy_task(meta, z, tmp_path)
    task.index = ivf.load_index(F.write_tree(str(tmp_path), z, 1), meta["corpus_len"], "cpu", kernels=IvfKernels())
    nq, L = meta["nq"], int(np.bincount(z["ent_query"]).max()) + 1
    coil = meta["kind"] == "coil"
    K = 1 if coil else 2
    repr_ = torch.zeros(nq, L, meta["d"])
    ids = torch.zeros((nq, L) if coil else (nq, L, K), dtype=torch.long)
    wts = torch.zeros((nq, L) if coil else (nq, L, K))
    att = torch.zeros(nq, L, dtype=torch.long)
    fill = [0] * nq
    for n, e, v in zip(z["ent_query"], z["ent_expert"], z["ent_vec"]):
        j = fill[n]
        fill[n] += 1
        repr_[n, j], att[n, j] = torch.from_numpy(v), 1
        if coil:
            ids[n, j], wts[n, j] = int(e), 1.0
        else:
            ids[n, j, 0], wts[n, j, 0] = int(e), 1.0
    out = {"expert_repr": repr_, "expert_ids": ids, "expert_weights": wts, "attention_mask": att}
    if "cls_q" in z:
        out["cls_repr"] = torch.from_numpy(z["cls_q"])

    class Enc(torch.nn.Module):
        def forward(self, token_ids, **kw):
            return dict(out)

    task.query_encoder = Enc()
    scores, top_ids, topics, questions, answers = task._eval_step(
        {"query_ids": {"input_ids": torch.zeros((nq, L), dtype=torch.long)}, "topic_ids": meta["topics"]}, 0)
    assert np.array_equal(np.array(scores, np.float32), z["top_scores"]) and np.array_equal(np.array(top_ids), z["top_ids"])
    assert task.merge_trec_results(topics, top_ids, scores) == meta["trec"]
    assert task.latency["encode_time"] > 0


def test_dropin_scope_and_signature():
    from dpr_scale_amd.task.citadel_retrieval import CITADELRetrievalTask

    base = dict(ctx_embeddings_dir="x", checkpoint_path="", transform=None, model=None, datamodule=None, optim=None)
    with pytest.raises(NotImplementedError, match="product quantisation"):
        CITADELRetrievalTask(quantizer="pq", **base)
    with pytest.raises(NotImplementedError, match="cuda=False"):
        CITADELRetrievalTask(cuda=False, **base)
    assert CITADELRetrievalTask(quantizer="None", **base).quantizer is None
    for m in ("setup", "forward", "_eval_step", "test_step", "test_epoch_end", "merge_trec_results", "merge_qa_results"):
        assert callable(getattr(CITADELRetrievalTask, m))


def test_dropin_signature_matches_reference():
    from oracle import ref_shim

    if not ref_shim.reference_available():
        pytest.skip("reference tree not present")
    import ast

    from dpr_scale_amd.task.citadel_retrieval import CITADELRetrievalTask

    # the reference module cannot be imported (it imports an index module it does not ship): read its constructor from the source
    src = open(os.path.join(ref_shim.REFERENCE_ROOT, "dpr_scale", "task", "citadel_retrieval_task.py")).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "CITADELRetrievalTask")
    init = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    names = [a.arg for a in init.args.args if a.arg != "self"]
    defaults = [ast.literal_eval(d) for d in init.args.defaults]
    sig = inspect.signature(CITADELRetrievalTask.__init__).parameters
    assert [p for p in sig if p not in ("self", "kwargs")] == names
    want = dict(zip(names[len(names) - len(defaults):], defaults))
    assert {k: sig[k].default for k in want} == want


def test_abi_surface_and_host_validation():
    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import HipKernels

    assert _lib.version() == 174
    for s in ("dprhot_ivf_workspace_bytes", "dprhot_ivf_score", "dprhot_ivf_search"):
        assert hasattr(_lib.lib, s) and s in _lib.SIGNATURES
    assert callable(HipKernels.ivf_score) and callable(HipKernels.ivf_search)
    lib, out = _lib.lib, ctypes.c_size_t(0)
    assert lib.dprhot_ivf_workspace_bytes(32, 1024, 65536, 1, ctypes.byref(out)) == 0 and 32 * 65536 * 4 <= out.value < 32 * 65536 * 4 + 256
    assert lib.dprhot_ivf_workspace_bytes(32, 1024, 65530, 1, ctypes.byref(out)) == -1  # chunk % 8
    assert lib.dprhot_ivf_workspace_bytes(2, 2 * 4096 + 1, 64, 0, ctypes.byref(out)) == -1 and b"4096" in lib.dprhot_last_error()
    one = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch
    args = lambda **kw: [kw.get(k, v) for k, v in dict(
        pv=one, pd=one, eo=one, P=10, V=4, dp=32, ev=one, eq=one, ne=2, be=one, bo=one, nb=1, nq=1, cq=None, cd=None, dc=0, cr=0,
        n=100, b=0, e=100, k=5, chunk=64, vals=one, idx=one, first=1, ws=one, wsb=1 << 20, st=None).items()]
    assert lib.dprhot_ivf_search(*args(n=2 ** 31)) == -1 and b"corpus_len" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_search(*args(P=2 ** 40)) == -1 and b"2^40" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_search(*args(k=0)) == -1 and lib.dprhot_ivf_search(*args(k=101)) == -1 and b"topk" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_search(*args(ne=4097, nb=1)) == -1 and b"entries per query" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_search(*args(dp=20)) == -1 and lib.dprhot_ivf_search(*args(chunk=12)) == -1
    assert lib.dprhot_ivf_search(*args(b=50, e=40)) == -1 and lib.dprhot_ivf_search(*args(e=101)) == -1
    assert lib.dprhot_ivf_search(*args(cq=one, cd=one, dc=16, cr=100)) == -1 and b"cls_doc" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_search(*args(wsb=16)) == -4  # workspace too small
    assert lib.dprhot_ivf_search(*args(k=5000, n=6000, e=6000, wsb=6000 * 4)) == -4  # k > 4096 needs the wide selection's state too
    assert lib.dprhot_ivf_score(one, one, one, 10, 4, 32, one, one, 2, one, one, 1, 1, 2 ** 31 - 10, 64, one, 64, None) == -1


def test_ivf_kernels_never_spill():
    cur, rows = None, {}
    for ln in open(REPORT, errors="replace"):
        m = re.search(r" Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", ln)
        if m and cur:
            rows[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    mine = {k: v for k, v in rows.items() if re.search(r"dprhot\d+ivf_\w+_kernel", k)}
    assert len(mine) >= 1, sorted(rows)
    for name, r in mine.items():
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
