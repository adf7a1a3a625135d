"""ColBERT search with centroid pruning on the CPU: host-side validation of dprhot_colbert_cand_*, and
ColBERTIndex.build_centroids / probe / candidates / score_candidates / search_pruned / save_centroids / load_centroids and the task
driven through the test-only stand-in (tests/_colbert_cand_standin.py).  Tokens, queries and the given centroids lie on a grid of
multiples of 1/4, so every score is exact in fp32 and in float64 alike: assignment, probing, lists, unions and the pruned top-k are
compared with exact equality."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _colbert_cand_standin as CS  # noqa: E402
import _colbert_oracle as CO  # noqa: E402
from dpr_scale_amd import colbert  # noqa: E402

REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
_BASE = dict(transform=None, model=None, datamodule=None, optim=None)
NQ, LQ, N, LD, D, C = 4, 6, 30, 40, 20, 16


def grid_index(seed=3, **kw):
    """(index with given grid centroids, q, passages, centroids)"""
    lengths = np.random.default_rng(seed).permutation(np.resize(np.array([0, 1, 5, 15, 16, 17, 31, 33, 39]), N))
    q, c, att = CO.make_padded(seed, NQ, LQ, N, LD, D, lengths=lengths, q_pad=2)
    index = colbert.ColBERTIndex.from_repr(c, att, list(range(N)), N, "cpu", kernels=CS.ColbertCandKernels(), **kw)
    cen = torch.from_numpy(np.random.default_rng(seed + 1).integers(-4, 5, size=(C, D)).astype(np.float32) / 4.0)
    cen[5] = cen[2]  # two equal centroids: every tie between them goes to the lower id
    index.build_centroids(C, centroids=cen)
    return index, q, CO.passages_of(c, att), cen


def top_ids(scores64, k):
    """int64 [rows, k]: the k best columns, score descending, ties to the lower id."""
    return torch.sort(scores64, dim=1, descending=True, stable=True).indices[:, :k]


_ONE = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch


def test_host_side_validation_of_the_three_entry_points():
    from dpr_scale_amd import _lib

    lib = _lib.lib
    out = ctypes.c_size_t(0)
    ws_bytes = lib.dprhot_colbert_cand_workspace_bytes
    assert ws_bytes(2, 64, ctypes.byref(out)) == 0 and out.value >= 2 * 64 * 4
    assert ws_bytes(2, 64, None) == -1 and ws_bytes(0, 64, ctypes.byref(out)) == -1
    assert ws_bytes(2, 0, ctypes.byref(out)) == -1 and ws_bytes(2, 12, ctypes.byref(out)) == -1

    head = dict(tok=_ONE, blk=_ONE, nb=10, n=100, dp=32, q=_ONE, nq=2, LQ=5, pool=0, off=_ONE, doc=_ONE, nc=50)
    good_score = dict(head, b=0, cols=8, S=_ONE, ld=8, st=None)
    score = lambda **bad: lib.dprhot_colbert_cand_score(*{**good_score, **bad}.values())
    for bad in (dict(S=None), dict(dp=40), dict(LQ=0), dict(LQ=513), dict(off=None), dict(doc=None), dict(nc=-1), dict(nc=2 ** 40),
                dict(cols=0), dict(ld=7), dict(b=-1), dict(pool=7), dict(n=0), dict(nq=0), dict(q=None)):
        assert score(**bad) == -1, (bad, lib.dprhot_last_error())
    assert score(dp=800) == -3

    good = dict(head, mc=40, k=5, chunk=64, vals=_ONE, idx=_ONE, ws=_ONE, wsb=1 << 20, st=None)
    search = lambda **bad: lib.dprhot_colbert_cand_search(*{**good, **bad}.values())
    for bad, word in ((dict(vals=None), b"NULL"), (dict(idx=None), b"NULL"), (dict(chunk=0), b"chunk"), (dict(chunk=12), b"chunk"),
                      (dict(k=0), b"topk"), (dict(k=101), b"topk"), (dict(mc=0), b"max_count"), (dict(dp=40), b"dp="),
                      (dict(LQ=0), b"LQ="), (dict(LQ=513), b"LQ="), (dict(nc=2 ** 40), b"n_cand"), (dict(off=None), b"NULL")):
        assert search(**bad) == -1 and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())
    for bad in (dict(ws=None), dict(wsb=16)):
        assert search(**bad) == -4
        err = lib.dprhot_last_error()
        assert b"colbert_cand_search needs" in err and b"dprhot_colbert_cand_workspace_bytes" in err and b"topk_wide" not in err, err
    assert search(n=6000, mc=6000, k=5000, wsb=2 * 64 * 4) == -4  # k > 4096: the wide selection's state is missing
    err = lib.dprhot_last_error()
    assert b"dprhot_colbert_cand_workspace_bytes + dprhot_topk_wide_workspace_bytes" in err, err


def test_version_stays_and_the_symbols_are_bound():
    from dpr_scale_amd import _lib

    assert _lib.version() == 174
    for s in ("dprhot_colbert_cand_workspace_bytes", "dprhot_colbert_cand_score", "dprhot_colbert_cand_search"):
        assert s in _lib.SIGNATURES and hasattr(_lib.lib, s)
    assert _lib.colbert_cand_workspace_bytes(3, 16) == _lib.colbert_workspace_bytes(3, 16)


def test_assignment_and_probe_are_the_exact_argmax_with_ties_to_the_lower_id():
    index, q, passages, cen = grid_index()
    assert index.centroids.dtype == torch.bfloat16 and index.centroids.shape == (C, index.dp)
    assert torch.equal(index.centroids[:, :D].float(), cen) and not index.centroids[:, D:].any()
    assert index.tok_centroid.dtype == torch.int32 and index.tok_centroid.shape == (index.n_blk * 16,)
    real = colbert._real_rows(index.blk_rows)
    assert int(real.sum()) == sum(p.shape[0] for p in passages) and bool((index.tok_centroid[~real] == -1).all())
    want = top_ids(index.tok[real].double() @ index.centroids.double().T, 1)[:, 0]
    assert torch.equal(index.tok_centroid[real].long(), want)
    assert not bool((index.tok_centroid == 5).any())  # centroid 5 equals centroid 2: the lower id takes every tie
    for nprobe in (1, 3, C):
        got = index.probe(q, nprobe)
        assert got.dtype == torch.int64 and got.shape == (NQ, LQ, nprobe)
        scores = CO.bf16(q).reshape(NQ * LQ, D) @ cen.double().T
        assert torch.equal(got.reshape(NQ * LQ, nprobe), top_ids(scores, nprobe))
    assert torch.equal(index.probe({"expert_repr": q}, 2), index.probe(q, 2))
    for bad in (0, C + 1):
        with pytest.raises(ValueError, match="nprobe"):
            index.probe(q, bad)


def test_inverted_lists_equal_the_lists_derived_on_the_host():
    index, _, passages, _ = grid_index()
    assert index.cen_off.dtype == torch.int64 and index.cen_off.shape == (C + 1,) and index.cen_doc.dtype == torch.int32
    off, docs = CS.lists_from_assignment(index.tok_centroid, index.doc_blk, C)
    assert index.cen_off.tolist() == off and index.cen_doc.tolist() == docs
    assert sorted(set(docs)) == [j for j, p in enumerate(passages) if p.shape[0]]  # every passage with a token is listed somewhere
    plain = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, N, D, kernels=CS.ColbertCandKernels())
    held = sum(t.numel() * t.element_size() for t in (index.centroids, index.tok_centroid, index.cen_off, index.cen_doc))
    assert index.nbytes == plain.nbytes + held
    with pytest.raises(ValueError, match="no centroids"):
        plain.candidates(torch.zeros(1, 2, D), 1)
    with pytest.raises(ValueError, match="centroids"):
        plain.build_centroids(C, centroids=torch.zeros(C + 1, D))


def test_candidates_are_the_union_of_the_probed_lists():
    index, q, passages, _ = grid_index()
    live = (q != 0).any(2)
    assert not bool(live[0, LQ - 2:].any()) and bool(live[1:].all())  # the padded tokens of query 0 are dropped from the union
    for nprobe in (1, 2, C):
        cand_off, cand_doc = index.candidates(q, nprobe)
        assert cand_off.dtype == torch.int64 and cand_off.shape == (NQ + 1,) and cand_doc.dtype == torch.int32
        off, docs = CS.union_of_lists(index.probe(q, nprobe), live, index.cen_off.tolist(), index.cen_doc.tolist())
        assert cand_off.tolist() == off and cand_doc.tolist() == docs
        for n in range(NQ):
            mine = docs[off[n]:off[n + 1]]
            assert mine == sorted(set(mine)) and all(0 <= j < N for j in mine)
            if nprobe == C:
                assert mine == [j for j, p in enumerate(passages) if p.shape[0]]
    # a query of padding only has no candidate
    cand_off, cand_doc = index.candidates(torch.zeros(2, 3, D), 2)
    assert cand_off.tolist() == [0, 0, 0] and cand_doc.numel() == 0
    v, i = index.search_pruned(torch.zeros(2, 3, D), 4, 2)
    assert bool((v == float("-inf")).all()) and bool((i == -1).all())


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_search_pruned_is_the_exhaustive_top_k_restricted_to_the_candidates(pool):
    index, q, passages, _ = grid_index(chunk=8)
    full = CO.score(q, passages, pool)
    for nprobe, k in ((1, 3), (2, 5), (2, N), (C, 7)):
        cand_off, cand_doc = index.candidates(q, nprobe)
        S = index.score_candidates(q, cand_off, cand_doc, pool)
        counts = (cand_off[1:] - cand_off[:-1]).tolist()
        assert S.shape == (NQ, max(counts)) and S.dtype == torch.float32
        v, i = index.search_pruned(q, k, nprobe, query_pool=pool)
        assert v.shape == (NQ, k) and v.dtype == torch.float32 and i.dtype == torch.int64
        for n in range(NQ):
            mine = cand_doc[cand_off[n]:cand_off[n + 1]].long()
            assert torch.equal(S[n, :counts[n]].double(), full[n, mine]) and bool(torch.isnan(S[n, counts[n]:]).all())
            tv, ti = CO.topk(full[n:n + 1, mine], k)  # sorted ids: ties to the lower position are ties to the lower doc id
            m = min(k, counts[n])
            assert torch.equal(v[n, :m].double(), tv[0]) and torch.equal(i[n, :m], mine[ti[0]]), (nprobe, k, n)
            assert bool((v[n, m:] == float("-inf")).all()) and bool((i[n, m:] == -1).all())
        if nprobe == C:  # every passage with a token is a candidate: the exhaustive search wherever only positive scores are returned
            ev, ei = index.search(q, k, query_pool=pool)
            rows = (ev > 0).all(1)
            assert bool(rows.any()) and torch.equal(v[rows], ev[rows]) and torch.equal(i[rows], ei[rows])
    assert set(index.latency) >= {"encode_time", "candidate_time", "search_time"} and index.latency["candidate_time"] > 0
    for bad in (0, N + 1):
        with pytest.raises(ValueError, match="topk"):
            index.search_pruned(q, bad, 2)
    with pytest.raises(NotImplementedError, match="pooling"):
        index.search_pruned(q, 3, 2, query_pool="mean")


def test_standin_takes_any_list_as_the_kernel_documents():
    """Unsorted lists with a duplicate, an id outside the corpus and offsets that run backwards: position order decides ties, an
    outside id is no candidate, an end below its begin is an empty list."""
    index, q, passages, _ = grid_index()
    full = CO.score(q, passages, "sum")
    cand_doc = torch.tensor([7, 3, 3, N, -1, 12, 0], dtype=torch.int32)
    cand_off = torch.tensor([0, 6, 4, 99, 7], dtype=torch.int64)  # query 0: 6 entries; 1: empty (4 < 6); 2: entries 4 .. 7; 3: empty
    S = index.score_candidates(q, cand_off, cand_doc)
    assert S.shape == (NQ, 6) and torch.equal(S[0, :3].double(), full[0, [7, 3, 3]]) and bool(torch.isnan(S[0, 3:5]).all())
    assert float(S[0, 5]) == float(full[0, 12]) and bool(torch.isnan(S[1]).all()) and bool(torch.isnan(S[3]).all())
    assert bool(torch.isnan(S[2, 0])) and torch.equal(S[2, 1:3].double(), full[2, [12, 0]]) and bool(torch.isnan(S[2, 3:]).all())
    v, i = index._search_candidates(index._queries(q), 0, 5, cand_off, cand_doc, 6)
    pos = torch.tensor([0, 1, 2, 5])  # query 0's candidates by position; a stable sort keeps the lower position first among equals
    order = pos[torch.sort(S[0, pos], descending=True, stable=True).indices]
    assert i[0].tolist() == cand_doc[order].tolist() + [-1] and v[0].tolist() == S[0, order].tolist() + [float("-inf")]
    assert i[1].tolist() == [-1] * 5 and sorted(i[2].tolist()) == [-1, -1, -1, 0, 12] and i[3].tolist() == [-1] * 5


def test_save_and_load_round_trip_to_identical_results(tmp_path):
    index, q, _, _ = grid_index()
    path = index.save_centroids(str(tmp_path / "centroids.pkl"))
    import pickle

    blob = pickle.load(open(path, "rb"))
    assert isinstance(blob, tuple) and len(blob) == 4 and blob[0].dtype == torch.bfloat16 and blob[1].dtype == torch.int32
    other = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, N, D, kernels=CS.ColbertCandKernels())
    assert other.load_centroids(path) is other
    for a, b in zip((index.centroids, index.tok_centroid, index.cen_off, index.cen_doc),
                    (other.centroids, other.tok_centroid, other.cen_off, other.cen_doc)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert torch.equal(index.probe(q, 3), other.probe(q, 3))
    for x, y in zip(index.search_pruned(q, 6, 2), other.search_pruned(q, 6, 2)):
        assert torch.equal(x, y)
    smaller = colbert.ColBERTIndex.from_packed(index.tok[:-16].contiguous(), index.doc_blk.clamp(max=index.n_blk - 1), N, D)
    with pytest.raises(ValueError, match="do not belong"):
        smaller.load_centroids(path)
    with pytest.raises(ValueError, match="no centroids"):
        smaller.save_centroids(str(tmp_path / "none.pkl"))


def test_trained_centroids_are_unit_norm_seeded_and_cover_every_token():
    index, q, passages, _ = grid_index()
    a = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, N, D, kernels=CS.ColbertCandKernels()).build_centroids(8, iters=3, seed=1)
    b = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, N, D, kernels=CS.ColbertCandKernels()).build_centroids(8, iters=3, seed=1)
    assert a.centroids.shape == (8, index.dp) and torch.equal(a.centroids, b.centroids) and torch.equal(a.tok_centroid, b.tok_centroid)
    assert bool(((a.centroids.float().norm(dim=1) - 1).abs() < 2 ** -7).all())  # unit norm, rounded to bf16 once
    real = colbert._real_rows(a.blk_rows)
    want = top_ids(a.tok[real].double() @ a.centroids.double().T, 1)[:, 0]
    assert torch.equal(a.tok_centroid[real].long(), want)
    other = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, N, D, kernels=CS.ColbertCandKernels()).build_centroids(8, iters=3, seed=2)
    assert not torch.equal(a.centroids, other.centroids)
    # more centroids than distinct directions: empty clusters are re-seeded from the sample, never left as zero rows
    rows = torch.cat([torch.eye(32)[:2].repeat(20, 1), torch.eye(32)[2:12]]).to(torch.bfloat16)
    cen = colbert.train_centroids(rows, 12, iters=4, seed=0, kernels=CS.ColbertCandKernels())
    assert cen.shape == (12, 32) and bool((cen.float().norm(dim=1) > 0.99).all())
    with pytest.raises(ValueError, match="n_centroids"):
        a.build_centroids(10 ** 6)
    v, i = a.search_pruned(q, 5, 8)
    ev, ei = a.search(q, 5)
    rows = (ev > 0).all(1)
    assert bool(rows.any()) and torch.equal(v[rows], ev[rows]) and torch.equal(i[rows], ei[rows])


def test_the_task_prunes_only_with_both_knobs_set(tmp_path):
    from dpr_scale_amd.task.citadel_retrieval import CITADELRetrievalTask
    from dpr_scale_amd.task.colbert_retrieval import ColBERTPQRetrievalTask, ColBERTPrunedRetrievalTask, ColBERTRetrievalTask

    index, q, passages, _ = grid_index()
    ctx = str(tmp_path / "ctx")
    b = colbert.TokenIndexBuilder()
    for j, p in enumerate(passages):
        if p.shape[0]:
            b.add(p.unsqueeze(0), torch.ones(1, p.shape[0]), [j])
    b.write(ctx, 0)
    base = dict(ctx_embeddings_dir=ctx, checkpoint_path="", topk=5, **_BASE)
    assert ColBERTRetrievalTask.__init__ is CITADELRetrievalTask.__init__ and ColBERTRetrievalTask.nprobe is None
    assert ColBERTRetrievalTask.n_centroids is None

    class Spy:
        def __init__(self, index):
            self.index, self.calls, self.device, self.latency = index, [], index.device, index.latency

        def search(self, *a, **kw):
            self.calls.append("search")
            return self.index.search(*a, **kw)

        def search_pruned(self, *a, **kw):
            self.calls.append(("search_pruned", a[2]))
            return self.index.search_pruned(*a, **kw)

    def run(task):
        task.kernels = CS.ColbertCandKernels()
        task.ctxs = range(N)
        task.index = Spy(task._load_index("cpu"))
        rep = {"expert_repr": q}
        return task.index, task._search(rep, NQ, 0.0)

    for kw in (dict(), dict(nprobe=2), dict(n_centroids=8), dict(nprobe=None, n_centroids=None)):
        spy, (v, i) = run(ColBERTPrunedRetrievalTask(**kw, **base))
        assert spy.calls == ["search"] and spy.index.centroids is None, kw
        assert torch.equal(i, index.search(q, 5)[1])
    spy, (v, i) = run(ColBERTPrunedRetrievalTask(nprobe=2, n_centroids=8, **base))
    assert spy.calls == [("search_pruned", 2)] and spy.index.centroids.shape[0] == 8
    want = colbert.load_index(ctx, N, "cpu", kernels=CS.ColbertCandKernels()).build_centroids(8).search_pruned(q, 5, 2)
    assert torch.equal(v, want[0]) and torch.equal(i, want[1])
    # centroids.pkl beside the token files is loaded instead of training
    index.save_centroids(os.path.join(ctx, ColBERTRetrievalTask.CENTROID_FILE))
    plain = ColBERTRetrievalTask(**base)
    plain.nprobe, plain.n_centroids = 3, C  # the knobs as attributes of the plain task
    spy, (v, i) = run(plain)
    assert spy.calls == [("search_pruned", 3)] and torch.equal(spy.index.centroids, index.centroids)
    want = index.search_pruned(q, 5, 3)
    assert torch.equal(v, want[0]) and torch.equal(i, want[1])
    # the product-quantised index refuses, with its reason
    with pytest.raises(NotImplementedError, match="dense rows only"):
        colbert.ColBERTPQIndex.__new__(colbert.ColBERTPQIndex).search_pruned(q, 5, 2)
    pq = ColBERTPQRetrievalTask(sub_vec_dim=4, **base)
    pq.nprobe, pq.n_centroids = 2, 8
    pq.index = colbert.ColBERTPQIndex.__new__(colbert.ColBERTPQIndex)
    with pytest.raises(NotImplementedError, match="dense rows only"):
        pq._search({"expert_repr": q}, NQ, 0.0)


def test_candidate_kernels_never_spill():
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
    mine = {k: v for k, v in rows.items() if re.search(r"dprhot\d+cbc_\w+_kernel", k)}
    assert len(mine) == 6, sorted(rows)  # the score kernel at dp = 32, 64, 96, 128 and any width, and the position-to-id launch
    for name, r in mine.items():
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
