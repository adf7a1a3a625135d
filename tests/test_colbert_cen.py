"""The centroid-interaction stage of the pruned ColBERT search on the CPU: host-side validation of
dprhot_colbert_cen_*, and ColBERTIndex.doc_centroids / centroid_table / approx_candidates / prune_candidates / search_pruned(ndocs=) and
the task driven through the test-only stand-in (tests/_colbert_cen_standin.py).  Tokens, queries and the given centroids lie on a grid
of multiples of 1/4, so every product, maximum and pooled sum is exact in fp32 and in float64 alike: lists, approximate scores,
survivors and the pruned top-k are compared with exact equality."""
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
import _colbert_cen_standin as CE  # noqa: E402
import _colbert_oracle as CO  # noqa: E402
from dpr_scale_amd import colbert  # noqa: E402

REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
_BASE = dict(transform=None, model=None, datamodule=None, optim=None)
NQ, LQ, N, LD, D, C = 4, 6, 30, 40, 20, 16
LT = 16


class Counting(CE.ColbertCenKernels):
    """The stand-in, noting the queries of every table it is asked for."""

    def __init__(self):
        self.tables = []

    def colbert_cen_table(self, index, q, T):
        self.tables.append(int(q.shape[0]))
        super().colbert_cen_table(index, q, T)


def grid_index(seed=3, kernels=None, **kw):
    """(index with given grid centroids, q, passages, centroids)"""
    lengths = np.random.default_rng(seed).permutation(np.resize(np.array([0, 1, 5, 15, 16, 17, 31, 33, 39]), N))
    q, c, att = CO.make_padded(seed, NQ, LQ, N, LD, D, lengths=lengths, q_pad=2)
    index = colbert.ColBERTIndex.from_repr(c, att, list(range(N)), N, "cpu", kernels=kernels or CE.ColbertCenKernels(), **kw)
    cen = torch.from_numpy(np.random.default_rng(seed + 1).integers(-4, 5, size=(C, D)).astype(np.float32) / 4.0)
    cen[5] = cen[2]
    index.build_centroids(C, centroids=cen)
    return index, q, CO.passages_of(c, att), cen


def approx64(index, q, pool):
    """float64 [NQ, N]: approx of every query and passage by its definition -- the exact score of the passages with every token replaced
    by its centroid (the maximum over a passage's tokens is the maximum over its duplicate-free centroid list)."""
    return CO.score(q, CE.centroid_passages(index), pool)


_ONE = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch


def test_host_side_validation_of_the_four_entry_points():
    from dpr_scale_amd import _lib

    lib = _lib.lib
    out = ctypes.c_size_t(0)
    ws_bytes = lib.dprhot_colbert_cen_workspace_bytes
    assert ws_bytes(2, 64, ctypes.byref(out)) == 0 and out.value >= 2 * 64 * 4
    assert ws_bytes(2, 64, None) == -1 and ws_bytes(0, 64, ctypes.byref(out)) == -1
    assert ws_bytes(2, 0, ctypes.byref(out)) == -1 and ws_bytes(2, 12, ctypes.byref(out)) == -1

    good_table = dict(cen=_ONE, C=16, dp=32, q=_ONE, nq=2, LQ=5, T=_ONE, st=None)
    table = lambda **bad: lib.dprhot_colbert_cen_table(*{**good_table, **bad}.values())
    for bad, word in ((dict(cen=None), b"NULL"), (dict(q=None), b"NULL"), (dict(T=None), b"NULL"), (dict(C=0), b"C="), (dict(C=-3), b"C="),
                      (dict(dp=40), b"dp="), (dict(dp=0), b"dp="), (dict(LQ=0), b"LQ="), (dict(LQ=513), b"LQ="), (dict(nq=0), b"nq="),
                      (dict(nq=65536), b"nq=")):
        assert table(**bad) == -1 and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())
    assert table(dp=800) == -3

    head = dict(off=_ONE, cen=_ONE, npairs=70, n=100, C=16, T=_ONE, nq=2, LQ=5, pool=0, coff=_ONE, cdoc=_ONE, nc=50)
    good_score = dict(head, b=0, cols=8, S=_ONE, ld=8, st=None)
    score = lambda **bad: lib.dprhot_colbert_cen_score(*{**good_score, **bad}.values())
    for bad in (dict(S=None), dict(off=None), dict(cen=None), dict(T=None), dict(T=ctypes.c_void_p(260)), dict(npairs=-1), dict(npairs=2 ** 40),
                dict(C=0), dict(LQ=0), dict(LQ=513), dict(coff=None), dict(cdoc=None), dict(nc=-1), dict(nc=2 ** 40), dict(cols=0),
                dict(ld=7), dict(b=-1), dict(pool=7), dict(n=0), dict(n=2 ** 31), dict(nq=0), dict(nq=65536)):
        assert score(**bad) == -1, (bad, lib.dprhot_last_error())

    good = dict(head, mc=40, k=5, chunk=64, vals=_ONE, idx=_ONE, ws=_ONE, wsb=1 << 20, st=None)
    search = lambda **bad: lib.dprhot_colbert_cen_search(*{**good, **bad}.values())
    for bad, word in ((dict(vals=None), b"NULL"), (dict(idx=None), b"NULL"), (dict(chunk=0), b"chunk"), (dict(chunk=12), b"chunk"),
                      (dict(k=0), b"topk"), (dict(k=101), b"topk"), (dict(mc=0), b"max_count"), (dict(mc=2 ** 31), b"max_count"),
                      (dict(C=0), b"C="), (dict(LQ=0), b"LQ="), (dict(LQ=513), b"LQ="), (dict(nc=2 ** 40), b"n_cand"),
                      (dict(npairs=2 ** 40), b"n_pairs"), (dict(off=None), b"NULL"), (dict(coff=None), b"NULL"), (dict(T=None), b"NULL"),
                      (dict(pool=2), b"pool")):
        assert search(**bad) == -1 and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())
    for bad in (dict(ws=None), dict(wsb=16)):
        assert search(**bad) == -4
        err = lib.dprhot_last_error()
        assert b"colbert_cen_search needs" in err and b"dprhot_colbert_cen_workspace_bytes" in err and b"topk_wide" not in err, err
    assert search(n=6000, mc=6000, k=5000, wsb=2 * 64 * 4) == -4  # k > 4096: the wide selection's state is missing
    err = lib.dprhot_last_error()
    assert b"dprhot_colbert_cen_workspace_bytes + dprhot_topk_wide_workspace_bytes" in err, err


def test_version_stays_and_the_symbols_are_bound():
    from dpr_scale_amd import _lib, hotpath

    assert _lib.version() == 174
    for s in ("dprhot_colbert_cen_table", "dprhot_colbert_cen_workspace_bytes", "dprhot_colbert_cen_score", "dprhot_colbert_cen_search"):
        assert s in _lib.SIGNATURES and hasattr(_lib.lib, s)
    assert _lib.colbert_cen_workspace_bytes(3, 16) == _lib.colbert_workspace_bytes(3, 16)
    for m in ("colbert_cen_table", "colbert_cen_score", "colbert_cen_workspace", "colbert_cen_search"):
        assert callable(getattr(hotpath.HipKernels, m))


def test_doc_centroids_are_the_lists_derived_on_the_host_and_the_transpose_of_the_inverted_lists():
    index, _, passages, _ = grid_index()
    before = index.nbytes
    four = sum(t.numel() * t.element_size() for t in (index.tok, index.doc_blk, index.centroids, index.tok_centroid, index.cen_off, index.cen_doc))
    assert before == four  # nothing is built by build_centroids
    doc_cen_off, doc_cen = index.doc_centroids()
    assert doc_cen_off.dtype == torch.int64 and doc_cen_off.shape == (N + 1,) and doc_cen.dtype == torch.int32
    off, cen = CE.doc_lists_from_assignment(index.tok_centroid, index.doc_blk)
    assert doc_cen_off.tolist() == off and doc_cen.tolist() == cen
    for j, p in enumerate(passages):
        mine = cen[off[j]:off[j + 1]]
        assert mine == sorted(set(mine)) and all(0 <= c < C for c in mine) and (len(mine) > 0) == (p.shape[0] > 0)
    # the transpose: (centroid, doc) pairs of cen_off / cen_doc are the (doc, centroid) pairs of doc_cen_off / doc_cen
    pairs = {(c, d) for c in range(C) for d in index.cen_doc[index.cen_off[c]:index.cen_off[c + 1]].tolist()}
    assert pairs == {(c, d) for d in range(N) for c in cen[off[d]:off[d + 1]]} and len(pairs) == len(cen) == index.cen_doc.numel()
    # cached, counted once built, dropped with the centroids
    again = index.doc_centroids()
    assert again[0] is doc_cen_off and again[1] is doc_cen
    assert index.nbytes == before + doc_cen_off.numel() * 8 + doc_cen.numel() * 4
    index._set_centroids(index.centroids, index.tok_centroid, index.cen_off, index.cen_doc)
    assert index.nbytes == before and index.doc_centroids()[0] is not doc_cen_off
    plain = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, N, D, kernels=CE.ColbertCenKernels())
    for call in (plain.doc_centroids, lambda: plain.centroid_table(torch.zeros(1, 2, D))):
        with pytest.raises(ValueError, match="no centroids"):
            call()


def test_the_centroid_pickle_stays_a_4_tuple(tmp_path):
    import pickle

    index, q, _, _ = grid_index()
    index.doc_centroids()
    blob = pickle.load(open(index.save_centroids(str(tmp_path / "c.pkl")), "rb"))
    assert isinstance(blob, tuple) and len(blob) == 4
    other = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, N, D, kernels=CE.ColbertCenKernels()).load_centroids(str(tmp_path / "c.pkl"))
    for a, b in zip(index.doc_centroids(), other.doc_centroids()):
        assert torch.equal(a, b)
    for x, y in zip(index.search_pruned(q, 3, 2, ndocs=5), other.search_pruned(q, 3, 2, ndocs=5)):
        assert torch.equal(x, y)


def test_centroid_table_is_the_matrix_of_products():
    index, q, _, cen = grid_index()
    T = index.centroid_table(q)
    assert T.dtype == torch.float32 and T.shape == (NQ, C, LT)
    want = torch.einsum("nid,cd->nci", CO.bf16(q), cen.double())
    assert torch.equal(T[:, :, :LQ].double(), want) and not T[:, :, LQ:].any()
    assert torch.equal(index.centroid_table({"expert_repr": q}), T)


def test_standin_takes_any_list_as_the_kernel_documents():
    """Hand-made per-passage lists with an id outside [0, C), a duplicate and offsets that run backwards, under hand-made candidate
    lists with a doc id outside the corpus: an outside centroid id is skipped, an outside doc id is no candidate."""
    index, q, _, _ = grid_index()
    T64 = index.centroid_table(q).double()
    doc_cen = torch.tensor([3, C, 7, -1, 7, 2, 9], dtype=torch.int32)
    doc_cen_off = torch.zeros(N + 1, dtype=torch.int64)
    doc_cen_off[1:] = 99                       # passage 0: entries 0 .. 7 (99 is clamped to the 7 entries)
    doc_cen_off[4], doc_cen_off[5] = 2, 5      # passage 3: empty (its end 2 lies below its begin 7); passage 4: entries 2, 3, 4
    index._doc_cen = (doc_cen_off, doc_cen)
    cand_doc = torch.tensor([0, 4, N, -1, 3, 4], dtype=torch.int32)
    cand_off = torch.tensor([0, 5, 3, 99, 6], dtype=torch.int64)  # query 0: 5 entries; 1: empty; 2: entries 3 .. 6; 3: empty
    S = index.approx_candidates(q, cand_off, cand_doc)
    assert S.shape == (NQ, 5)
    assert float(S[0, 0]) == float(CE.approx_of_list(T64[0], [3, 7, 2, 9], LQ, "sum"))       # C and -1 are skipped
    assert float(S[0, 1]) == float(CE.approx_of_list(T64[0], [7], LQ, "sum"))                # 7, -1, 7
    assert bool(torch.isnan(S[0, 2:4]).all()) and float(S[0, 4]) == 0.0                      # outside ids; an empty list scores 0
    assert bool(torch.isnan(S[1]).all()) and bool(torch.isnan(S[3]).all())
    assert bool(torch.isnan(S[2, 0])) and float(S[2, 1]) == 0.0 and bool(torch.isnan(S[2, 3:]).all())
    assert float(S[2, 2]) == float(CE.approx_of_list(T64[2], [7], LQ, "sum"))
    keep = index.prune_candidates(q, cand_off, cand_doc, 4)
    assert keep.dtype == torch.int32 and keep[0].tolist() == [-1, 0, 3, 4] and keep[1].tolist() == [-1] * 4
    assert keep[2].tolist() == [-1, -1, 3, 4] and keep[3].tolist() == [-1] * 4


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_approx_candidates_equal_the_definition_in_float64(pool):
    index, q, _, _ = grid_index()
    A = approx64(index, q, pool)
    assert bool((A > 0).any())
    for nprobe in (1, 2, C):
        cand_off, cand_doc = index.candidates(q, nprobe)
        counts = (cand_off[1:] - cand_off[:-1]).tolist()
        S = index.approx_candidates(q, cand_off, cand_doc, pool)
        assert S.shape == (NQ, max(counts)) and S.dtype == torch.float32
        for n in range(NQ):
            mine = cand_doc[cand_off[n]:cand_off[n + 1]].long()
            assert torch.equal(S[n, :counts[n]].double(), A[n, mine]) and bool(torch.isnan(S[n, counts[n]:]).all()), (nprobe, n)
    with pytest.raises(ValueError, match="cand_off"):
        index.approx_candidates(q, cand_off[:-1], cand_doc)


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_survivors_are_the_top_ndocs_of_the_approximate_matrix_sorted(pool):
    index, q, _, _ = grid_index()
    cand_off, cand_doc = index.candidates(q, 2)
    S = index.approx_candidates(q, cand_off, cand_doc, pool)
    counts = (cand_off[1:] - cand_off[:-1]).tolist()
    for ndocs in (1, 4, 9, max(counts) + 3):
        keep = index.prune_candidates(q, cand_off, cand_doc, ndocs, pool)
        assert keep.dtype == torch.int32 and keep.shape == (NQ, ndocs)
        _, ids = CS.topk_of_positions(S, ndocs, cand_off, cand_doc)
        assert torch.equal(keep.long(), torch.sort(ids, dim=1).values), ndocs
        for n in range(NQ):  # -1 entries first, then ascending doc ids of the query's own list
            m = min(ndocs, counts[n])
            assert keep[n, :ndocs - m].tolist() == [-1] * (ndocs - m) and set(keep[n, ndocs - m:].tolist()) <= set(cand_doc[cand_off[n]:cand_off[n + 1]].tolist())
    with pytest.raises(ValueError, match="ndocs"):
        index.prune_candidates(q, cand_off, cand_doc, 0)


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_search_pruned_with_ndocs_is_the_exhaustive_top_k_restricted_to_the_survivors(pool):
    index, q, passages, _ = grid_index(chunk=8)
    full = CO.score(q, passages, pool)
    for nprobe, ndocs, k in ((2, 6, 3), (2, 6, 6), (C, 10, 7), (1, 2, 1)):
        cand_off, cand_doc = index.candidates(q, nprobe)
        counts = (cand_off[1:] - cand_off[:-1]).tolist()
        assert max(counts) > ndocs  # the stage runs
        keep = index.prune_candidates(q, cand_off, cand_doc, ndocs, pool)
        index.latency.pop("interaction_time", None)
        v, i = index.search_pruned(q, k, nprobe, query_pool=pool, ndocs=ndocs)
        assert index.latency["interaction_time"] > 0
        assert v.shape == (NQ, k) and v.dtype == torch.float32 and i.dtype == torch.int64
        for n in range(NQ):
            mine = keep[n][keep[n] >= 0].long()
            tv, ti = CO.topk(full[n:n + 1, mine], k)  # sorted ids: ties to the lower position are ties to the lower doc id
            m = min(k, mine.numel())
            assert torch.equal(v[n, :m].double(), tv[0]) and torch.equal(i[n, :m], mine[ti[0]]), (nprobe, ndocs, k, n)
            assert bool((v[n, m:] == float("-inf")).all()) and bool((i[n, m:] == -1).all())
    # ndocs at or above every query's count: the stage is skipped, the result is today's
    cand_off, _ = index.candidates(q, 2)
    most = int((cand_off[1:] - cand_off[:-1]).max())
    want = index.search_pruned(q, 5, 2, query_pool=pool)
    for ndocs in (most, most + 1, 10 ** 6):
        index.latency.pop("interaction_time", None)
        got = index.search_pruned(q, 5, 2, query_pool=pool, ndocs=ndocs)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and "interaction_time" not in index.latency
    for bad in (4, 1):
        with pytest.raises(ValueError, match="ndocs"):
            index.search_pruned(q, 5, 2, ndocs=bad)
    # a query of padding only has no candidate and no survivor
    v, i = index.search_pruned(torch.zeros(2, 3, D), 4, 2, ndocs=4)
    assert bool((v == float("-inf")).all()) and bool((i == -1).all())


def test_the_result_does_not_depend_on_the_table_batch(monkeypatch):
    kn = Counting()
    index, q, _, _ = grid_index(kernels=kn)
    per_query = C * LT * 4
    assert colbert.CEN_TABLE_BYTES == 1 << 28
    cand_off, cand_doc = index.candidates(q, 2)
    kn.tables.clear()
    want = index.search_pruned(q, 4, 2, ndocs=6)
    want_keep, want_S = index.prune_candidates(q, cand_off, cand_doc, 6), index.approx_candidates(q, cand_off, cand_doc)
    assert kn.tables == [NQ] * 3  # the default: one batch
    for limit, batches in ((1, [1] * NQ), (per_query, [1] * NQ), (2 * per_query, [2, 2]), (3 * per_query, [3, 1]), (NQ * per_query, [NQ])):
        monkeypatch.setattr(colbert, "CEN_TABLE_BYTES", limit)
        kn.tables.clear()
        got = index.search_pruned(q, 4, 2, ndocs=6)
        assert kn.tables == batches, limit
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), limit
        assert torch.equal(index.prune_candidates(q, cand_off, cand_doc, 6), want_keep)
        assert torch.equal(index.approx_candidates(q, cand_off, cand_doc).view(torch.int32), want_S.view(torch.int32))


def test_the_task_passes_ndocs_only_with_pruning_on(tmp_path):
    from dpr_scale_amd.task.citadel_retrieval import CITADELRetrievalTask
    from dpr_scale_amd.task.colbert_retrieval import ColBERTPQRetrievalTask, ColBERTPrunedRetrievalTask, ColBERTRetrievalTask

    index, q, passages, _ = grid_index()
    ctx = str(tmp_path / "ctx")
    b = colbert.TokenIndexBuilder()
    for j, p in enumerate(passages):
        if p.shape[0]:
            b.add(p.unsqueeze(0), torch.ones(1, p.shape[0]), [j])
    b.write(ctx, 0)
    index.save_centroids(os.path.join(ctx, ColBERTRetrievalTask.CENTROID_FILE))
    base = dict(ctx_embeddings_dir=ctx, checkpoint_path="", topk=5, **_BASE)
    assert ColBERTRetrievalTask.__init__ is CITADELRetrievalTask.__init__ and ColBERTRetrievalTask.ndocs is None

    class Spy:
        def __init__(self, index):
            self.index, self.calls, self.device, self.latency = index, [], index.device, index.latency

        def search(self, *a, **kw):
            self.calls.append(("search", kw))
            return self.index.search(*a, **kw)

        def search_pruned(self, *a, **kw):
            self.calls.append(("search_pruned", kw))
            return self.index.search_pruned(*a, **kw)

    def run(task):
        task.kernels = CE.ColbertCenKernels()
        task.ctxs = range(N)
        task.index = Spy(task._load_index("cpu"))
        return task.index, task._search({"expert_repr": q}, NQ, 0.0)

    for kw in (dict(ndocs=6), dict(ndocs=6, nprobe=2), dict(ndocs=6, n_centroids=C)):  # pruning off: ndocs goes nowhere
        spy, (v, i) = run(ColBERTPrunedRetrievalTask(**kw, **base))
        assert spy.calls == [("search", dict(query_pool="sum"))], kw
        assert torch.equal(i, index.search(q, 5)[1])
    spy, (v, i) = run(ColBERTPrunedRetrievalTask(nprobe=2, n_centroids=C, **base))
    assert spy.calls == [("search_pruned", dict(query_pool="sum"))]
    spy, (v, i) = run(ColBERTPrunedRetrievalTask(nprobe=2, n_centroids=C, ndocs=6, **base))
    assert spy.calls == [("search_pruned", dict(query_pool="sum", ndocs=6))]
    want = index.search_pruned(q, 5, 2, ndocs=6)
    assert torch.equal(v, want[0]) and torch.equal(i, want[1])
    plain = ColBERTRetrievalTask(**base)
    plain.nprobe, plain.n_centroids, plain.ndocs = 2, C, 7  # the knobs as attributes of the plain task
    spy, (v, i) = run(plain)
    assert spy.calls == [("search_pruned", dict(query_pool="sum", ndocs=7))]
    want = index.search_pruned(q, 5, 2, ndocs=7)
    assert torch.equal(v, want[0]) and torch.equal(i, want[1])
    # the product-quantised index still refuses, with its reason
    with pytest.raises(NotImplementedError, match="dense rows only"):
        colbert.ColBERTPQIndex.__new__(colbert.ColBERTPQIndex).search_pruned(q, 5, 2, ndocs=6)
    pq = ColBERTPQRetrievalTask(sub_vec_dim=4, **base)
    pq.nprobe, pq.n_centroids, pq.ndocs = 2, 8, 6
    pq.index = colbert.ColBERTPQIndex.__new__(colbert.ColBERTPQIndex)
    with pytest.raises(NotImplementedError, match="dense rows only"):
        pq._search({"expert_repr": q}, NQ, 0.0)


def test_centroid_interaction_kernels_never_spill():
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
    mine = {k: v for k, v in rows.items() if re.search(r"dprhot\d+cbi_\w+_kernel", k)}
    assert len(mine) == 6, sorted(rows)  # the table kernel at dp = 32, 64, 96, 128 and any width, and the score kernel
    assert sum("cbi_table_kernel" in k for k in mine) == 5 and sum("cbi_score_kernel" in k for k in mine) == 1
    for name, r in mine.items():
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
