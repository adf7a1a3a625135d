"""Inverted-index retrieval on the MI355X (csrc/ivf.h through dprhot_ivf_score / dprhot_ivf_search).

Grid fixtures (tests/golden/ivf_*.npz, written from the reference's tasks) must come out BIT-EQUAL.  Gaussian inputs are compared
with the float64 oracle on bf16-rounded operands under a per-cell bound derived from the arithmetic, not measured:
  * a dot product of dp exact products accumulated in fp32 is off by at most dp * 2^-23 * sum_k |u_k v_k|;
  * a cell that receives m contributions (+ the CLS part) in fp32 is off by at most a further (m + 1) * 2^-23 * sum |contribution|,
    and |contribution| <= sum_k |u_k v_k|.
With A[n, doc] = the sum over the cell's entries (and its CLS part) of sum_k |u_k v_k| (for an entry: the largest such sum among the
doc's postings), bound[n, doc] = (max(dp, dc) + m + 1) * 2^-23 * A[n, doc]."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ivf_fixture as F  # noqa: E402
import _ivf_oracle as O  # noqa: E402
from dpr_scale_amd import ivf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5


def synth(seed, ndocs, V, d, nq, ne, dc=0, hot_frac=0.6):
    """Zipf expert sizes; expert 0 holds a posting in more than half of the docs (and several postings in many of them)."""
    g = np.random.default_rng(seed)
    post = {}
    for e in range(V):
        n = max(2, int(ndocs * hot_frac * 1.6 / (e + 1)))
        ids = np.sort(g.integers(0, ndocs, size=n))
        if e == 0:
            ids = np.sort(np.concatenate([ids, g.permutation(ndocs)[: int(ndocs * hot_frac)]]))
        post[e] = (ids, g.standard_normal((len(ids), d)).astype(np.float32))
    queries = []
    for _ in range(nq):
        q = {}
        for _ in range(ne):
            e = 0 if g.random() < 0.25 else int(g.integers(0, V))
            q.setdefault(e, []).append(torch.from_numpy(g.standard_normal(d).astype(np.float32)))
        queries.append(q)
    cq = torch.from_numpy(g.standard_normal((nq, dc)).astype(np.float32)) if dc else []
    cd = torch.from_numpy(g.standard_normal((ndocs, dc)).astype(np.float32)) if dc else None
    return post, queries, cq, cd


def build(post, cd, ndocs, chunk=None):
    ex = torch.cat([torch.full((len(v[0]),), e, dtype=torch.int64) for e, v in post.items()])
    docs = torch.cat([torch.from_numpy(np.asarray(v[0], dtype=np.int64)) for v in post.values()])
    vecs = torch.cat([torch.from_numpy(v[1]) for v in post.values()])
    return ivf.IVFIndex(ex, docs, vecs, cd, ndocs, DEV, chunk=chunk)


def bare_search(index, qb, k, chunk, guard=False, id_ranges=None):
    """dprhot_ivf_search through ctypes alone; with guard=True every output and an exactly sized workspace sit between bands."""
    from dpr_scale_amd import _lib

    qb = qb.to(DEV)
    n = ctypes.c_size_t(0)
    _lib.check(_lib.lib.dprhot_ivf_workspace_bytes(qb.nq, qb.n_entries, chunk, int(index.cls is not None), ctypes.byref(n)))
    nws = n.value
    if k > 4096:
        _lib.check(_lib.lib.dprhot_topk_wide_workspace_bytes(qb.nq, k, ctypes.byref(n)))
        nws += n.value
    raws = []

    def alloc(nbytes):
        raw = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        raws.append((raw, nbytes))
        return raw[GUARD:GUARD + nbytes]

    values = alloc(qb.nq * k * 4).view(torch.float32).view(qb.nq, k)
    indices = alloc(qb.nq * k * 8).view(torch.int64).view(qb.nq, k)
    ws = alloc(nws)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    first = 1
    for b, e in (id_ranges or [(0, index.corpus_len)]):
        _lib.check(_lib.lib.dprhot_ivf_search(
            p(index.post_vec), p(index.post_doc), p(index.exp_off), index.n_postings, index.n_experts, index.dp, p(qb.ent_vec), p(qb.ent_q),
            qb.n_entries, p(qb.bexp), p(qb.boff), int(qb.bexp.shape[0]), qb.nq, p(qb.cls), p(index.cls), index.dc,
            0 if index.cls is None else index.cls.shape[0], index.corpus_len, b, e, k, chunk, p(values), p(indices), first, p(ws), nws,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "dprhot_ivf_search")
        first = 0
    torch.cuda.synchronize()
    if guard:
        for raw, nb in raws:
            assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[GUARD + nb:] == PATTERN).all()), "guard band overwritten"
    return values.clone(), indices.clone()


@pytest.mark.parametrize("name", F.NAMES)
def test_golden_bit_equal(name, tmp_path):
    meta, z = F.load(name)
    cls_q, emb, wts = F.queries(meta, z)
    for splits in (1, 2):
        index = ivf.load_index(F.write_tree(str(tmp_path / str(splits)), z, splits), meta["corpus_len"], DEV)
        v, i = index.search(cls_q, emb, wts, meta["topk"])
        assert np.array_equal(v.cpu().numpy(), z["top_scores"]) and np.array_equal(i.cpu().numpy(), z["top_ids"])
    v, i = bare_search(index, ivf.pack_queries(cls_q, emb, wts), meta["topk"], 8, guard=True)
    assert np.array_equal(v.cpu().numpy(), z["top_scores"]) and np.array_equal(i.cpu().numpy(), z["top_ids"])
    # the whole score matrix through dprhot_ivf_score (on top of the CLS part computed here in fp32: grid values, exact)
    from dpr_scale_amd import hotpath

    S = torch.zeros((meta["nq"], meta["corpus_len"]), device=DEV)
    if "cls_q" in z:
        S += torch.from_numpy(z["cls_q"] @ z["cls_doc"].T).to(DEV)
    hotpath.default_kernels().ivf_score(index, ivf.pack_queries([], emb, wts).to(DEV), 0, meta["corpus_len"], S)
    assert np.array_equal(S.cpu().numpy(), z["scores"])


def test_ties_go_to_the_lower_doc_id():
    u = torch.tensor([1.0, -2.0, 0.5, 3.0] * 8)
    post = {4: (np.array([3, 5, 9, 9]), np.stack([-u.numpy(), u.numpy(), -u.numpy(), -2 * u.numpy()]))}  # docs 3 and 9: clamped to 0
    index = build(post, None, 16)
    v, i = index.search([], [{4: [u]}], None, 16)
    assert i[0].tolist() == [5] + [d for d in range(16) if d != 5]
    assert v[0, 0].item() == float(u @ u) and not v[0, 1:].any()


@pytest.mark.parametrize("d,dc", [(32, 0), (20, 24)])
def test_gaussian_within_the_derived_bound(d, dc):
    ndocs, k = 2003, 100
    post, queries, cq, cd = synth(11 + d, ndocs, 60, d, 8, 24, dc)
    assert len(np.unique(post[0][0])) > ndocs // 2
    index = build(post, cd, ndocs)
    S, A, m = O.score_matrix(post, queries, ndocs, cq if dc else None, cd, bf16=True, return_abs=True)
    bound = (max(index.dp, index.dc) + m + 1) * 2.0 ** -23 * A
    v, i = index.search(cq, queries, None, k)
    v, i = v.cpu().numpy().astype(np.float64), i.cpu().numpy()
    worst = 0.0
    for n in range(len(queries)):
        assert len(set(i[n].tolist())) == k and i[n].min() >= 0 and i[n].max() < ndocs
        err = np.abs(v[n] - S[n, i[n]])
        worst = max(worst, float((err / np.maximum(bound[n, i[n]], 1e-300)).max()))
        assert (err <= bound[n, i[n]]).all(), (n, float(err.max()))
        assert (np.diff(v[n]) <= 0).all()
        rest = np.setdiff1d(np.arange(ndocs), i[n])
        # nothing left out may beat the k-th returned score by more than the two cells' bounds
        kth = int(np.argmin(v[n]))
        assert (S[n, rest] <= v[n, kth] + bound[n, rest] + bound[n, i[n][kth]]).all()
    print(f"d={d} dc={dc}: worst error / bound = {worst:.3f}")
    # the full matrix of the expert part
    from dpr_scale_amd import hotpath

    S0, A0, m0 = O.score_matrix(post, queries, ndocs, bf16=True, return_abs=True)
    Sg = torch.zeros((len(queries), ndocs), device=DEV)
    hotpath.default_kernels().ivf_score(index, ivf.pack_queries([], queries, None).to(DEV), 0, ndocs, Sg)
    assert (np.abs(Sg.cpu().numpy().astype(np.float64) - S0) <= (index.dp + m0 + 1) * 2.0 ** -23 * A0).all()


def test_runs_are_bit_identical_and_independent_of_chunk_batch_and_shards(tmp_path):
    ndocs, k = 2003, 50
    post, queries, cq, cd = synth(3, ndocs, 60, 32, 8, 24, 16)
    index = build(post, cd, ndocs)
    ref_v, ref_i = index.search(cq, queries, None, k, chunk=2008)
    again_v, again_i = index.search(cq, queries, None, k, chunk=2008)
    assert torch.equal(ref_v, again_v) and torch.equal(ref_i, again_i)  # property A
    for chunk in (128, 1000):  # property B: chunk
        v, i = index.search(cq, queries, None, k, chunk=chunk)
        assert torch.equal(ref_v, v) and torch.equal(ref_i, i), chunk
    v, i = index.search(cq, queries, None, k, id_ranges=[(700, 2003), (0, 700)], chunk=256)
    assert torch.equal(ref_v, v) and torch.equal(ref_i, i)
    for n in (0, 5):  # property B: a batch of one
        v, i = index.search(cq[n:n + 1], queries[n:n + 1], None, k)
        assert torch.equal(ref_v[n:n + 1], v) and torch.equal(ref_i[n:n + 1], i), n
    # property B: one shard directory against two (file trees as the index writer lays them out)
    z = dict(post_expert=np.concatenate([np.full(len(p[0]), e) for e, p in post.items()]),
             post_doc=np.concatenate([p[0] for p in post.values()]).astype(np.int64),
             post_weight=np.ones(sum(len(p[0]) for p in post.values()), np.float32),
             post_vec=np.concatenate([p[1] for p in post.values()]), cls_doc=cd.numpy(), scores=np.zeros((1, ndocs)))
    for splits in (1, 2):
        idx = ivf.load_index(F.write_tree(str(tmp_path / str(splits)), z, splits), ndocs, DEV)
        v, i = idx.search(cq, queries, None, k)
        assert torch.equal(ref_v, v) and torch.equal(ref_i, i), splits


def test_guard_bands_and_topk_edges():
    ndocs = 5003
    post, queries, cq, cd = synth(7, ndocs, 40, 20, 3, 10, 8)
    queries[1] = {}                                   # a query with no entries: its scores are the CLS part
    queries[2][1000] = [torch.ones(20)]               # an expert the index does not hold
    index = build(post, cd, ndocs)
    S, A, m = O.score_matrix(post, queries, ndocs, cq, cd, bf16=True, return_abs=True)
    bound = (max(index.dp, index.dc) + m + 1) * 2.0 ** -23 * A  # (the module docstring's bound)
    qb = ivf.pack_queries(cq, queries, None)
    for k, chunk in ((1, 1024), (ndocs, 2048), (4500, 1024)):  # 4500 > 4096: the HBM-resident selection
        v, i = bare_search(index, qb, k, chunk, guard=True)
        v, i = v.cpu().numpy(), i.cpu().numpy()
        for n in range(3):
            assert len(set(i[n].tolist())) == k
            assert (np.abs(v[n] - S[n, i[n]]) <= bound[n, i[n]]).all() and (np.diff(v[n]) <= 0).all()
            assert abs(v[n, 0] - S[n].max()) <= 2 * bound[n].max()
        if k == ndocs:
            assert np.array_equal(np.sort(i, 1), np.broadcast_to(np.arange(ndocs), (3, ndocs)))
    # no CLS, no entries at all: every score is 0 and the ids come in ascending order
    index0 = build(post, None, ndocs)
    v, i = bare_search(index0, ivf.pack_queries([], [{}, {}], None, d=20), 7, 512, guard=True)
    assert not v.any() and i.tolist() == [list(range(7))] * 2
    # dprhot_ivf_score between bands
    from dpr_scale_amd import hotpath

    raw = torch.full((2 * GUARD + 3 * 1000 * 4,), PATTERN, dtype=torch.uint8, device=DEV)
    Sg = raw[GUARD:-GUARD].view(torch.float32).view(3, 1000)
    Sg.zero_()
    hotpath.default_kernels().ivf_score(index0, ivf.pack_queries([], queries, None).to(DEV), 4003, 1000, Sg)
    torch.cuda.synchronize()
    assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[-GUARD:] == PATTERN).all())
    S0, A0, m0 = O.score_matrix(post, queries, ndocs, bf16=True, return_abs=True)
    assert (np.abs(Sg.cpu().numpy() - S0[:, 4003:]) <= ((index0.dp + m0 + 1) * 2.0 ** -23 * A0)[:, 4003:]).all()


def test_error_returns():
    from dpr_scale_amd import _lib

    post, queries, cq, cd = synth(9, 300, 10, 32, 2, 4, 8)
    index = build(post, cd, 300)
    qb = ivf.pack_queries(cq, queries, None)
    with pytest.raises(_lib.DprhotError, match="topk"):
        bare_search(index, qb, 301, 64)
    with pytest.raises(_lib.DprhotError, match="chunk"):
        index._kernels().ivf_search(index, qb.to(DEV), 0, 300, torch.empty((2, 5), device=DEV),
                                    torch.empty((2, 5), dtype=torch.int64, device=DEV), True, 12, torch.empty(1 << 16, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.DprhotError, match="range"):
        bare_search(index, qb, 5, 64, id_ranges=[(10, 301)])
    with pytest.raises(_lib.DprhotError, match="workspace"):
        index._kernels().ivf_search(index, qb.to(DEV), 0, 300, torch.empty((2, 5), device=DEV),
                                    torch.empty((2, 5), dtype=torch.int64, device=DEV), True, 64, torch.empty(64, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="CLS"):
        index.search([], queries, None, 5)
    with pytest.raises(ValueError, match="corpus_len"):
        ivf.IVFIndex(torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.zeros(1, 32), None, 2 ** 31, DEV)
