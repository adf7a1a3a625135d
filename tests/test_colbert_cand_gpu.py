"""MaxSim over candidate lists on the MI355X (csrc/colbert_cand.h through dprhot_colbert_cand_score / dprhot_colbert_cand_search) and
ColBERTIndex.search_pruned end to end.

The yardstick is the exhaustive kernel: a candidate cell must be BIT-EQUAL to the cell dprhot_colbert_score writes for the same query and
passage (torch.equal, no tolerance), whatever the list, the window and the other queries are.  Against the float64 oracle on gaussian
inputs the derived per-cell bound of tests/test_colbert_gpu.py holds unchanged -- the arithmetic is the same:
    bound[n, doc] = (dp + LQ + 1) * 2^-23 * A[n, doc],   A[n, doc] = sum_i max_j sum_k |q_ik c_jk|
`cand_search` is compared with the total-order top-k of the kernel's own `cand_score` matrix mapped to doc ids, with torch.equal.
S, values, indices and the workspace are exactly sized and sit between 4 KiB guard bands.  Every list is valid; nothing here provokes a
fault."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _colbert_cand_standin as CS  # noqa: E402
import _colbert_oracle as CO  # noqa: E402
from dpr_scale_amd import colbert  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
LENGTHS = [0, 1, 15, 16, 17, 31, 33, 64, 65, 180, 513]
NP = 40
SHAPES = {  # d (dp), nq, LQ, poolings
    "d24": (24, 5, 7, ("sum", "max")),       # dp = 32: one k-step, one fragment
    "d128": (128, 3, 33, ("sum", "max")),    # dp = 128: four k-steps, three fragments
    "d160": (160, 2, 16, ("sum",)),          # dp = 160: the any-width instantiation
    "d32-long": (32, 2, 260, ("sum",)),      # 17 fragments: five passes over every passage
}
SHAPE_POOLS = [(s, p) for s, v in SHAPES.items() for p in v[3]]


@functools.lru_cache(maxsize=None)
def corpus(shape, nq=None):
    """(q, passages, index) of a shape: 40 gaussian bf16-exact passages of LENGTHS repeated (doc id = position)."""
    d, nq0, LQ, _ = SHAPES[shape]
    nq = nq0 if nq is None else nq
    g = torch.Generator().manual_seed(1000 + d + LQ)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    lengths = [int(x) for x in np.resize(np.array(LENGTHS), NP)]
    passages = [rnd(n, d) for n in lengths]
    q = rnd(nq, LQ, d)
    q[0, LQ - 1:] = 0.0  # one padded query token
    index = colbert.ColBERTIndex(list(range(NP)), lengths, torch.cat(passages, 0), NP, DEV)
    return q, passages, index


@functools.lru_cache(maxsize=None)
def exhaustive(shape, pool, nq=None):
    """The exhaustive kernel's score matrix [nq, 40]: the reference of every cell below.  Never modified."""
    q, _, index = corpus(shape, nq)
    return index.score(q, 0, None, pool)


def _banded(raws, nbytes):
    raw = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    raws.append((raw, nbytes))
    return raw[GUARD:GUARD + nbytes]


def _check_bands(raws):
    torch.cuda.synchronize()
    for raw, nb in raws:
        assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[GUARD + nb:] == PATTERN).all()), "guard band overwritten"


_p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def lists(per_query):
    """(cand_off int64 [nq + 1], cand_doc int32) on the device from one Python list of doc ids per query."""
    off = np.cumsum([0] + [len(x) for x in per_query])
    flat = [j for x in per_query for j in x]
    return torch.tensor(off, dtype=torch.int64, device=DEV), torch.tensor(flat, dtype=torch.int32, device=DEV)


def _head(index, qb, pool, cand_off, cand_doc):
    nq, LQ, dp = qb.shape
    return (_p(index.tok), _p(index.doc_blk), index.n_blk, index.corpus_len, dp, _p(qb), nq, LQ, CO.POOL[pool], _p(cand_off), _p(cand_doc),
            cand_doc.shape[0])


def bare_score(index, q, pool, cand_off, cand_doc, pos_begin, cols):
    """dprhot_colbert_cand_score through ctypes alone into an exactly sized S [nq, cols] between guard bands."""
    from dpr_scale_amd import _lib

    qb = colbert._bf16_padded(q.to(DEV), index.dp)
    raws = []
    S = _banded(raws, qb.shape[0] * cols * 4).view(torch.float32).view(qb.shape[0], cols)
    _lib.check(_lib.lib.dprhot_colbert_cand_score(*_head(index, qb, pool, cand_off, cand_doc), pos_begin, cols, _p(S), cols, _stream()),
               "dprhot_colbert_cand_score")
    _check_bands(raws)
    return S.clone()


def bare_search(index, q, pool, cand_off, cand_doc, max_count, k, chunk):
    """dprhot_colbert_cand_search through ctypes alone: values, indices and an exactly sized workspace sit between guard bands."""
    from dpr_scale_amd import _lib

    qb = colbert._bf16_padded(q.to(DEV), index.dp)
    nq = qb.shape[0]
    n = ctypes.c_size_t(0)
    _lib.check(_lib.lib.dprhot_colbert_cand_workspace_bytes(nq, chunk, ctypes.byref(n)))
    nws = n.value
    if k > 4096:
        _lib.check(_lib.lib.dprhot_topk_wide_workspace_bytes(nq, k, ctypes.byref(n)))
        nws += n.value
    raws = []
    values = _banded(raws, nq * k * 4).view(torch.float32).view(nq, k)
    indices = _banded(raws, nq * k * 8).view(torch.int64).view(nq, k)
    ws = _banded(raws, nws)
    _lib.check(_lib.lib.dprhot_colbert_cand_search(*_head(index, qb, pool, cand_off, cand_doc), max_count, k, chunk, _p(values), _p(indices),
                                                   _p(ws), nws, _stream()), "dprhot_colbert_cand_search")
    _check_bands(raws)
    return values.clone(), indices.clone()


@pytest.mark.parametrize("shape,pool", SHAPE_POOLS)
def test_all_candidates_equal_the_exhaustive_matrix_bit_for_bit(shape, pool):
    q, passages, index = corpus(shape)
    nq, LQ = q.shape[0], q.shape[1]
    want = exhaustive(shape, pool)
    cand_off, cand_doc = lists([list(range(NP))] * nq)
    S = bare_score(index, q, pool, cand_off, cand_doc, 0, NP)
    assert torch.equal(S, want)
    assert torch.equal(index.score_candidates(q, cand_off, cand_doc, pool), want)
    for pos_begin in (0, 8, 24):
        for cols in (8, 13):
            assert torch.equal(bare_score(index, q, pool, cand_off, cand_doc, pos_begin, cols), want[:, pos_begin:pos_begin + cols]), (pos_begin, cols)
    # the float64 oracle, under the bound derived for the exhaustive kernel
    ref = CO.score(q, passages, pool)
    bound = (index.dp + LQ + 1) * 2.0 ** -23 * CO.magnitude(q, passages)
    err = (S.cpu().double() - ref).abs()
    print(f"{shape}/{pool}: max err {err.max().item():.3e}, max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())
    assert not S[:, [j for j, p in enumerate(passages) if p.shape[0] == 0]].any()  # a passage without tokens scores 0


RAGGED = [[], [10], list(range(NP)), list(range(1, 39, 2)), [0]]  # none; the 513-token passage; all; every other id (19); the empty passage


@pytest.mark.parametrize("shape,pool", [("d24", "sum"), ("d24", "max"), ("d128", "sum"), ("d128", "max")])
def test_ragged_lists(shape, pool):
    q, passages, index = corpus(shape, 5)
    assert passages[10].shape[0] == 513 and passages[0].shape[0] == 0
    want = exhaustive(shape, pool, 5)
    cand_off, cand_doc = lists(RAGGED)
    width = NP + 3  # a window wider than the longest list: the cells behind a list are written too
    S = bare_score(index, q, pool, cand_off, cand_doc, 0, width)
    again = bare_score(index, q, pool, cand_off, cand_doc, 0, width)
    assert torch.equal(S.view(torch.int32), again.view(torch.int32))  # two runs: the same bits, NaN cells included
    for n, mine in enumerate(RAGGED):
        assert torch.equal(S[n, :len(mine)], want[n, mine]), n       # present cells: the exhaustive cells, bit for bit
        assert bool(torch.isnan(S[n, len(mine):]).all()), n          # absent cells: no candidate
    assert float(S[4, 0]) == 0.0
    # absent cells are never selected: a k above a row's count leaves -inf / -1 behind the row's candidates
    v, i = bare_search(index, q, pool, cand_off, cand_doc, NP, 30, 8)
    for n, mine in enumerate(RAGGED):
        m = min(30, len(mine))
        got = i[n, :m].tolist()
        assert set(got) <= set(mine) and len(set(got)) == m, n      # m distinct ids of the row's own list
        assert bool((i[n, m:] == -1).all()) and bool((v[n, m:] == float("-inf")).all()) and not bool(torch.isnan(v[n]).any())
    # a cell does not depend on the rest of its list, on the other queries or on the window
    rev_off, rev_doc = lists([list(reversed(RAGGED[3]))])
    alone = bare_score(index, q[3:4], pool, rev_off, rev_doc, 0, 19)
    assert torch.equal(alone.flip(1), S[3:4, :19])
    off2, doc2 = lists([RAGGED[3][5:9], [10, 7], RAGGED[3]])
    mixed = bare_score(index, q[[3, 1, 3]], pool, off2, doc2, 0, 19)
    assert torch.equal(mixed[0, :4], S[3, 5:9]) and torch.equal(mixed[2], S[3, :19]) and torch.equal(mixed[1, 0], S[1, 0])
    assert torch.equal(mixed[1, 1], want[1, 7]) and bool(torch.isnan(mixed[1, 2:]).all())
    # windows hold NaN cells: compared as bit patterns (the kernel writes ONE quiet NaN)
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(bare_score(index, q, pool, cand_off, cand_doc, 11, 7)), bits(S[:, 11:18]))
    assert torch.equal(bits(bare_score(index, q, pool, cand_off, cand_doc, 32, 9)), bits(S[:, 32:41]))  # a window that begins at a second run


@pytest.mark.parametrize("shape,pool", [("d24", "sum"), ("d128", "max")])
def test_search_is_the_top_k_of_the_kernels_own_scores(shape, pool):
    q, _, index = corpus(shape, 5)
    cand_off, cand_doc = lists(RAGGED)
    S = bare_score(index, q, pool, cand_off, cand_doc, 0, NP)
    for k in (1, 5, 30):  # 30: above the counts 0, 1, 19 and 1 -- tails of -inf / -1
        tv, ti = CS.topk_of_positions(S, k, cand_off, cand_doc)
        for chunk in (8, 64):
            v, i = bare_search(index, q, pool, cand_off, cand_doc, NP, k, chunk)
            assert torch.equal(v.cpu(), tv) and torch.equal(i.cpu(), ti), (k, chunk)
    # sorted, duplicate-free lists: ties to the lower doc id, the rule of the exhaustive search
    v, i = bare_search(index, q[2:3], pool, *lists([RAGGED[2]]), NP, 12, 16)
    ev, ei = index.search(q[2:3], 12, query_pool=pool)
    assert torch.equal(v, ev) and torch.equal(i, ei)


def test_wide_selection_over_candidate_lists():
    n, k = 6000, 5000
    g = torch.Generator().manual_seed(77)
    lengths = [int(x) for x in np.random.default_rng(5).integers(1, 4, size=n)]
    rows = torch.randn(sum(lengths), 32, generator=g).to(torch.bfloat16).float()
    q = torch.randn(2, 4, 32, generator=g).to(torch.bfloat16).float()
    index = colbert.ColBERTIndex(list(range(n)), lengths, rows, n, DEV)
    per_query = [list(range(n)), list(range(0, n, 2))]  # 6000 candidates; 3000: below k, a tail of -inf / -1
    cand_off, cand_doc = lists(per_query)
    S = bare_score(index, q, "sum", cand_off, cand_doc, 0, n)
    full = index.score(q)
    assert torch.equal(S[0], full[0]) and torch.equal(S[1, :3000], full[1, ::2]) and bool(torch.isnan(S[1, 3000:]).all())
    tv, ti = CS.topk_of_positions(S, k, cand_off, cand_doc)
    v, i = bare_search(index, q, "sum", cand_off, cand_doc, n, k, 2048)
    assert torch.equal(v.cpu(), tv) and torch.equal(i.cpu(), ti)
    assert bool((i[1, 3000:] == -1).all()) and bool((i[1, :3000] % 2 == 0).all())


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_search_pruned_end_to_end(pool, tmp_path):
    C, k = 16, 10
    q, passages, index = corpus("d24", 5)
    pruned = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, NP, index.d)
    cen = torch.from_numpy(np.random.default_rng(8).integers(-4, 5, size=(C, index.d)).astype(np.float32) / 4.0)
    pruned.build_centroids(C, centroids=cen)
    real = colbert._real_rows(pruned.blk_rows)
    assert bool((pruned.tok_centroid[~real] == -1).all()) and int(pruned.tok_centroid.max()) < C and int(pruned.tok_centroid[real].min()) >= 0
    # grid centroids against bf16 rows: products exact, fp32 sums of 24 terms compared with float64 -- ties aside, the same argmax
    t64, c64 = pruned.tok[real].double(), pruned.centroids.double()
    s64 = t64 @ c64.T
    got = s64.gather(1, pruned.tok_centroid[real].long().unsqueeze(1))[:, 0]
    tol = 2 * pruned.dp * 2.0 ** -23 * (t64.abs() @ c64.abs().T).max(1).values  # two fp32 dot products of dp exact products each
    assert bool((got >= s64.max(1).values - tol).all())
    off, docs = CS.lists_from_assignment(pruned.tok_centroid.cpu(), pruned.doc_blk.cpu(), C)
    assert pruned.cen_off.tolist() == off and pruned.cen_doc.tolist() == docs
    # every centroid probed: every passage with a token is a candidate, and the search is the exhaustive one where scores are positive
    cand_off, cand_doc = pruned.candidates(q, C)
    with_tokens = [j for j, p in enumerate(passages) if p.shape[0]]
    assert cand_off.tolist() == [len(with_tokens) * n for n in range(6)] and cand_doc.tolist() == with_tokens * 5
    ev, ei = index.search(q, k, query_pool=pool)
    assert bool((ev > 0).all())  # k = 10 of 36 passages with tokens: every returned score is positive
    v, i = pruned.search_pruned(q, k, C, query_pool=pool)
    assert torch.equal(v, ev) and torch.equal(i, ei)
    # two centroids per query token: the exhaustive scores restricted to the candidates
    cand_off, cand_doc = pruned.candidates(q, 2)
    live = (q != 0).any(2)
    off, docs = CS.union_of_lists(pruned.probe(q, 2).cpu(), live, pruned.cen_off.tolist(), pruned.cen_doc.tolist())
    assert cand_off.tolist() == off and cand_doc.tolist() == docs
    full = exhaustive("d24", pool, 5)
    masked = torch.full_like(full, float("nan")).cpu()
    for n in range(5):
        mine = docs[off[n]:off[n + 1]]
        masked[n, :len(mine)] = full[n, mine].cpu()
    tv, ti = CS.topk_of_positions(masked[:, :max(1, max(off[n + 1] - off[n] for n in range(5)))], k, cand_off, cand_doc)
    for chunk in (None, 8):
        v, i = pruned.search_pruned(q, k, 2, query_pool=pool, chunk=chunk)
        assert torch.equal(v.cpu(), tv) and torch.equal(i.cpu(), ti), chunk
    # a saved and reloaded set of centroids searches bit-identically
    other = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, NP, index.d).load_centroids(pruned.save_centroids(str(tmp_path / "c.pkl")))
    v2, i2 = other.search_pruned(q, k, 2, query_pool=pool)
    assert torch.equal(v2, v) and torch.equal(i2, i) and torch.equal(other.probe(q, 3), pruned.probe(q, 3))


def test_trained_centroids_on_the_device_are_seeded():
    q, passages, index = corpus("d128")
    a = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, NP, index.d).build_centroids(32, iters=3, seed=4)
    b = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, NP, index.d).build_centroids(32, iters=3, seed=4)
    assert torch.equal(a.centroids, b.centroids) and torch.equal(a.tok_centroid, b.tok_centroid) and torch.equal(a.cen_doc, b.cen_doc)
    assert bool(((a.centroids.float().norm(dim=1) - 1).abs() < 2 ** -7).all())
    v, i = a.search_pruned(q, 10, 32)
    ev, ei = index.search(q, 10)
    assert bool((ev > 0).all()) and torch.equal(v, ev) and torch.equal(i, ei)
