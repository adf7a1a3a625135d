"""The centroid-interaction stage on the MI355X (csrc/colbert_cen.h through dprhot_colbert_cen_table / _score / _search) and
ColBERTIndex.search_pruned(ndocs=) end to end.

The yardstick is the exhaustive kernel.  A table column must be BIT-EQUAL to the scores dprhot_colbert_score writes for a
one-token-per-passage index of the centroids under a query that is zero except one token, and an approximate cell must be BIT-EQUAL to
the cell dprhot_colbert_score writes for the index rebuilt from centroids[tok_centroid] (torch.equal, no tolerance), whatever the
list, the window and the other queries are.  Against the float64 definition on gaussian queries the derived per-cell bound of
tests/test_colbert_gpu.py holds with centroid rows for token rows -- the arithmetic is the same:
    bound[n, doc] = (dp + LQ + 1) * 2^-23 * A[n, doc],   A[n, doc] = sum_i max_j sum_k |q_ik c_jk|
`cen_search` is compared with the total-order top-k of the kernel's own `cen_score` matrix mapped to doc ids, with torch.equal.
T, S, values, indices and the workspace are exactly sized and sit between 4 KiB guard bands.  Every list is valid; nothing here
provokes a fault."""
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
import _colbert_cen_standin as CE  # noqa: E402
import _colbert_oracle as CO  # noqa: E402
from dpr_scale_amd import colbert  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
LENGTHS = [0, 1, 15, 16, 17, 31, 33, 64, 65, 180, 513]
NP, C = 40, 300
SHAPES = {  # d (dp), nq, LQ (LT), poolings
    "d24": (24, 5, 7, ("sum", "max")),       # dp = 32; LT = 16: a partial fragment, 4 pieces per table row
    "d128": (128, 3, 33, ("sum", "max")),    # dp = 128; LT = 48: 12 pieces on 16 lanes
    "d160": (160, 2, 16, ("sum",)),          # dp = 160: the any-width table kernel
    "d32-long": (32, 2, 260, ("sum",)),      # LT = 272: a 1088-byte table row, two passes over every list
}
SHAPE_POOLS = [(s, p) for s, v in SHAPES.items() for p in v[3]]
RAGGED = [[], [10], list(range(NP)), list(range(1, 39, 2)), [0]]  # the RAGGED lists of tests/test_colbert_cand_gpu.py


def twin_of(index):
    """The index of the same doc_blk whose token rows are centroids[tok_centroid], zero rows on padding."""
    tc = index.tok_centroid.long()
    tok = index.centroids[tc.clamp(min=0)] * (tc >= 0).unsqueeze(1)
    return colbert.ColBERTIndex.from_packed(tok.contiguous(), index.doc_blk, index.corpus_len, index.d)


@functools.lru_cache(maxsize=None)
def corpus(shape, nq=None):
    """(q, index, twin) of a shape: 40 gaussian bf16-exact passages of LENGTHS repeated (doc id = position) under C = 300 given grid
    centroids (integers in -4 .. 4 divided by 4), and the twin index whose token rows are centroids[tok_centroid]."""
    d, nq0, LQ, _ = SHAPES[shape]
    nq = nq0 if nq is None else nq
    g = torch.Generator().manual_seed(2000 + d + LQ)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    lengths = [int(x) for x in np.resize(np.array(LENGTHS), NP)]
    rows = rnd(sum(lengths), d)
    q = rnd(nq, LQ, d)
    q[0, LQ - 1:] = 0.0  # one padded query token
    index = colbert.ColBERTIndex(list(range(NP)), lengths, rows, NP, DEV)
    cen = torch.from_numpy(np.random.default_rng(d + LQ).integers(-4, 5, size=(C, d)).astype(np.float32) / 4.0)
    index.build_centroids(C, centroids=cen)
    return q, index, twin_of(index)


@functools.lru_cache(maxsize=None)
def twin_scores(shape, pool, nq=None):
    """The exhaustive kernel's score matrix [nq, 40] over the twin index: the reference of every approximate cell.  Never modified."""
    q, _, twin = corpus(shape, nq)
    return twin.score(q, 0, None, pool)


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


def bare_table(index, q):
    """dprhot_colbert_cen_table through ctypes alone into an exactly sized T [nq, C, LT] between guard bands."""
    from dpr_scale_amd import _lib

    qb = colbert._bf16_padded(q.to(DEV), index.dp)
    nq, LQ, dp = qb.shape
    n_cen, LT = int(index.centroids.shape[0]), (LQ + 15) // 16 * 16
    raws = []
    T = _banded(raws, nq * n_cen * LT * 4).view(torch.float32).view(nq, n_cen, LT)
    _lib.check(_lib.lib.dprhot_colbert_cen_table(_p(index.centroids), n_cen, dp, _p(qb), nq, LQ, _p(T), _stream()), "dprhot_colbert_cen_table")
    _check_bands(raws)
    return T.clone()


def _head(index, T, LQ, pool, cand_off, cand_doc):
    doc_cen_off, doc_cen = index.doc_centroids()
    return (_p(doc_cen_off), _p(doc_cen), doc_cen.shape[0], index.corpus_len, T.shape[1], _p(T), T.shape[0], LQ, CO.POOL[pool], _p(cand_off),
            _p(cand_doc), cand_doc.shape[0])


def bare_score(index, T, LQ, pool, cand_off, cand_doc, pos_begin, cols):
    """dprhot_colbert_cen_score through ctypes alone into an exactly sized S [nq, cols] between guard bands."""
    from dpr_scale_amd import _lib

    raws = []
    S = _banded(raws, T.shape[0] * cols * 4).view(torch.float32).view(T.shape[0], cols)
    _lib.check(_lib.lib.dprhot_colbert_cen_score(*_head(index, T, LQ, pool, cand_off, cand_doc), pos_begin, cols, _p(S), cols, _stream()),
               "dprhot_colbert_cen_score")
    _check_bands(raws)
    return S.clone()


def bare_search(index, T, LQ, pool, cand_off, cand_doc, max_count, k, chunk):
    """dprhot_colbert_cen_search through ctypes alone: values, indices and an exactly sized workspace sit between guard bands."""
    from dpr_scale_amd import _lib

    nq = T.shape[0]
    n = ctypes.c_size_t(0)
    _lib.check(_lib.lib.dprhot_colbert_cen_workspace_bytes(nq, chunk, ctypes.byref(n)))
    nws = n.value
    if k > 4096:
        _lib.check(_lib.lib.dprhot_topk_wide_workspace_bytes(nq, k, ctypes.byref(n)))
        nws += n.value
    raws = []
    values = _banded(raws, nq * k * 4).view(torch.float32).view(nq, k)
    indices = _banded(raws, nq * k * 8).view(torch.int64).view(nq, k)
    ws = _banded(raws, nws)
    _lib.check(_lib.lib.dprhot_colbert_cen_search(*_head(index, T, LQ, pool, cand_off, cand_doc), max_count, k, chunk, _p(values), _p(indices),
                                                  _p(ws), nws, _stream()), "dprhot_colbert_cen_search")
    _check_bands(raws)
    return values.clone(), indices.clone()


@functools.lru_cache(maxsize=None)
def table(shape, nq=None):
    """The kernel's own table of a shape's queries.  Never modified."""
    q, index, _ = corpus(shape, nq)
    return bare_table(index, q)


def test_the_corpus_exercises_what_it_is_meant_to():
    for shape in SHAPES:
        _, index, _ = corpus(shape)
        off = index.doc_centroids()[0].tolist()
        assert off[11] - off[10] > 64, shape  # the 513-token passage: a list longer than one wave's batch of ids
        assert off[1] - off[0] == 0 and off[2] - off[1] == 1  # the passage without tokens has no list; one token, one centroid
        host_off, host_cen = CE.doc_lists_from_assignment(index.tok_centroid.cpu(), index.doc_blk.cpu())
        assert off == host_off and index.doc_centroids()[1].tolist() == host_cen


@pytest.mark.parametrize("shape", list(SHAPES))
def test_table_columns_equal_the_exhaustive_kernel_bit_for_bit(shape):
    q, index, _ = corpus(shape)
    nq, LQ, d = q.shape
    T = table(shape)
    LT = (LQ + 15) // 16 * 16
    assert T.shape == (nq, C, LT) and not T[:, :, LQ:].any()
    assert torch.equal(index.centroid_table(q), T)
    # one passage per centroid, one token each; query (n, i) is zero except token i, which is q[n, i]: its "sum" score of passage c is
    # max(0, <q[n, i], centroid_c>), the product itself where it is positive.  The negated query gives the negated products bit for
    # bit (negation is exact in bf16 and round-to-nearest is symmetric), so the two score matrices hold every product.
    one = colbert.ColBERTIndex(list(range(C)), [1] * C, index.centroids[:, :d].float(), C, DEV)
    single = torch.zeros(nq * LQ, LQ, d)
    single[torch.arange(nq * LQ), torch.arange(nq * LQ) % LQ] = q.reshape(nq * LQ, d)
    pos, neg = one.score(single), one.score(-single)
    assert bool((pos > 0).any()) and bool((neg > 0).any()) and not bool(((pos > 0) & (neg > 0)).any())
    assert torch.equal(T[:, :, :LQ].permute(0, 2, 1).reshape(nq * LQ, C), pos - neg)


@pytest.mark.parametrize("shape,pool", SHAPE_POOLS)
def test_all_candidates_equal_the_exhaustive_matrix_of_the_twin_bit_for_bit(shape, pool):
    q, index, twin = corpus(shape)
    nq, LQ = q.shape[0], q.shape[1]
    want, T = twin_scores(shape, pool), table(shape)
    cand_off, cand_doc = lists([list(range(NP))] * nq)
    S = bare_score(index, T, LQ, pool, cand_off, cand_doc, 0, NP)
    assert torch.equal(S, want)
    assert torch.equal(index.approx_candidates(q, cand_off, cand_doc, pool), want)
    for pos_begin in (0, 8, 24):
        for cols in (8, 13):
            assert torch.equal(bare_score(index, T, LQ, pool, cand_off, cand_doc, pos_begin, cols), want[:, pos_begin:pos_begin + cols]), (pos_begin, cols)
    # the float64 definition, under the bound derived for the exhaustive kernel with centroid rows for token rows
    passages = CE.centroid_passages(index)
    ref = CO.score(q, passages, pool)
    bound = (index.dp + LQ + 1) * 2.0 ** -23 * CO.magnitude(q, passages)
    err = (S.cpu().double() - ref).abs()
    print(f"{shape}/{pool}: max err {err.max().item():.3e}, max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())
    assert not S[:, [j for j, p in enumerate(passages) if p.shape[0] == 0]].any()  # a passage without tokens scores 0
    assert bool((S > 0).any())


@pytest.mark.parametrize("shape,pool", [("d24", "sum"), ("d24", "max"), ("d128", "sum"), ("d128", "max")])
def test_ragged_lists(shape, pool):
    q, index, _ = corpus(shape, 5)
    LQ = q.shape[1]
    want, T = twin_scores(shape, pool, 5), table(shape, 5)
    cand_off, cand_doc = lists(RAGGED)
    width = NP + 3  # a window wider than the longest list: the cells behind a list are written too
    S = bare_score(index, T, LQ, pool, cand_off, cand_doc, 0, width)
    again = bare_score(index, T, LQ, pool, cand_off, cand_doc, 0, width)
    assert torch.equal(S.view(torch.int32), again.view(torch.int32))  # two runs: the same bits, NaN cells included
    for n, mine in enumerate(RAGGED):
        assert torch.equal(S[n, :len(mine)], want[n, mine]), n       # present cells: the all-candidates cells, bit for bit
        assert bool(torch.isnan(S[n, len(mine):]).all()), n          # absent cells: no candidate
    assert float(S[4, 0]) == 0.0
    # absent cells are never selected: a k above a row's count leaves -inf / -1 behind the row's candidates
    v, i = bare_search(index, T, LQ, pool, cand_off, cand_doc, NP, 30, 8)
    for n, mine in enumerate(RAGGED):
        m = min(30, len(mine))
        got = i[n, :m].tolist()
        assert set(got) <= set(mine) and len(set(got)) == m, n
        assert bool((i[n, m:] == -1).all()) and bool((v[n, m:] == float("-inf")).all()) and not bool(torch.isnan(v[n]).any())
    # a cell does not depend on the rest of its list, on the other queries or on the window
    rev_off, rev_doc = lists([list(reversed(RAGGED[3]))])
    alone = bare_score(index, T[3:4].contiguous(), LQ, pool, rev_off, rev_doc, 0, 19)
    assert torch.equal(alone.flip(1), S[3:4, :19])
    off2, doc2 = lists([RAGGED[3][5:9], [10, 7], RAGGED[3]])
    mixed = bare_score(index, T[[3, 1, 3]].contiguous(), LQ, pool, off2, doc2, 0, 19)
    assert torch.equal(mixed[0, :4], S[3, 5:9]) and torch.equal(mixed[2], S[3, :19]) and torch.equal(mixed[1, 0], S[1, 0])
    assert torch.equal(mixed[1, 1], want[1, 7]) and bool(torch.isnan(mixed[1, 2:]).all())
    # windows hold NaN cells: compared as bit patterns (the kernel writes ONE quiet NaN)
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(bare_score(index, T, LQ, pool, cand_off, cand_doc, 11, 7)), bits(S[:, 11:18]))
    assert torch.equal(bits(bare_score(index, T, LQ, pool, cand_off, cand_doc, 32, 9)), bits(S[:, 32:41]))  # a window that begins at a second run


@pytest.mark.parametrize("shape,pool", [("d24", "sum"), ("d128", "max")])
def test_search_is_the_top_k_of_the_kernels_own_scores(shape, pool):
    q, index, _ = corpus(shape, 5)
    LQ, T = q.shape[1], table(shape, 5)
    cand_off, cand_doc = lists(RAGGED)
    S = bare_score(index, T, LQ, pool, cand_off, cand_doc, 0, NP)
    for k in (1, 5, 30):  # 30: above the counts 0, 1, 19 and 1 -- tails of -inf / -1
        tv, ti = CS.topk_of_positions(S, k, cand_off, cand_doc)
        for chunk in (8, 64):
            v, i = bare_search(index, T, LQ, pool, cand_off, cand_doc, NP, k, chunk)
            assert torch.equal(v.cpu(), tv) and torch.equal(i.cpu(), ti), (k, chunk)


def test_wide_selection_over_candidate_lists():
    n, k, n_cen = 6000, 5000, 64
    g = torch.Generator().manual_seed(78)
    lengths = [int(x) for x in np.random.default_rng(6).integers(1, 4, size=n)]
    rows = torch.randn(sum(lengths), 32, generator=g).to(torch.bfloat16).float()
    q = torch.randn(2, 4, 32, generator=g).to(torch.bfloat16).float()
    index = colbert.ColBERTIndex(list(range(n)), lengths, rows, n, DEV)
    index.build_centroids(n_cen, centroids=torch.from_numpy(np.random.default_rng(7).integers(-4, 5, size=(n_cen, 32)).astype(np.float32) / 4.0))
    per_query = [list(range(n)), list(range(0, n, 2))]  # 6000 candidates; 3000: below k, a tail of -inf / -1
    cand_off, cand_doc = lists(per_query)
    T = bare_table(index, q)
    S = bare_score(index, T, 4, "sum", cand_off, cand_doc, 0, n)
    full = twin_of(index).score(q)
    assert torch.equal(S[0], full[0]) and torch.equal(S[1, :3000], full[1, ::2]) and bool(torch.isnan(S[1, 3000:]).all())
    tv, ti = CS.topk_of_positions(S, k, cand_off, cand_doc)
    v, i = bare_search(index, T, 4, "sum", cand_off, cand_doc, n, k, 2048)
    assert torch.equal(v.cpu(), tv) and torch.equal(i.cpu(), ti)
    assert bool((i[1, 3000:] == -1).all()) and bool((i[1, :3000] % 2 == 0).all())


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_search_pruned_with_ndocs_end_to_end(pool, monkeypatch):
    k, ndocs = 10, 12
    q, index, _ = corpus("d24", 5)
    full = index.score(q, 0, None, pool)  # the exhaustive kernel's own matrix
    cand_off, cand_doc = index.candidates(q, 2)
    counts = (cand_off[1:] - cand_off[:-1]).tolist()
    assert max(counts) > ndocs  # the stage runs
    A = index.approx_candidates(q, cand_off, cand_doc, pool)  # the kernel's own approximate matrix
    _, ids = CS.topk_of_positions(A, ndocs, cand_off, cand_doc)
    keep = torch.sort(ids, dim=1).values
    assert torch.equal(index.prune_candidates(q, cand_off, cand_doc, ndocs, pool).cpu().long(), keep)
    masked = torch.full((5, ndocs), float("nan"))
    for n in range(5):
        masked[n, keep[n] >= 0] = full[n, keep[n][keep[n] >= 0].to(DEV)].cpu()
    tv, ti = CS.topk_of_positions(masked, k, torch.arange(6) * ndocs, keep.to(torch.int32).reshape(-1))
    want = None
    for chunk in (None, 8):
        v, i = index.search_pruned(q, k, 2, query_pool=pool, chunk=chunk, ndocs=ndocs)
        assert torch.equal(v.cpu(), tv) and torch.equal(i.cpu(), ti), chunk
        want = (v, i)
    assert index.latency["interaction_time"] > 0
    monkeypatch.setattr(colbert, "CEN_TABLE_BYTES", 1)  # one query per batch
    v, i = index.search_pruned(q, k, 2, query_pool=pool, ndocs=ndocs)
    assert torch.equal(v, want[0]) and torch.equal(i, want[1])
    monkeypatch.undo()
    # ndocs above every count: the call without ndocs
    ev, ei = index.search_pruned(q, k, 2, query_pool=pool)
    v, i = index.search_pruned(q, k, 2, query_pool=pool, ndocs=10 ** 6)
    assert torch.equal(v, ev) and torch.equal(i, ei)
