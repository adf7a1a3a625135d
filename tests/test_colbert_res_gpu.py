"""The residual-compressed ColBERT index on the MI355X (csrc/colbert_res.h through dprhot_colbert_res_encode / _score / _search) and
ColBERTResidualIndex end to end.

The yardstick is `decode()`: the dense ColBERTIndex over the rows decoded in torch, searched by the dense candidate kernel.  Every
comparison is torch.equal -- of the raw bit patterns where a window holds NaN cells -- and there is no tolerance in this file: the
bf16 fed to the MFMA is the decoded row's, in the same k order.  The lossless grid case at the end checks the rule itself, against the
uncompressed index.  S, the codes, values, indices and the workspace of the bare calls are exactly sized and sit between 4 KiB guard
bands.  Every list and index is one the contract allows; nothing here provokes a fault."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _colbert_res_standin as RS  # noqa: E402
from dpr_scale_amd import colbert  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
BF16 = torch.bfloat16
NP, C, NQ = 30, 16, 4
LENGTHS = [int(x) for x in np.random.default_rng(5).permutation(np.resize(np.array([0, 1, 15, 16, 17, 33, 40]), NP))]
POOL = {"sum": 0, "max": 1}


def _unit(seed, n, d):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1)


@functools.lru_cache(maxsize=None)
def dense_index(d):
    """30 passages of unit-norm gaussian rows (empty, one-block and three-block ones) under 16 given centroids, two of them equal."""
    dense = colbert.ColBERTIndex(list(range(NP)), LENGTHS, _unit(100 + d, sum(LENGTHS), d), NP, DEV)
    cen = _unit(200 + d, C, d)
    cen[5] = cen[2]
    return dense.build_centroids(C, centroids=cen)


@functools.lru_cache(maxsize=None)
def built(d, nbits):
    """(res, dec): the compressed index under trained buckets and its decode(), the reference of every case.  Never modified."""
    res = dense_index(d).compress(nbits)
    return res, res.decode()


def queries(d, LQ, seed=7):
    q = torch.randn(NQ, LQ, d, generator=torch.Generator().manual_seed(seed + LQ))
    q[0, LQ - 1:] = 0.0  # one padded query token
    return q


def lists(per_query):
    off = np.cumsum([0] + [len(x) for x in per_query])
    flat = [j for x in per_query for j in x]
    return torch.tensor(off, dtype=torch.int64, device=DEV), torch.tensor(flat, dtype=torch.int32, device=DEV)


def bits(x):
    return x.contiguous().view(torch.int32)


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


def _res_head(res, qb, pool, cand_off, cand_doc):
    nq, LQ, dp = qb.shape
    return (_p(res.res_code), _p(res.tok_centroid), _p(res.centroids), res.centroids.shape[0], _p(res.weights), res.nbits, _p(res.doc_blk),
            res.n_blk, res.corpus_len, dp, _p(qb), nq, LQ, POOL[pool], _p(cand_off), _p(cand_doc), cand_doc.shape[0])


def _dense_head(dec, qb, pool, cand_off, cand_doc):
    nq, LQ, dp = qb.shape
    return (_p(dec.tok), _p(dec.doc_blk), dec.n_blk, dec.corpus_len, dp, _p(qb), nq, LQ, POOL[pool], _p(cand_off), _p(cand_doc),
            cand_doc.shape[0])


def bare_window(index, q, pool, cand_off, cand_doc, pos_begin, cols, ld):
    """dprhot_colbert_res_score (a residual index) or dprhot_colbert_cand_score (a dense one) through ctypes alone into a window of an
    exactly sized, pre-filled S [nq, ld] between guard bands."""
    from dpr_scale_amd import _lib

    qb = colbert._bf16_padded(q.to(DEV), index.dp)
    raws = []
    S = _banded(raws, qb.shape[0] * ld * 4).view(torch.float32).view(qb.shape[0], ld)
    S.fill_(-3.5)
    if isinstance(index, colbert.ColBERTResidualIndex):
        rc = _lib.lib.dprhot_colbert_res_score(*_res_head(index, qb, pool, cand_off, cand_doc), pos_begin, cols, _p(S), ld, _stream())
    else:
        rc = _lib.lib.dprhot_colbert_cand_score(*_dense_head(index, qb, pool, cand_off, cand_doc), pos_begin, cols, _p(S), ld, _stream())
    _lib.check(rc, "score")
    _check_bands(raws)
    return S.clone()


CASES = [(nbits, d) for nbits in (1, 2, 4) for d in (24, 128)] + [(2, 64), (4, 96)]  # dp = 32 and 128 for every nbits; 64 and 96 once


@pytest.mark.parametrize("nbits,d", CASES)
def test_scores_of_random_rows_equal_the_decoded_index_bit_for_bit(nbits, d):
    """Unit-norm gaussian rows under trained buckets: centroid + weight has to be ROUNDED to bf16 nearly everywhere, so a decode that
    rounds differently (or adds in another precision) cannot pass."""
    res, dec = built(d, nbits)
    assert res.dp == (d + 31) // 32 * 32 and res.res_code.shape == (res.n_blk * 16, res.dp * nbits // 8)
    assert torch.equal(dec.tok, RS.decode_rule(res.res_code, res.tok_centroid, res.centroids, res.weights, nbits))
    exact = res.centroids[res.tok_centroid.clamp(min=0).long()].float() + res.weights[colbert.res_unpack(res.res_code, nbits)]
    real = res.tok_centroid >= 0  # a bf16 centroid plus an fp32 weight fits bf16 only by coincidence: the rounding matters
    assert float((exact[real][:, :d] != dec.tok[real][:, :d].float()).float().mean()) > 0.25
    cand_off, cand_doc = lists([list(range(NP))] * NQ)
    for LQ in (1, 17, 32, 65):  # 65: five fragments, two passes of query fragments
        q = queries(d, LQ)
        for pool in ("sum", "max"):
            S = res.score_candidates(q, cand_off, cand_doc, pool)
            want = dec.score_candidates(q, cand_off, cand_doc, pool)
            assert S.shape == (NQ, NP) and not bool(torch.isnan(S).any())
            assert torch.equal(S, want), (LQ, pool, float((S - want).abs().max()))
    assert not S[:, [j for j, n in enumerate(LENGTHS) if n == 0]].any()  # a passage without tokens scores 0


@pytest.mark.parametrize("nbits,d", [(1, 128), (2, 24), (4, 128)])
def test_ragged_and_hostile_lists_give_the_dense_kernels_window(nbits, d):
    """An empty list, -1 and out-of-corpus doc ids, a duplicate, a cand_off pair beyond n_cand and a decreasing pair; a window with
    pos_begin > 0, cols no multiple of 32 and ld > cols.  The cells outside the window stay as they were and NaN stands exactly where
    the dense kernel writes NaN: the bit patterns of the whole S are compared."""
    res, dec = built(d, nbits)
    long_list = [j % NP for j in range(7, 52)]  # 45 entries (two runs of 32 positions), ids repeating
    flat = [-1, NP, 3, 3, 2 ** 31 - 1, 11] + long_list
    cand_doc = torch.tensor(flat, dtype=torch.int32, device=DEV)
    cand_off = torch.tensor([0, 0, 6, 99, 5], dtype=torch.int64, device=DEV)  # empty; 6 entries; 6 .. n_cand (99 is clamped); 99 > 5: empty
    q = queries(d, 17)
    for pool in ("sum", "max"):
        for pos_begin, cols, ld in ((0, 45, 45), (3, 37, 41), (40, 9, 12)):
            got = bare_window(res, q, pool, cand_off, cand_doc, pos_begin, cols, ld)
            want = bare_window(dec, q, pool, cand_off, cand_doc, pos_begin, cols, ld)
            assert torch.equal(bits(got), bits(want)), (pool, pos_begin, cols, ld)
            assert bool((got[:, cols:] == -3.5).all())
            if pos_begin == 0:
                assert bool(torch.isnan(got[0]).all()) and bool(torch.isnan(got[3]).all())
                assert torch.isnan(got[1, :6]).tolist() == [True, True, False, False, True, False] and bool(torch.isnan(got[1, 6:]).all())
                assert float(got[1, 2]) == float(got[1, 3]) and not bool(torch.isnan(got[2]).any())
    S = res.score_candidates(q, cand_off, cand_doc)
    assert S.shape == (NQ, 45) and torch.equal(bits(S), bits(dec.score_candidates(q, cand_off, cand_doc)))


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_a_hostile_index_decodes_to_zero_rows_and_never_indexes_with_its_ids(nbits):
    """tok_centroid entries >= C and = -1 on real rows, and padding rows whose code bytes are 0xFF, through from_packed: equal to decode(),
    where those rows are exact zeros."""
    d = 128
    res, _ = built(d, nbits)
    tc, code = res.tok_centroid.clone(), res.res_code.clone()
    real = torch.nonzero(tc >= 0).reshape(-1)
    code[tc < 0] = 0xFF
    for i, bad in enumerate((C, C + 5, 2 ** 31 - 1, -1, -(2 ** 31))):
        tc[real[i::7]] = bad
    hostile = colbert.ColBERTResidualIndex.from_packed(code, tc, res.centroids, res.cutoffs, res.weights, res.doc_blk, NP, d,
                                                       cen_off=res.cen_off, cen_doc=res.cen_doc)
    dec = hostile.decode()
    assert not dec.tok[(tc < 0) | (tc >= C)].any() and bool(dec.tok[(tc >= 0) & (tc < C)].any())
    assert float(((tc < 0) | (tc >= C))[real].float().mean()) > 0.5
    cand_off, cand_doc = lists([list(range(NP))] * NQ)
    q = queries(d, 33)
    for pool in ("sum", "max"):
        assert torch.equal(hostile.score_candidates(q, cand_off, cand_doc, pool), dec.score_candidates(q, cand_off, cand_doc, pool))
    for a, b in zip(hostile.search_pruned(q, 6, 3), dec.search_pruned(q, 6, 3)):
        assert torch.equal(a, b)
    for a, b in zip(hostile.search_pruned(q, 3, 3, ndocs=4), dec.search_pruned(q, 3, 3, ndocs=4)):  # doc_centroids skips the ids too
        assert torch.equal(a, b)


@pytest.mark.parametrize("nbits,d", [(1, 24), (2, 128), (4, 64)])
def test_encode_is_the_rule_writes_every_byte_and_nothing_else(nbits, d):
    from dpr_scale_amd import _lib, hotpath

    dense = dense_index(d)
    res, _ = built(d, nbits)
    rows, tc = dense.tok.clone(), dense.tok_centroid.clone()
    real = torch.nonzero(tc >= 0).reshape(-1)
    rows[real[0], 3] = float("nan")                       # a NaN residual encodes as 0
    rows[real[1]] = (dense.centroids[tc[real[1]].long()].float() + res.cutoffs[0]).to(BF16)  # residuals at (or a rounding from) a cutoff
    tc[real[2]], tc[real[3]] = C, 2 ** 31 - 1             # ids outside [0, C): zero bytes
    want = RS.encode_rule(rows, tc, dense.centroids, res.cutoffs, nbits)
    n, rb = rows.shape[0], dense.dp * nbits // 8
    assert n * dense.dp // 8 > 256 and not want[real[2]].any() and not want[tc < 0].any() and bool(want.any())
    raws = []
    out = _banded(raws, n * rb).view(n, rb)
    runs = []
    for _ in range(2):
        out.fill_(0x5A)
        _lib.check(_lib.lib.dprhot_colbert_res_encode(_p(rows), _p(tc), n, dense.dp, _p(dense.centroids), C, _p(res.cutoffs), nbits, _p(out),
                                                      _stream()), "dprhot_colbert_res_encode")
        _check_bands(raws)
        runs.append(out.clone())
    assert torch.equal(runs[0], want) and torch.equal(runs[1], runs[0])
    assert torch.equal(hotpath.default_kernels().colbert_res_encode(rows, res.cutoffs, nbits, tc, dense.centroids), want)
    assert torch.equal(res.res_code, RS.encode_rule(dense.tok, dense.tok_centroid, dense.centroids, res.cutoffs, nbits))  # compress itself


@pytest.mark.parametrize("nbits,d", [(1, 128), (2, 128), (4, 24)])
def test_search_pruned_end_to_end_equals_the_decoded_index(nbits, d):
    from dpr_scale_amd import _lib

    res, dec = built(d, nbits)
    q = queries(d, 33)
    cand_off, _ = res.candidates(q, 2)
    longest = int((cand_off[1:] - cand_off[:-1]).max())
    assert 4 < longest < NP
    for pool in ("sum", "max"):
        for k, nprobe, chunk, ndocs in ((1, 2, None, None), (5, 2, 8, None), (NP, 2, 8, None), (NP, 1, None, None), (4, 2, 8, longest - 3),
                                        (4, 2, None, longest + 3), (5, C, 8, 6)):
            got = res.search_pruned(q, k, nprobe, pool, chunk=chunk, ndocs=ndocs)
            want = dec.search_pruned(q, k, nprobe, pool, chunk=chunk, ndocs=ndocs)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (pool, k, nprobe, chunk, ndocs)
            assert got[0].shape == (NQ, k) and got[1].dtype == torch.int64
            if k == NP:  # more than any list holds: -inf / -1 tails
                assert bool((got[0][:, -1] == float("-inf")).all()) and bool((got[1][:, -1] == -1).all())
    # the bare entry point: values, indices and an exactly sized workspace between guard bands
    qb = colbert._bf16_padded(q.to(DEV), res.dp)
    cand_off, cand_doc = res.candidates(q, 2)
    n = ctypes.c_size_t(0)
    _lib.check(_lib.lib.dprhot_colbert_cand_workspace_bytes(NQ, 8, ctypes.byref(n)))
    raws = []
    values = _banded(raws, NQ * 5 * 4).view(torch.float32).view(NQ, 5)
    indices = _banded(raws, NQ * 5 * 8).view(torch.int64).view(NQ, 5)
    ws = _banded(raws, n.value)
    _lib.check(_lib.lib.dprhot_colbert_res_search(*_res_head(res, qb, "sum", cand_off, cand_doc), longest, 5, 8, _p(values), _p(indices), _p(ws),
                                                  n.value, _stream()), "dprhot_colbert_res_search")
    _check_bands(raws)
    want = dec.search_pruned(q, 5, 2, chunk=8)
    assert torch.equal(values, want[0]) and torch.equal(indices, want[1])


def test_search_pruned_above_k_4096_takes_the_wide_selection():
    """4200 one-token passages under 4 centroids, every centroid probed: k = 4100 candidates per query through the wide selection."""
    n, d, k = 4200, 32, 4100
    dense = colbert.ColBERTIndex(list(range(n)), [1] * n, _unit(31, n, d), n, DEV).build_centroids(4, centroids=_unit(32, 4, d))
    res = dense.compress(2)
    dec = res.decode()
    q = torch.randn(2, 3, d, generator=torch.Generator().manual_seed(33))
    got, want = res.search_pruned(q, k, 4), dec.search_pruned(q, k, 4)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool((got[1] >= 0).all()) and all(len(set(r)) == k for r in got[1].tolist())


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_a_lossless_grid_equals_the_uncompressed_index(nbits):
    """Rows, centroids and weights are multiples of 1/8 and every row IS centroid + weight: encode recovers the weight's index, decode
    the row, and the residual search_pruned equals the search_pruned of the index that was never compressed -- the rule itself, not only
    self-consistency."""
    d, nb = 32, 1 << nbits
    g = torch.Generator().manual_seed(40 + nbits)
    weights = (torch.arange(nb, dtype=torch.float32) * 2 - (nb - 1)) / 8      # odd multiples of 1/8 ...
    cutoffs = (weights[1:] + weights[:-1]) / 2                                # ... with the cutoffs half way
    cen = torch.randint(-8, 9, (C, d), generator=g).float() / 8
    cen[5] = cen[2]
    total = sum(LENGTHS)
    assign = torch.randint(0, C, (total,), generator=g)
    pick = torch.randint(0, nb, (total, d), generator=g)
    rows = cen[assign] + weights[pick]
    assert torch.equal(rows.to(BF16).float(), rows)
    dense = colbert.ColBERTIndex(list(range(NP)), LENGTHS, rows, NP, DEV)
    tok_centroid = torch.full((dense.n_blk * 16,), -1, dtype=torch.int32, device=DEV)
    dest = colbert._dest_rows(dense.doc_blk, torch.arange(NP, device=DEV), torch.tensor(LENGTHS, device=DEV))
    tok_centroid[dest] = assign.to(DEV, torch.int32)
    cen_dev = cen.to(DEV, BF16)
    dense._set_centroids(cen_dev, tok_centroid, *colbert._centroid_lists(tok_centroid, dense.doc_blk, C, NP))
    res = dense.compress(nbits, buckets=(cutoffs, weights))
    assert torch.equal(colbert.res_unpack(res.res_code, nbits)[dest], pick.to(DEV)) and torch.equal(res.decode().tok, dense.tok)
    q = (torch.randint(-8, 9, (NQ, 17, d), generator=g).float() / 8)
    cand_off, cand_doc = lists([list(range(NP))] * NQ)
    for pool in ("sum", "max"):
        assert torch.equal(res.score_candidates(q, cand_off, cand_doc, pool), dense.score_candidates(q, cand_off, cand_doc, pool))
        assert torch.equal(res.score_candidates(q, cand_off, cand_doc, pool), dense.score(q, query_pool=pool))
        for k, nprobe, ndocs in ((5, 2, None), (NP, 1, None), (3, 4, 5)):
            got, want = res.search_pruned(q, k, nprobe, pool, ndocs=ndocs), dense.search_pruned(q, k, nprobe, pool, ndocs=ndocs)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (pool, k, nprobe, ndocs)


def test_streaming_build_on_the_device_equals_the_one_shot_build():
    d = 40
    passages = list(torch.split(_unit(50, sum(LENGTHS), d).to(BF16), LENGTHS))
    b = colbert.TokenIndexBuilder(NP, device=DEV)
    for sel in (list(range(0, 11)), list(range(11, 12)), list(range(12, NP))):
        L = max(max(LENGTHS[j] for j in sel), 1)
        x, att = torch.zeros(len(sel), L, d, dtype=BF16), torch.zeros(len(sel), L)
        for r, j in enumerate(sel):
            x[r, :LENGTHS[j]], att[r, :LENGTHS[j]] = passages[j], 1
        b.add(x, att, sel)
    res = b.finish(quantizer="residual", nbits=2, n_centroids=8, iters=2, seed=1)
    assert type(res) is colbert.ColBERTResidualIndex and res.device.type == "cuda" and res.dp == 64
    dense = b.finish().build_centroids(8, centroids=res.centroids[:, :d])
    want = dense.compress(2, buckets=(res.cutoffs, res.weights))
    for (name, a), w in zip(res._tensors().items(), want._tensors().values()):
        assert a.dtype == w.dtype and torch.equal(a, w), name
    q = queries(d, 17)
    for a, w in zip(res.search_pruned(q, 5, 2, ndocs=6), want.decode().search_pruned(q, 5, 2, ndocs=6)):
        assert torch.equal(a, w)


@pytest.mark.parametrize("nbits,d", [(1, 32), (2, 128), (4, 64)])
def test_an_index_without_a_token_block_scores_zero_for_present_candidates(nbits, d):
    """n_blk == 0 (every passage empty): the ABI admits NULL res_code, tok_centroid, centroids and weights; a present candidate scores
    0, every other cell is NaN, as the dense kernel writes for the same empty index."""
    from dpr_scale_amd import _lib

    n = 5
    doc_blk = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    cand_doc = torch.tensor([0, 3, -1, n, 4, 2], dtype=torch.int32, device=DEV)
    cand_off = torch.tensor([0, 4, 4, 6, 6], dtype=torch.int64, device=DEV)  # 4 entries (two of them no passage); none; 2; none
    q = queries(d, 17)
    qb = colbert._bf16_padded(q.to(DEV), d)
    dense = colbert.ColBERTIndex.from_packed(torch.zeros((0, d), dtype=BF16, device=DEV), doc_blk, n, d)
    for pool in ("sum", "max"):
        raws = []
        S = _banded(raws, NQ * 5 * 4).view(torch.float32).view(NQ, 5)
        S.fill_(-3.5)
        _lib.check(_lib.lib.dprhot_colbert_res_score(None, None, None, 4, None, nbits, _p(doc_blk), 0, n, d, _p(qb), NQ, 17, POOL[pool],
                                                     _p(cand_off), _p(cand_doc), 6, 0, 4, _p(S), 5, _stream()), "dprhot_colbert_res_score")
        _check_bands(raws)
        assert S[0, :2].tolist() == [0.0, 0.0] and S[2, :2].tolist() == [0.0, 0.0] and bool((S[:, 4] == -3.5).all())
        assert bool(torch.isnan(S[0, 2:4]).all()) and bool(torch.isnan(S[1, :4]).all()) and bool(torch.isnan(S[2, 2:4]).all())
        assert bool(torch.isnan(S[3, :4]).all())
        assert torch.equal(bits(S[:, :4]), bits(bare_window(dense, q, pool, cand_off, cand_doc, 0, 4, 4)))
    # the same through the product, whose empty tensors reach the library as NULL, and the search entry: 0 for the present ones, then tails
    cen = _unit(9, 4, d).to(DEV, BF16)
    cutoffs, weights = torch.zeros((1 << nbits) - 1, device=DEV), torch.zeros(1 << nbits, device=DEV)
    res = colbert.ColBERTResidualIndex.from_packed(torch.zeros((0, d * nbits // 8), dtype=torch.uint8, device=DEV),
                                                   torch.zeros(0, dtype=torch.int32, device=DEV), cen, cutoffs, weights, doc_blk, n, d)
    got = res.score_candidates(q, cand_off, cand_doc)
    assert got.shape == (NQ, 4) and torch.equal(bits(got), bits(S[:, :4]))
    v, i = res._search_candidates(qb, 0, 3, cand_off, cand_doc, 4)
    assert v[0].tolist() == [0.0, 0.0, float("-inf")] and i[0].tolist() == [0, 3, -1] and i[2].tolist() == [4, 2, -1]
    assert bool((i[1] == -1).all()) and bool((i[3] == -1).all())
