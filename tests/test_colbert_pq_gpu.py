"""The product-quantised ColBERT token index on the MI355X (csrc/colbert_pq.h through dprhot_colbert_pq_encode / _score / _search;
DESIGN.md section 12.1).

The contract is bit equality, so every check is torch.equal and no tolerance appears: ColBERTPQIndex.score / .search against
decode().score / .search -- the dense kernel of csrc/colbert.h over the decoded rows -- and, on rows drawn from a grid that a codebook
holds without loss, against the UNQUANTISED index.  Every input is valid; nothing here provokes a fault."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _colbert_pq_standin as PS  # noqa: E402
import _pq_oracle as PO  # noqa: E402
from dpr_scale_amd import colbert  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
LENGTHS = PS.GPU_LENGTHS  # [0, 1, 15, 16, 17, 31, 33, 64, 65, 180, 513] and 40 short passages: 51 = three runs of 16 and a run of 3
NQ, LQ = 3, 33
POOLS = {"sum": 0, "max": 1}


def _dense(passages, d):
    rows = torch.cat(passages, 0)
    return colbert.ColBERTIndex(list(range(len(passages))), [p.shape[0] for p in passages], rows, len(passages), DEV)


@functools.lru_cache(maxsize=None)
def case(d, dsub):
    """(q, dense index, its ColBERTPQIndex under a codebook of train_pq(iters=2) on the corpus's own rows, decode()) -- built once."""
    g = torch.Generator().manual_seed(1000 * d + dsub)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    passages = [rnd(n, d) for n in LENGTHS]
    q = rnd(NQ, LQ, d)
    q[0, LQ - 2:] = 0.0
    dense = _dense(passages, d)
    pq = dense.quantize(dsub=dsub, iters=2)
    return q, dense, pq, pq.decode()


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


def _head(pq, qb, pool):
    nq, lq, dp = qb.shape
    return (_p(pq.tok_code), _p(pq.blk_rows), _p(pq.codebook), pq.dsub, _p(pq.doc_blk), pq.n_blk, pq.corpus_len, dp, _p(qb), nq, lq, pool)


@pytest.mark.parametrize("pool", ["sum", "max"])
@pytest.mark.parametrize("dsub", [2, 4, 8])
@pytest.mark.parametrize("d", [24, 96, 128])
def test_score_and_search_equal_the_dense_kernel_over_decode(d, dsub, pool):
    q, dense, pq, dec = case(d, dsub)
    n = len(LENGTHS)
    assert pq.dp == (d + 31) // 32 * 32 and pq.n_blk == dense.n_blk and torch.equal(pq.blk_rows, dense.blk_rows)
    S = pq.score(q, 0, None, pool)
    assert S.shape == (NQ, n) and torch.equal(S, dec.score(q, 0, None, pool))
    assert not S[:, 0].any() and bool((S[:, 1:] >= 0).all())  # the empty passage; the clamp
    assert torch.equal(pq.score(q, 3, 5, pool), dec.score(q, 3, 5, pool)) and torch.equal(pq.score(q, 3, 5, pool), S[:, 3:8])
    for k in (1, 7, n):
        for kw in (dict(chunk=8), dict(), dict(chunk=8, id_ranges=[(0, 5), (5, 11)])):
            if "id_ranges" in kw and k > 11:
                continue
            (v, i), (dv, di) = pq.search(q, k, query_pool=pool, **kw), dec.search(q, k, query_pool=pool, **kw)
            assert torch.equal(v, dv) and torch.equal(i, di), (k, kw)


@pytest.mark.parametrize("dsub", [2, 4, 8])
def test_lossless_grid_equals_the_unquantised_search(dsub):
    q, passages = PS.grid_corpus(dsub)
    dense = _dense(passages, 128)
    pq = dense.quantize(dsub=dsub, iters=2, train_size=dense.tok.shape[0])
    assert torch.equal(pq.decode().tok, dense.tok)
    for pool in ("sum", "max"):
        assert torch.equal(pq.score(q, 0, None, pool), dense.score(q, 0, None, pool))
        for k in (1, 7, len(passages)):
            (v, i), (dv, di) = pq.search(q, k, query_pool=pool), dense.search(q, k, query_pool=pool)
            assert torch.equal(v, dv) and torch.equal(i, di)


@pytest.mark.parametrize("lq", [130, 260, 512])
def test_long_queries_one_pass(lq):
    """9, 17 and 32 fragments per query: one query per workgroup, the widest term table."""
    _, dense, pq, dec = case(128, 2)
    q = torch.randn(2, lq, 128, generator=torch.Generator().manual_seed(lq)).to(torch.bfloat16).float()
    for pool in ("sum", "max"):
        assert torch.equal(pq.score(q, 0, None, pool), dec.score(q, 0, None, pool))


@pytest.mark.parametrize("nq,lq", [(1, 4), (1, 33), (2, 20), (5, 7), (7, 16), (8, 16)])
def test_few_fragments_share_the_passages_among_the_waves(nq, lq):
    """1, 3, 4, 5 and 7 fragments in the workgroup: 8, 2, 2, 1 and 1 waves per fragment (idle waves at 3, 5 and 7); 8: one each."""
    for d, dsub in ((24, 2), (128, 8)):
        _, dense, pq, dec = case(d, dsub)
        q = torch.randn(nq, lq, d, generator=torch.Generator().manual_seed(nq * lq)).to(torch.bfloat16).float()
        for pool in ("sum", "max"):
            assert torch.equal(pq.score(q, 0, None, pool), dec.score(q, 0, None, pool))
            assert torch.equal(pq.score(q, 3, 5, pool), dec.score(q, 3, 5, pool))


@pytest.mark.parametrize("n", [40000, 140000])
def test_many_short_passages_several_runs_per_workgroup(n):
    """2500 and 8750 runs of 16 passages in one chunk: two and eight runs per workgroup, a ragged last workgroup."""
    g = torch.Generator().manual_seed(n)
    lens = torch.randint(0, 4, (n,), generator=g)
    rows = torch.randn(int(lens.sum()), 32, generator=g).to(torch.bfloat16)
    dense = colbert.ColBERTIndex(torch.arange(n), lens, rows, n, DEV)
    pq = dense.quantize(dsub=8, iters=1, train_size=4096)
    dec = pq.decode()
    q = torch.randn(2, 4, 32, generator=g).to(torch.bfloat16).float()
    assert torch.equal(pq.score(q), dec.score(q))
    (v, i), (dv, di) = pq.search(q, 10), dec.search(q, 10)
    assert torch.equal(v, dv) and torch.equal(i, di)


def test_encode_equals_the_numpy_oracle_at_dp_128():
    from dpr_scale_amd.hotpath import default_kernels

    kn = default_kernels()
    for dsub in (2, 4, 8):
        g = torch.Generator().manual_seed(dsub)
        cb = torch.randn(128 // dsub, 256, dsub, generator=g).to(torch.bfloat16)
        cb[:, 9] = cb[:, 4]      # an exact tie between two centroids: the lower index wins
        cb[:, 200] = cb[:, 4]
        x = torch.randn(1000, 128, generator=g).to(torch.bfloat16)
        x[10:20] = cb[:, 4].reshape(1, 128)   # rows that sit on the tied centroid
        x[5] = float("nan")                   # a row of NaNs: code 0
        x[6, 64:] = float("nan")
        raws = []
        codes = kn.colbert_pq_encode(x.to(DEV), cb.to(DEV))
        want = PO.encode(x.float().numpy(), cb.float().numpy())
        assert codes.dtype == torch.uint8 and np.array_equal(codes.cpu().numpy(), want)
        assert not codes[5].any() and bool((codes[10:20] == 4).all())
        # through ctypes alone, the codes between guard bands
        from dpr_scale_amd import _lib

        xd, cd = x.to(DEV), cb.to(DEV)
        out = _banded(raws, 1000 * (128 // dsub))
        _lib.check(_lib.lib.dprhot_colbert_pq_encode(_p(xd), 1000, 128, _p(cd), dsub, _p(out), _stream()), "dprhot_colbert_pq_encode")
        _check_bands(raws)
        assert np.array_equal(out.view(1000, 128 // dsub).cpu().numpy(), want)


def test_padding_code_bytes_are_never_decoded():
    q, dense, pq, dec = case(96, 4)
    cb = pq.codebook.clone()
    cb[:, 255] = 1.0  # whatever centroid 255 was: now it is certainly not a zero row
    base = colbert.ColBERTPQIndex.from_packed(pq.tok_code, pq.blk_rows, cb, pq.doc_blk, pq.corpus_len, pq.d)
    code = pq.tok_code.clone()
    code[~colbert._real_rows(pq.blk_rows)] = 0xFF
    other = colbert.ColBERTPQIndex.from_packed(code, pq.blk_rows, cb, pq.doc_blk, pq.corpus_len, pq.d)
    for pool in ("sum", "max"):
        assert torch.equal(other.score(q, 0, None, pool), base.score(q, 0, None, pool))
        assert torch.equal(other.score(q, 0, None, pool), base.decode().score(q, 0, None, pool))


def test_a_nan_centroid_never_wins():
    q, dense, pq, dec = case(128, 8)
    cb = pq.codebook.clone()
    real = colbert._real_rows(pq.blk_rows)
    used = int(pq.tok_code[real][7, 3])
    cb[3, used] = float("nan")
    hit = (pq.tok_code[:, 3] == used) & real
    assert 0 < int(hit.sum()) < int(real.sum())
    bad = colbert.ColBERTPQIndex.from_packed(pq.tok_code, pq.blk_rows, cb, pq.doc_blk, pq.corpus_len, pq.d)
    for pool in ("sum", "max"):
        S = bad.score(q, 0, None, pool)
        assert not torch.isnan(S).any() and torch.equal(S, bad.decode().score(q, 0, None, pool))
        (v, i), (dv, di) = bad.search(q, 7, query_pool=pool), bad.decode().search(q, 7, query_pool=pool)
        assert torch.equal(v, dv) and torch.equal(i, di)


@pytest.mark.parametrize("d,dsub", [(24, 2), (128, 8)])
def test_bare_abi_between_guard_bands(d, dsub):
    from dpr_scale_amd import _lib

    q, dense, pq, dec = case(d, dsub)
    qb = colbert._bf16_padded(q.to(DEV), pq.dp)
    n, k, chunk = len(LENGTHS), 7, 16
    for pool in (0, 1):
        name = "max" if pool else "sum"
        # dprhot_colbert_pq_score into an exactly sized window S [nq, 5]
        raws = []
        S = _banded(raws, NQ * 5 * 4).view(torch.float32).view(NQ, 5)
        _lib.check(_lib.lib.dprhot_colbert_pq_score(*_head(pq, qb, pool), 3, 5, _p(S), 5, _stream()), "dprhot_colbert_pq_score")
        _check_bands(raws)
        assert torch.equal(S, dec.score(q, 3, 5, name))
        # dprhot_colbert_pq_search: values, indices and an exactly sized workspace
        nws = ctypes.c_size_t(0)
        _lib.check(_lib.lib.dprhot_colbert_workspace_bytes(NQ, chunk, ctypes.byref(nws)))
        raws = []
        values = _banded(raws, NQ * k * 4).view(torch.float32).view(NQ, k)
        indices = _banded(raws, NQ * k * 8).view(torch.int64).view(NQ, k)
        ws = _banded(raws, nws.value)
        first = 1
        for b, e in ((0, 20), (20, n)):
            _lib.check(_lib.lib.dprhot_colbert_pq_search(*_head(pq, qb, pool), b, e, k, chunk, _p(values), _p(indices), first, _p(ws),
                                                         nws.value, _stream()), "dprhot_colbert_pq_search")
            first = 0
        _check_bands(raws)
        dv, di = dec.search(q, k, query_pool=name)
        assert torch.equal(values, dv) and torch.equal(indices, di)
    # an index without a block scores 0 everywhere
    raws = []
    S = _banded(raws, NQ * 8 * 4).view(torch.float32).view(NQ, 8)
    zero_blk = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib.dprhot_colbert_pq_score(None, None, _p(pq.codebook), pq.dsub, _p(zero_blk), 0, n, pq.dp, _p(qb), NQ, LQ, 0, 0, 8, _p(S), 8,
                                                _stream()), "dprhot_colbert_pq_score")
    _check_bands(raws)
    assert not S.any()


def test_two_runs_give_the_same_bits():
    q, dense, pq, dec = case(128, 4)
    (v, i), (v2, i2) = pq.search(q, 7), pq.search(q, 7)
    assert torch.equal(v, v2) and torch.equal(i, i2) and torch.equal(pq.score(q), pq.score(q))
    rows = dense.tok[colbert._real_rows(dense.blk_rows)]
    a = colbert.train_pq(rows, dsub=4, iters=3, train_size=512, seed=5)
    b = colbert.train_pq(rows, dsub=4, iters=3, train_size=512, seed=5)
    assert a.shape == (32, 256, 4) and a.is_cuda and torch.equal(a, b)
    assert not torch.equal(a, colbert.train_pq(rows, dsub=4, iters=3, train_size=512, seed=6))


def test_streaming_build_on_the_device_equals_quantize(tmp_path):
    q, dense, pq, dec = case(96, 4)
    real = colbert._real_rows(dense.blk_rows)
    rows = dense.tok[real][:, :96].cpu()
    lens = torch.tensor(LENGTHS)
    start = torch.cumsum(lens, 0) - lens
    for rank, sel in ((0, list(range(1, len(LENGTHS), 2))), (1, list(range(0, len(LENGTHS), 2)))):
        b = colbert.TokenIndexBuilder()
        for j in sel:
            if LENGTHS[j]:
                b.add(rows[start[j]:start[j] + LENGTHS[j]].unsqueeze(0), torch.ones(1, LENGTHS[j]), [j])
        b.write(str(tmp_path), rank)
    got = colbert.load_index(str(tmp_path), len(LENGTHS), DEV, quantizer="pq", sub_vec_dim=4, codebook=pq.codebook)
    for name in ("tok_code", "blk_rows", "doc_blk", "codebook"):
        assert torch.equal(getattr(got, name), getattr(pq, name)), name
    trained = colbert.load_index(str(tmp_path), len(LENGTHS), DEV, quantizer="pq", sub_vec_dim=4, iters=1, train_size=300)
    again = dense.quantize(dsub=4, codebook=trained.codebook)
    assert torch.equal(trained.tok_code, again.tok_code) and torch.equal(trained.blk_rows, again.blk_rows)
    (v, i), (dv, di) = trained.search(q, 7), trained.decode().search(q, 7)
    assert torch.equal(v, dv) and torch.equal(i, di)
