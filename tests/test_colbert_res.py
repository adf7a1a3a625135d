"""The residual-compressed ColBERT token index on the CPU: host-side validation of dprhot_colbert_res_*, the
encode / decode rule on hand-made rows, train_buckets, and ColBERTIndex.compress / ColBERTResidualIndex / the streaming builds /
ColBERTResidualRetrievalTask driven through the test-only stand-in (tests/_colbert_res_standin.py).  The contract is bit-equality with
`decode()`: every comparison is torch.equal, there is no tolerance in this file."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _colbert_res_standin as RS  # noqa: E402
from dpr_scale_amd import colbert  # noqa: E402

REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
_BASE = dict(transform=None, model=None, datamodule=None, optim=None)
BF16 = torch.bfloat16
LENGTHS = [0, 1, 15, 16, 17, 33, 40] * 4
N, D, C, NQ, LQ = len(LENGTHS), 24, 16, 3, 5


def _unit(seed, n, d):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1)


def _dense(kn=None, d=D, **kw):
    """(dense index with C given centroids, two of them equal; queries)"""
    dense = colbert.ColBERTIndex(list(range(N)), LENGTHS, _unit(1, sum(LENGTHS), d), N, "cpu", kernels=kn or RS.ColbertResKernels(), **kw)
    cen = _unit(2, C, d)
    cen[5] = cen[2]
    return dense.build_centroids(C, centroids=cen), torch.randn(NQ, LQ, d, generator=torch.Generator().manual_seed(3))


def _same(a, b):
    return (all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(a._tensors().values(), b._tensors().values()))
            and (a.corpus_len, a.d, a.dp, a.nbits, a.n_blk) == (b.corpus_len, b.d, b.dp, b.nbits, b.n_blk))


_ONE = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch
_ODD = ctypes.c_void_p(264)  # 8-byte aligned only


def test_host_side_validation_of_the_three_entry_points():
    from dpr_scale_amd import _lib

    lib = _lib.lib
    head = dict(code=_ONE, tc=_ONE, cen=_ONE, C=4, w=_ONE, nbits=2, blk=_ONE, nb=10, n=100, dp=32, q=_ONE, nq=2, LQ=5, pool=0, off=_ONE,
                doc=_ONE, nc=50)
    refusals = ((dict(nbits=0), -1, b"nbits"), (dict(nbits=3), -1, b"nbits"), (dict(nbits=8), -1, b"nbits"), (dict(cen=None), -1, b"NULL"),
                (dict(w=None), -1, b"NULL"), (dict(tc=None), -1, b"NULL"), (dict(code=None), -1, b"NULL"), (dict(C=0), -1, b"C="),
                (dict(dp=40), -1, b"dp="), (dict(dp=0), -1, b"dp="), (dict(code=_ODD), -1, b"res_code and the centroid rows"), (dict(cen=_ODD), -1, b"res_code and the centroid rows"),
                (dict(dp=160), -3, b"dp=160"), (dict(dp=800), -3, b"residual ColBERT index"),
                # the limits of dprhot_colbert_cand_score / _search
                (dict(LQ=0), -1, b"LQ="), (dict(LQ=513), -1, b"LQ="), (dict(off=None), -1, b"NULL"), (dict(doc=None), -1, b"NULL"),
                (dict(nc=-1), -1, b"n_cand"), (dict(nc=2 ** 40), -1, b"n_cand"), (dict(pool=7), -1, b"pool"), (dict(n=0), -1, b"corpus_len"),
                (dict(nq=0), -1, b"nq"), (dict(q=None), -1, b"NULL"), (dict(blk=None), -1, b"NULL"))
    good_score = dict(head, b=0, cols=8, S=_ONE, ld=8, st=None)
    score = lambda **bad: lib.dprhot_colbert_res_score(*{**good_score, **bad}.values())
    good = dict(head, mc=40, k=5, chunk=64, vals=_ONE, idx=_ONE, ws=_ONE, wsb=1 << 20, st=None)
    search = lambda **bad: lib.dprhot_colbert_res_search(*{**good, **bad}.values())
    for bad, code, word in refusals:
        for f in (score, search):
            assert f(**bad) == code and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())
    for bad in (dict(S=None), dict(cols=0), dict(ld=7), dict(b=-1)):
        assert score(**bad) == -1, (bad, lib.dprhot_last_error())
    for bad, word in ((dict(vals=None), b"NULL"), (dict(idx=None), b"NULL"), (dict(chunk=0), b"chunk"), (dict(chunk=12), b"chunk"),
                      (dict(k=0), b"topk"), (dict(k=101), b"topk"), (dict(mc=0), b"max_count")):
        assert search(**bad) == -1 and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())
    for bad in (dict(ws=None), dict(wsb=16)):
        assert search(**bad) == -4 and b"colbert_res_search needs" in lib.dprhot_last_error()
    assert search(n=6000, mc=6000, k=5000, wsb=2 * 64 * 4) == -4 and b"topk_wide" in lib.dprhot_last_error()  # k > 4096: the wide state
    # with no token block the index tensors may be NULL (n_blk == 0 scores 0 for present candidates): validation passes them
    assert score(nb=0, code=None, tc=None, cen=None, w=None, S=None) == -1 and b"NULL pointer (centroids" not in lib.dprhot_last_error()

    good_enc = dict(tok=_ONE, tc=_ONE, n=10, dp=32, cen=_ONE, C=4, cut=_ONE, nbits=2, code=_ONE, st=None)
    enc = lambda **bad: lib.dprhot_colbert_res_encode(*{**good_enc, **bad}.values())
    for bad, code, word in ((dict(nbits=3), -1, b"nbits"), (dict(nbits=0), -1, b"nbits"), (dict(C=0), -1, b"C="), (dict(dp=40), -1, b"dp="),
                            (dict(dp=160), -3, b"dp=160"), (dict(cen=None), -1, b"NULL"), (dict(cut=None), -1, b"NULL"),
                            (dict(tc=None), -1, b"NULL"), (dict(tok=None), -1, b"NULL"), (dict(code=None), -1, b"NULL"),
                            (dict(n=-1), -1, b"n_rows"), (dict(n=2 ** 40), -1, b"n_rows"), (dict(cen=_ODD), -1, b"aligned"),
                            (dict(tok=_ODD), -1, b"aligned")):
        assert enc(**bad) == code and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())
    assert enc(n=0, tok=None, tc=None, code=None) == 0  # nothing to encode: no launch


def test_version_stays_and_the_symbols_are_bound():
    from dpr_scale_amd import _lib, hotpath

    assert _lib.version() == 174
    for s in ("dprhot_colbert_res_encode", "dprhot_colbert_res_score", "dprhot_colbert_res_search"):
        assert s in _lib.SIGNATURES and hasattr(_lib.lib, s)
    assert not hasattr(_lib.lib, "dprhot_colbert_res_workspace_bytes")  # the workspace is dprhot_colbert_cand_workspace_bytes
    for m in ("colbert_res_encode", "colbert_res_workspace", "colbert_res_score", "colbert_res_search"):
        assert callable(getattr(hotpath.HipKernels, m))


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_the_encode_and_decode_rule_on_hand_made_rows(nbits):
    """Eight-feature pieces written out by hand: a residual equal to a cutoff (not above it: the lower code), a NaN residual (code 0),
    a padding row (-1) and a centroid id >= C (zero bytes / exact zero rows whatever the bytes hold), and the bit layout byte by byte."""
    nb = 1 << nbits
    cutoffs = (torch.arange(1, nb, dtype=torch.float32) - nb / 2) / 8       # multiples of 1/8, ascending
    weights = (torch.arange(nb, dtype=torch.float32) - nb / 2 + 0.5) / 8
    cen = torch.zeros(2, 32)
    cen[1] = 0.5
    cen = cen.to(BF16)
    res = torch.zeros(5, 32)
    res[0, :nb - 1] = cutoffs                   # equal to a cutoff: `res > cutoff` is false, the code is the cutoff's own index
    res[0, nb - 1:2 * nb - 2] = cutoffs + 1 / 16  # just above: the next code
    res[0, 30], res[0, 31] = -100.0, 100.0      # the two ends
    res[1] = res[0]
    rows = (res + cen.float()[[0, 1, 1, 0, 1]]).to(BF16)
    rows[2, 3] = float("nan")
    tc = torch.tensor([0, 1, 1, -1, 2], dtype=torch.int32)
    want = torch.zeros(5, 32, dtype=torch.int64)
    want[:3] = nb // 2 - 1                      # a residual of 0 IS the middle cutoff: the code below it ...
    want[2, 3] = 0                              # ... but for the NaN
    want[0, :nb - 1] = torch.arange(nb - 1)
    want[0, nb - 1:2 * nb - 2] = torch.arange(1, nb)
    want[0, 30], want[0, 31] = 0, nb - 1
    want[1] = want[0]
    per = 8 // nbits
    packed = torch.zeros(5, 32 // per, dtype=torch.int64)
    for t in range(32):
        packed[:, t // per] += want[:, t] << (nbits * (t % per))
    kn = RS.ColbertResKernels()
    codes = kn.colbert_res_encode(rows, cutoffs, nbits, tc, cen)
    assert codes.dtype == torch.uint8 and codes.shape == (5, 32 * nbits // 8) and torch.equal(codes.long(), packed)
    assert torch.equal(colbert.res_unpack(codes, nbits), want)
    assert torch.equal(want[:2], torch.bucketize(res[:2], cutoffs))  # the rule is torch.bucketize for a non-NaN residual
    # decode through the product: 16 rows = one block of one passage; hostile bytes on the rows without a centroid
    res_code = torch.full((16, 32 * nbits // 8), 0xFF, dtype=torch.uint8)
    res_code[:3] = codes[:3]
    tok_centroid = torch.full((16,), -1, dtype=torch.int32)
    tok_centroid[:5] = tc
    doc_blk = torch.tensor([0, 1], dtype=torch.int64)
    index = colbert.ColBERTResidualIndex.from_packed(res_code, tok_centroid, cen, cutoffs, weights, doc_blk, 1, 32, kernels=kn)
    assert index.nbits == nbits and index.cen_off.tolist() == [0, 1, 2] and index.cen_doc.tolist() == [0, 0]
    tok = index.decode().tok
    assert tok.dtype == BF16 and not tok[3:].any()
    assert torch.equal(tok[:3].float(), (cen.float()[tc[:3].long()] + weights[want[:3]]).to(BF16).float())
    assert torch.equal(tok, RS.decode_rule(res_code, tok_centroid, cen, weights, nbits))
    # every code value decodes: the all-ones bytes under a real centroid are the last weight
    tok_centroid[3] = 1
    again = colbert.ColBERTResidualIndex.from_packed(res_code, tok_centroid, cen, cutoffs, weights, doc_blk, 1, 32, kernels=kn).decode().tok
    assert torch.equal(again[3].float(), (cen[1].float() + weights[-1]).to(BF16).float()) and not again[4:].any()


def test_train_buckets_is_torch_quantile_and_seeded():
    dense, _ = _dense()
    real = torch.nonzero(dense.tok_centroid >= 0).reshape(-1)
    res = dense.tok[real].float()[:, :D] - dense.centroids[dense.tok_centroid[real].long()].float()[:, :D]
    for nbits in (1, 2, 4):
        nb = 1 << nbits
        cutoffs, weights = colbert.train_buckets(res, nbits)
        assert cutoffs.dtype == weights.dtype == torch.float32 and cutoffs.shape == (nb - 1,) and weights.shape == (nb,)
        assert torch.equal(cutoffs, torch.quantile(res.reshape(-1), torch.arange(1, nb) / nb))
        assert torch.equal(weights, torch.quantile(res.reshape(-1), (torch.arange(nb) + 0.5) / nb))
        assert bool((cutoffs[1:] >= cutoffs[:-1]).all()) and bool((weights[:-1] <= cutoffs).all()) and bool((cutoffs <= weights[1:]).all())
        full = dense.compress(nbits)  # fewer rows than train_size: trained on every stored row
        assert torch.equal(full.cutoffs, cutoffs) and torch.equal(full.weights, weights)
        a, b, other = dense.compress(nbits, train_size=50, seed=4), dense.compress(nbits, train_size=50, seed=4), dense.compress(nbits, train_size=50, seed=5)
        assert _same(a, b) and not torch.equal(a.cutoffs, other.cutoffs)
        pick = colbert._sample(int(real.shape[0]), 50, 4)
        assert torch.equal(a.cutoffs, colbert.train_buckets(res[pick], nbits)[0])
        given = dense.compress(nbits, buckets=(a.cutoffs, a.weights), train_size=1, seed=99)  # given buckets train nothing
        assert _same(given, a)
    with pytest.raises(ValueError, match="nbits"):
        colbert.train_buckets(res, 3)
    with pytest.raises(ValueError, match="2\\^24"):
        colbert.train_buckets(torch.zeros(0), 2)
    assert inspect.signature(colbert.ColBERTIndex.compress).parameters["train_size"].default == 65536


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_every_result_equals_the_decoded_index(nbits):
    dense, q = _dense(chunk=8)
    res = dense.compress(nbits)
    assert type(res) is colbert.ColBERTResidualIndex and isinstance(res, colbert.ChunkedIndex) and not hasattr(res, "tok")
    assert (res.dp, res.d, res.nbits, res.n_blk, res.corpus_len, res.chunk) == (32, D, nbits, dense.n_blk, N, 8)
    assert res.res_code.shape == (dense.n_blk * 16, 32 * nbits // 8) and res.res_code.dtype == torch.uint8
    assert res.tok_centroid is dense.tok_centroid and res.centroids is dense.centroids and res.doc_blk is dense.doc_blk
    assert res.cen_off is dense.cen_off and res.cen_doc is dense.cen_doc
    held = (res.res_code, res.tok_centroid, res.centroids, res.cen_off, res.cen_doc, res.cutoffs, res.weights, res.doc_blk)
    assert res.nbytes == sum(t.numel() * t.element_size() for t in held) and res.nbytes < dense.nbytes
    assert torch.equal(res.res_code, RS.encode_rule(dense.tok, dense.tok_centroid, dense.centroids, res.cutoffs, nbits))
    assert not res.res_code[dense.tok_centroid < 0].any()
    dec = res.decode()
    assert type(dec) is colbert.ColBERTIndex and dec.tok_centroid is res.tok_centroid and dec.cen_doc is res.cen_doc
    assert torch.equal(dec.tok, RS.decode_rule(res.res_code, res.tok_centroid, res.centroids, res.weights, nbits))
    assert torch.equal(res.probe(q, 3), dense.probe(q, 3))
    for nprobe in (1, 3):
        cand_off, cand_doc = res.candidates(q, nprobe)
        assert all(torch.equal(a, b) for a, b in zip((cand_off, cand_doc), dense.candidates(q, nprobe)))
        for pool in ("sum", "max"):
            S = res.score_candidates(q, cand_off, cand_doc, pool)
            assert torch.equal(S.nan_to_num(nan=-7.0), dec.score_candidates(q, cand_off, cand_doc, pool).nan_to_num(nan=-7.0))
            assert bool(torch.isnan(S).any()) or nprobe == C
            A = res.approx_candidates(q, cand_off, cand_doc, pool)
            assert torch.equal(A.nan_to_num(nan=-7.0), dec.approx_candidates(q, cand_off, cand_doc, pool).nan_to_num(nan=-7.0))
            assert torch.equal(res.prune_candidates(q, cand_off, cand_doc, 4, pool), dec.prune_candidates(q, cand_off, cand_doc, 4, pool))
            for k, ndocs in ((1, None), (5, None), (N, None), (3, 4), (4, 1000)):
                got, want = res.search_pruned(q, k, nprobe, pool, ndocs=ndocs), dec.search_pruned(q, k, nprobe, pool, ndocs=ndocs)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[0].shape == (NQ, k), (nprobe, pool, k, ndocs)
    assert bool((res.search_pruned(q, N, 1)[1] == -1).any())  # fewer candidates than topk: -inf / -1 tails
    assert set(res.latency) >= {"encode_time", "candidate_time", "search_time", "interaction_time"}
    with pytest.raises(ValueError, match="topk"):
        res.search_pruned(q, 5, 2, ndocs=4)


def test_refusals_name_decode_and_compress_needs_centroids():
    dense, q = _dense()
    res = dense.compress(2)
    for call in (lambda: res.search(q, 3), lambda: res.score(q), lambda: res.compress(1), lambda: res.quantize()):
        with pytest.raises(NotImplementedError, match=r"decode\(\)"):
            call()
    with pytest.raises(TypeError, match="compress"):
        colbert.ColBERTResidualIndex()
    plain = colbert.ColBERTIndex.from_packed(dense.tok, dense.doc_blk, N, D, kernels=RS.ColbertResKernels())
    with pytest.raises(ValueError, match="no centroids"):
        plain.compress(2)
    with pytest.raises(ValueError, match="nbits"):
        dense.compress(3)
    with pytest.raises(ValueError, match="buckets"):
        dense.compress(2, buckets=(torch.zeros(2), torch.zeros(4)))
    # the dense class kept its methods through the mixin, the product-quantised one its refusal
    assert colbert.ColBERTIndex.search_pruned is colbert.ColBERTResidualIndex.search_pruned
    with pytest.raises(NotImplementedError, match="dense rows only"):
        colbert.ColBERTPQIndex.__new__(colbert.ColBERTPQIndex).search_pruned(q, 5, 2)


def test_save_and_load_round_trip(tmp_path):
    dense, q = _dense()
    res = dense.compress(4)
    path = res.save(str(tmp_path / "colbert_res.pt"))
    blob = torch.load(path, weights_only=True)
    assert blob["format"] == "dpr_scale_amd.colbert_res/1" and blob["nbits"] == 4 and blob["res_code"].dtype == torch.uint8
    back = colbert.load_residual_index(path, "cpu", chunk=16, kernels=RS.ColbertResKernels())
    assert _same(back, res) and back.chunk == 16
    for a, b in zip(back.search_pruned(q, 4, 2, ndocs=5), res.search_pruned(q, 4, 2, ndocs=5)):
        assert torch.equal(a, b)
    torch.save({"format": "something/1"}, str(tmp_path / "other.pt"))
    with pytest.raises(ValueError, match="not a residual"):
        colbert.load_residual_index(str(tmp_path / "other.pt"), "cpu")


class _CountingKernels(RS.ColbertResKernels):
    def __init__(self):
        self.encoded = []

    def colbert_res_encode(self, rows, cutoffs, nbits, tok_centroid=None, centroids=None):
        self.encoded.append(int(rows.shape[0]))
        return super().colbert_res_encode(rows, cutoffs, nbits, tok_centroid, centroids)


def _two_files(path, d, seed):
    """tokens_0000.pkl holds the even doc ids, tokens_0001.pkl the odd ones; returns the passages as row tensors."""
    rows = _unit(seed, sum(LENGTHS), d).to(BF16)
    passages = list(torch.split(rows, LENGTHS))
    for rank in (0, 1):
        b = colbert.TokenIndexBuilder()
        for j in range(rank, N, 2):
            if LENGTHS[j]:
                b.add(passages[j].unsqueeze(0), torch.ones(1, LENGTHS[j]), [j])
        b.write(str(path), rank)
    return passages


def _one_shot(passages, d, like, kn):
    dense = colbert.ColBERTIndex(list(range(N)), LENGTHS, torch.cat(passages), N, "cpu", kernels=kn)
    dense.build_centroids(int(like.centroids.shape[0]), centroids=like.centroids[:, :d])
    return dense.compress(like.nbits, buckets=(like.cutoffs, like.weights))


@pytest.mark.parametrize("nbits", [1, 4])
def test_streaming_load_index_equals_the_one_shot_build(nbits, tmp_path):
    passages = _two_files(tmp_path, D, 11)
    count = _CountingKernels()
    res = colbert.load_index(str(tmp_path), N, "cpu", chunk=8, kernels=count, quantizer="residual", nbits=nbits, n_centroids=8, iters=2,
                             train_size=120, seed=3)
    assert type(res) is colbert.ColBERTResidualIndex and res.chunk == 8 and res.nbits == nbits and res.centroids.shape == (8, 32)
    per_file = sorted([sum(LENGTHS[0::2]), sum(LENGTHS[1::2])])
    assert sorted(count.encoded) == per_file  # each encode call sees one file's rows
    assert _same(res, _one_shot(passages, D, res, RS.ColbertResKernels()))
    again = colbert.load_index(str(tmp_path), N, "cpu", kernels=RS.ColbertResKernels(), quantizer="residual", nbits=nbits, n_centroids=8, iters=2,
                               train_size=120, seed=3)
    assert _same(again, res)
    count = _CountingKernels()
    given = colbert.load_index(str(tmp_path), N, "cpu", kernels=count, quantizer="residual", nbits=nbits, centroids=res.centroids[:, :D],
                               buckets=(res.cutoffs, res.weights))
    assert _same(given, res) and sorted(count.encoded) == per_file
    with pytest.raises(NotImplementedError, match="quantizer"):
        colbert.load_index(str(tmp_path), N, "cpu", kernels=count, quantizer="sq")
    for kw in (dict(iters=3), dict(n_centroids=8), dict(buckets=(res.cutoffs, res.weights)), dict(quantizer="pq", n_centroids=8),
               dict(quantizer="residual", n_centroids=8, lloyd=3),
               dict(quantizer="residual", centroids=res.centroids[:, :D], buckets=(res.cutoffs, res.weights), seed=1)):
        with pytest.raises(TypeError):
            colbert.load_index(str(tmp_path), N, "cpu", kernels=count, **kw)
    with pytest.raises(ValueError, match="n_centroids"):
        colbert.load_index(str(tmp_path), N, "cpu", kernels=count, quantizer="residual")


def test_builder_finish_residual_part_by_part():
    d = 40
    passages = list(torch.split(_unit(40, sum(LENGTHS), d).to(BF16), LENGTHS))
    count = _CountingKernels()
    b = colbert.TokenIndexBuilder(N, kernels=count)
    groups = (list(range(0, 9)), list(range(9, 10)), list(range(10, N)))
    for sel in groups:
        L = max(max(LENGTHS[j] for j in sel), 1)
        x, att = torch.zeros(len(sel), L, d, dtype=BF16), torch.zeros(len(sel), L)
        for r, j in enumerate(sel):
            x[r, :LENGTHS[j]], att[r, :LENGTHS[j]] = passages[j], 1
        b.add(x, att, sel)
    res = b.finish(quantizer="residual", nbits=2, n_centroids=6, iters=1)
    assert count.encoded == [sum(LENGTHS[j] for j in sel) for sel in groups]  # assigned and encoded batch by batch
    assert res.dp == 64 and res.d == d and _same(res, _one_shot(passages, d, res, RS.ColbertResKernels()))
    for f in (colbert.load_index, colbert.TokenIndexBuilder.finish):
        p = inspect.signature(f).parameters
        assert p["quantizer"].default is None and p["nbits"].default == 2 and p["n_centroids"].default is None
        assert p["centroids"].default is None and p["buckets"].default is None
    with pytest.raises(TypeError):
        b.finish(n_centroids=6)


class _Enc(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, token_ids, **kw):
        return dict(self.out)


def test_the_task_writes_and_rereads_its_index_file(tmp_path):
    from dpr_scale_amd.task.colbert_retrieval import ColBERTPQRetrievalTask, ColBERTResidualRetrievalTask, ColBERTRetrievalTask

    ctx = str(tmp_path / "ctx")
    os.makedirs(ctx)
    _two_files(tmp_path / "ctx", D, 21)
    base = dict(ctx_embeddings_dir=ctx, checkpoint_path="", topk=3, output_path=str(tmp_path / "out"), **_BASE)
    a = inspect.signature(ColBERTResidualRetrievalTask.__init__).parameters
    assert a["nbits"].default == 2 and a["save_compressed"].default is False and a["nprobe"].default is None and a["ndocs"].default is None
    assert ColBERTResidualRetrievalTask._search is ColBERTRetrievalTask._search and ColBERTResidualRetrievalTask.RES_FILE == "colbert_res.pt"
    assert not issubclass(ColBERTResidualRetrievalTask, ColBERTPQRetrievalTask)
    for kw in (dict(), dict(nprobe=2), dict(n_centroids=8)):
        with pytest.raises(ValueError, match="nprobe and n_centroids"):
            ColBERTResidualRetrievalTask(**kw, **base)
    with pytest.raises(NotImplementedError, match="nbits=3"):
        ColBERTResidualRetrievalTask(nbits=3, nprobe=2, n_centroids=8, **base)
    with pytest.raises(NotImplementedError, match="cuda=False"):
        ColBERTResidualRetrievalTask(nprobe=2, n_centroids=8, cuda=False, **base)

    kn = RS.ColbertResKernels()
    knobs = dict(nbits=4, nprobe=2, n_centroids=8)
    task = ColBERTResidualRetrievalTask(**knobs, **base)
    assert (task.nbits, task.nprobe, task.n_centroids, task.ndocs, task.save_compressed) == (4, 2, 8, None, False)
    task.kernels, task.ctxs = kn, range(N)
    built = task._load_index("cpu")
    assert type(built) is colbert.ColBERTResidualIndex and built.nbits == 4 and not os.path.exists(os.path.join(ctx, "colbert_res.pt"))
    task = ColBERTResidualRetrievalTask(save_compressed=True, **knobs, **base)
    task.kernels, task.ctxs = kn, range(N)
    task.index = task._load_index("cpu")
    assert os.path.exists(os.path.join(ctx, "colbert_res.pt")) and _same(task.index, built)
    os.remove(os.path.join(ctx, "tokens_0000.pkl"))  # from here on only the saved file can give the whole index
    reread = ColBERTResidualRetrievalTask(ndocs=5, **knobs, **base)
    reread.kernels, reread.ctxs = kn, range(N)
    reread.index = reread._load_index("cpu")
    assert _same(reread.index, built)
    q = torch.randn(2, 5, D, generator=torch.Generator().manual_seed(9))
    reread.query_encoder = _Enc({"expert_repr": q})
    out = reread.test_step({"query_ids": {"input_ids": torch.zeros((2, 6), dtype=torch.long)}, "topic_ids": ["a", "b"]}, 0)
    v, i = built.decode().search_pruned(q, 3, 2, ndocs=5)  # ndocs is passed on
    assert out[0] == v.tolist() and out[1] == i.tolist()
    v_all, i_all = built.decode().search_pruned(q, 3, 2)
    seen = []
    reread.index.search_pruned = lambda *a, **kw: seen.append(kw) or (v_all, i_all)
    reread._search({"expert_repr": q}, 2, 0.0)
    reread.ndocs = None
    reread._search({"expert_repr": q}, 2, 0.0)
    assert seen[0]["ndocs"] == 5 and "ndocs" not in seen[1]
    other = ColBERTResidualRetrievalTask(nbits=2, nprobe=2, n_centroids=8, **base)
    other.kernels, other.ctxs = kn, range(N)
    with pytest.raises(ValueError, match="nbits=4"):
        other._load_index("cpu")


def _report():
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
    return rows


def test_residual_kernels_never_spill_and_the_other_families_keep_their_counts():
    rows = _report()
    mine = {k: v for k, v in rows.items() if re.search(r"dprhot\d+cbr_\w+_kernel", k)}
    assert sum("cbr_score_kernel" in k for k in mine) == 12 and sum("cbr_encode_kernel" in k for k in mine) == 3 and len(mine) == 15, sorted(rows)
    for name, r in mine.items():
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
    for family, count in (("cb_", 5), ("cbc_", 6), ("cbi_", 6), ("cbpq_", 12)):
        assert len([k for k in rows if re.search(r"dprhot\d+%s\w+_kernel" % family, k)]) == count, family
    assert len([k for k in rows if re.search(r"dprhot\d+pq_encode_kernel", k)]) == 3
