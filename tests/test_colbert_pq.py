"""The product-quantised ColBERT token index on the CPU: ColBERTIndex.quantize / ColBERTPQIndex / the streaming
builds / ColBERTPQRetrievalTask driven through the test-only stand-in (tests/_colbert_pq_standin.py), the pinned limit of ivf.train_pq,
the ABI surface with the host-side validation of dprhot_colbert_pq_*, and the compiler's resource report of csrc/colbert_pq.h."""
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

import _colbert_pq_standin as PS  # noqa: E402
import _pq_oracle as PO  # noqa: E402
from dpr_scale_amd import colbert, ivf  # noqa: E402

REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
_BASE = dict(transform=None, model=None, datamodule=None, optim=None)
LENGTHS = [0, 1, 15, 16, 17, 33]
BF16 = torch.bfloat16


def _rows(seed, n, d):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed)).to(BF16)


def _corpus(seed, lengths, d, dsub, kn, nq=2, LQ=5):
    rows = _rows(seed, sum(lengths), d)
    dense = colbert.ColBERTIndex(list(range(len(lengths))), lengths, rows, len(lengths), "cpu", kernels=kn)
    q = _rows(seed + 1, nq * LQ, d).float().reshape(nq, LQ, d)
    return rows, dense, q


def _equal(a, b):
    return (torch.equal(a.tok_code, b.tok_code) and torch.equal(a.blk_rows, b.blk_rows) and torch.equal(a.doc_blk, b.doc_blk)
            and torch.equal(a.codebook, b.codebook) and (a.corpus_len, a.d, a.dp, a.dsub, a.n_blk) == (b.corpus_len, b.d, b.dp, b.dsub, b.n_blk))


@pytest.mark.parametrize("d,dsub", [(24, 2), (40, 4), (128, 8)])
def test_quantize_decode_round_trip_and_blk_rows(d, dsub):
    kn = PS.ColbertPQKernels()
    rows, dense, q = _corpus(d, LENGTHS, d, dsub, kn)
    assert dense.blk_rows.tolist() == [1, 15, 16, 16, 1, 16, 16, 1] and dense.blk_rows.dtype == torch.uint8
    pq = dense.quantize(dsub=dsub, iters=1, train_size=64)
    dp = (d + 31) // 32 * 32
    assert type(pq) is colbert.ColBERTPQIndex and isinstance(pq, colbert.ChunkedIndex) and not hasattr(pq, "tok")
    assert (pq.dp, pq.d, pq.dsub, pq.n_blk, pq.corpus_len) == (dp, d, dsub, 8, 6)
    assert pq.tok_code.shape == (128, dp // dsub) and pq.tok_code.dtype == torch.uint8 and pq.codebook.shape == (dp // dsub, 256, dsub)
    assert torch.equal(pq.blk_rows, dense.blk_rows) and pq.doc_blk is dense.doc_blk
    assert pq.nbytes == 128 * dp // dsub + 8 + dp * 512 + 7 * 8
    # the encode rule on the real rows, zero bytes on the padding rows
    real = colbert._real_rows(pq.blk_rows)
    assert int(real.sum()) == sum(LENGTHS) and not pq.tok_code[~real].any()
    want = PO.encode(dense.tok[real].float().numpy(), pq.codebook.float().numpy())
    assert np.array_equal(pq.tok_code[real].numpy(), want)
    # decode: the decoded rows, exact zeros behind blk_rows
    dec = pq.decode()
    assert type(dec) is colbert.ColBERTIndex and dec.tok.shape == dense.tok.shape and torch.equal(dec.doc_blk, dense.doc_blk)
    assert torch.equal(dec.tok[real], ivf.pq_decode(pq.tok_code, pq.codebook)[real]) and not dec.tok[~real].any()
    assert torch.equal(dec.blk_rows, pq.blk_rows)
    for pool in ("sum", "max"):
        assert torch.equal(pq.score(q, 0, None, pool), dec.score(q, 0, None, pool))
        assert torch.equal(pq.score(q, 2, 3, pool), dec.score(q, 2, 3, pool))
        for kw in (dict(), dict(chunk=8, id_ranges=[(3, 6), (0, 3)])):
            (v, i), (dv, di) = pq.search(q, 4, query_pool=pool, **kw), dec.search(q, 4, query_pool=pool, **kw)
            assert torch.equal(v, dv) and torch.equal(i, di)
    assert pq.default_chunk(4) == dense.default_chunk(4) and pq.latency["search_time"] > 0 and "encode_time" in pq.latency
    # a given codebook is used as it is; nothing to train with then
    again = dense.quantize(dsub=dsub, codebook=pq.codebook)
    assert _equal(again, pq)
    with pytest.raises(TypeError, match="nothing to train"):
        dense.quantize(dsub=dsub, codebook=pq.codebook, iters=2)
    with pytest.raises(TypeError, match="quantised already"):
        pq.quantize()
    with pytest.raises(TypeError):
        colbert.ColBERTPQIndex()
    with pytest.raises(ValueError, match="sub_vec_dim"):
        dense.quantize(dsub=3)
    with pytest.raises(ValueError, match="codebook"):
        dense.quantize(dsub=dsub, codebook=pq.codebook.float())


def test_padding_code_bytes_change_nothing():
    kn = PS.ColbertPQKernels()
    _, dense, q = _corpus(3, LENGTHS, 24, 4, kn)
    pq = dense.quantize(dsub=4, iters=1)
    cb = pq.codebook.clone()
    cb[:, 255] = 1.0  # centroid 255 is not a zero row: the padding rows are zeroed by blk_rows, not by what their codes decode to
    assert not (pq.tok_code == 255).any()
    pq = colbert.ColBERTPQIndex.from_packed(pq.tok_code, pq.blk_rows, cb, pq.doc_blk, pq.corpus_len, pq.d, kernels=kn)
    code = pq.tok_code.clone()
    code[~colbert._real_rows(pq.blk_rows)] = 0xFF
    other = colbert.ColBERTPQIndex.from_packed(code, pq.blk_rows, cb, pq.doc_blk, pq.corpus_len, pq.d, kernels=kn)
    assert not torch.equal(other.tok_code, pq.tok_code) and torch.equal(other.decode().tok, pq.decode().tok)
    assert ivf.pq_decode(code, cb)[~colbert._real_rows(pq.blk_rows)].all()
    for pool in ("sum", "max"):
        assert torch.equal(other.score(q, 0, None, pool), pq.score(q, 0, None, pool))


def test_from_packed_derives_blk_rows_from_the_last_non_zero_row():
    tok = torch.zeros((48, 32), dtype=BF16)
    tok[0:16, 0] = 1
    tok[16:19, 5] = 2
    index = colbert.ColBERTIndex.from_packed(tok, torch.tensor([0, 2, 3]), 2, 20, kernels=PS.ColbertPQKernels())
    assert index.blk_rows.tolist() == [16, 3, 0]
    pq = index.quantize(dsub=8, iters=0)
    assert torch.equal(pq.decode().tok, tok)  # 2 distinct sub-vectors per subspace: the initial codebook holds them


def test_save_and_load_pq_index(tmp_path):
    kn = PS.ColbertPQKernels()
    _, dense, q = _corpus(5, LENGTHS, 40, 8, kn)
    pq = dense.quantize(dsub=8, iters=1)
    path = pq.save(str(tmp_path / "colbert_pq.pt"))
    blob = torch.load(path, weights_only=True)
    assert blob["format"] == "dpr_scale_amd.colbert_pq/1" and sorted(blob) == sorted(
        ["format", "corpus_len", "d", "dsub", "tok_code", "blk_rows", "codebook", "doc_blk"])
    back = colbert.load_pq_index(path, "cpu", chunk=8, kernels=kn)
    assert _equal(back, pq) and back.chunk == 8
    (v, i), (bv, bi) = pq.search(q, 3), back.search(q, 3)
    assert torch.equal(v, bv) and torch.equal(i, bi)
    torch.save(dict(format="something else"), str(tmp_path / "other.pt"))
    with pytest.raises(ValueError, match="not a product-quantised"):
        colbert.load_pq_index(str(tmp_path / "other.pt"), "cpu")


def _two_files(tmp_path, lengths, d, seed):
    """Passages (doc id = position) written as two token files with interleaved doc ids, the second file first in id order."""
    passages = [_rows(seed + j, n, d) for j, n in enumerate(lengths)]
    att = [torch.ones(1, max(p.shape[0], 1)) * (p.shape[0] > 0) for p in passages]
    for rank, sel in ((1, list(range(0, len(lengths), 2))), (0, list(range(len(lengths) - 1 - len(lengths) % 2, 0, -2)))):
        b = colbert.TokenIndexBuilder()
        for j in sel:
            x = passages[j] if passages[j].shape[0] else torch.zeros(1, d, dtype=BF16)
            b.add(x.unsqueeze(0), att[j], [j])
        b.write(str(tmp_path), rank)
    return passages


class _CountingKernels(PS.ColbertPQKernels):
    def __init__(self):
        self.encoded = []

    def colbert_pq_encode(self, vec, codebook):
        self.encoded.append(int(vec.shape[0]))
        return super().colbert_pq_encode(vec, codebook)


@pytest.mark.parametrize("dsub", [2, 8])
def test_streaming_load_index_equals_quantize_of_the_dense_load(dsub, tmp_path):
    lengths, d = [3, 0, 17, 16, 1, 33, 15], 24
    _two_files(tmp_path, lengths, d, 11)
    kn = PS.ColbertPQKernels()
    dense = colbert.load_index(str(tmp_path), len(lengths), "cpu", kernels=kn)
    assert type(dense) is colbert.ColBERTIndex
    count = _CountingKernels()
    pq = colbert.load_index(str(tmp_path), len(lengths), "cpu", chunk=8, kernels=count, quantizer="pq", sub_vec_dim=dsub, iters=1, train_size=40,
                            seed=3)
    assert type(pq) is colbert.ColBERTPQIndex and pq.chunk == 8 and pq.dsub == dsub
    assert _equal(pq, dense.quantize(dsub=dsub, codebook=pq.codebook))
    # trained on a sample of 40 rows, then encoded file by file: the last two encode calls are the two files' rows
    per_file = sorted([sum(lengths[0::2]), sum(lengths[1::2])])
    assert sorted(count.encoded[-2:]) == per_file and count.encoded[:-2] == [40]
    # same seed, same codebook; a given codebook trains nothing
    again = colbert.load_index(str(tmp_path), len(lengths), "cpu", kernels=kn, quantizer="pq", sub_vec_dim=dsub, iters=1, train_size=40, seed=3)
    assert _equal(again, pq)
    count = _CountingKernels()
    given = colbert.load_index(str(tmp_path), len(lengths), "cpu", kernels=count, quantizer="pq", sub_vec_dim=dsub, codebook=pq.codebook)
    assert _equal(given, pq) and sorted(count.encoded) == per_file
    with pytest.raises(NotImplementedError, match="quantizer"):
        colbert.load_index(str(tmp_path), len(lengths), "cpu", kernels=kn, quantizer="sq")
    with pytest.raises(TypeError):
        colbert.load_index(str(tmp_path), len(lengths), "cpu", kernels=kn, iters=3)


def test_builder_finish_quantised_part_by_part():
    lengths, d = [3, 0, 17, 16, 1, 33, 15], 40
    passages = [_rows(40 + j, n, d) for j, n in enumerate(lengths)]
    count = _CountingKernels()
    b = colbert.TokenIndexBuilder(len(lengths), kernels=count)
    for sel in ([6, 2], [0], [5, 3, 4]):
        L = max(lengths[j] for j in sel)
        x, att = torch.zeros(len(sel), L, d, dtype=BF16), torch.zeros(len(sel), L)
        for r, j in enumerate(sel):
            x[r, :lengths[j]], att[r, :lengths[j]] = passages[j], 1
        b.add(x, att, sel)
    dense = b.finish()
    assert type(dense) is colbert.ColBERTIndex
    pq = b.finish(quantizer="pq", sub_vec_dim=4, iters=1)
    assert count.encoded == [85, 15 + 17, 3, 33 + 16 + 1]  # one Lloyd iteration on all rows, then the codes batch by batch
    assert _equal(pq, dense.quantize(dsub=4, codebook=pq.codebook))
    for f in (colbert.load_index, colbert.TokenIndexBuilder.finish):
        p = inspect.signature(f).parameters
        assert p["quantizer"].default is None and p["sub_vec_dim"].default == 8 and p["codebook"].default is None


class _Enc(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, token_ids, **kw):
        return dict(self.out)


def test_pq_task_writes_and_rereads_its_index_file(tmp_path):
    from dpr_scale_amd.task.colbert_retrieval import ColBERTPQRetrievalTask, ColBERTRetrievalTask

    lengths, d = [3, 0, 17, 16, 1, 33, 15], 24
    ctx = str(tmp_path / "ctx")
    os.makedirs(ctx)
    _two_files(tmp_path / "ctx", lengths, d, 21)
    base = dict(ctx_embeddings_dir=ctx, checkpoint_path="", topk=3, output_path=str(tmp_path / "out"), **_BASE)
    a = inspect.signature(ColBERTPQRetrievalTask.__init__).parameters
    assert a["sub_vec_dim"].default == 8 and a["save_quantized"].default is False and a["quantizer"].default == "pq"
    assert ColBERTPQRetrievalTask._search is ColBERTRetrievalTask._search and ColBERTPQRetrievalTask.PQ_FILE == "colbert_pq.pt"
    with pytest.raises(NotImplementedError, match="sub_vec_dim=3"):
        ColBERTPQRetrievalTask(sub_vec_dim=3, **base)
    with pytest.raises(NotImplementedError, match="quantizer"):
        ColBERTPQRetrievalTask(quantizer="sq", **base)
    with pytest.raises(NotImplementedError, match="cuda=False"):
        ColBERTPQRetrievalTask(cuda=False, **base)
    with pytest.raises(NotImplementedError):  # the plain class is as it was
        ColBERTRetrievalTask(quantizer="pq", **base)

    kn = PS.ColbertPQKernels()
    task = ColBERTPQRetrievalTask(sub_vec_dim=4, **base)
    assert task.quantizer == "pq" and task.sub_vec_dim == 4 and task.save_quantized is False
    task.kernels, task.ctxs = kn, range(len(lengths))
    built = task._load_index("cpu")
    assert type(built) is colbert.ColBERTPQIndex and built.dsub == 4 and not os.path.exists(os.path.join(ctx, "colbert_pq.pt"))
    task = ColBERTPQRetrievalTask(sub_vec_dim=4, save_quantized=True, **base)
    task.kernels, task.ctxs = kn, range(len(lengths))
    task.index = task._load_index("cpu")
    assert os.path.exists(os.path.join(ctx, "colbert_pq.pt")) and _equal(task.index, built)
    os.remove(os.path.join(ctx, "tokens_0000.pkl"))  # from here on only the saved file can give the whole index
    reread = ColBERTPQRetrievalTask(sub_vec_dim=4, **base)
    reread.kernels, reread.ctxs = kn, range(len(lengths))
    reread.index = reread._load_index("cpu")
    assert _equal(reread.index, built)
    q = _rows(99, 2 * 5, d).float().reshape(2, 5, d)
    reread.query_encoder = _Enc({"expert_repr": q})
    out = reread.test_step({"query_ids": {"input_ids": torch.zeros((2, 6), dtype=torch.long)}, "topic_ids": ["a", "b"]}, 0)
    v, i = built.decode().search(q, 3)
    assert out[0] == v.tolist() and out[1] == i.tolist()
    reread.test_epoch_end([out])
    assert len(open(os.path.join(reread.output_path, "retrieval_0000.trec")).read().splitlines()) == 6
    other = ColBERTPQRetrievalTask(sub_vec_dim=8, **base)
    other.kernels, other.ctxs = kn, range(len(lengths))
    with pytest.raises(ValueError, match="sub_vec_dim=4"):
        other._load_index("cpu")


def test_train_pq_keeps_its_limit_and_the_colbert_entry_lifts_it():
    kn = PS.ColbertPQKernels()
    rows = _rows(1, 300, 128)
    with pytest.raises(NotImplementedError, match="at most 64"):
        ivf.train_pq(rows, dsub=4, kernels=kn)
    p = inspect.signature(ivf.train_pq).parameters
    assert p["max_dp"].kind is p["encode"].kind is inspect.Parameter.KEYWORD_ONLY and p["max_dp"].default == 64 and p["encode"].default is None
    seen = []
    a = colbert.train_pq(rows, dsub=8, iters=2, kernels=kn, on_iteration=lambda i, cb: seen.append(i))
    b = ivf.train_pq(rows, dsub=8, iters=2, kernels=kn, max_dp=128, encode=kn.colbert_pq_encode)
    assert a.shape == (16, 256, 8) and a.dtype == BF16 and torch.equal(a, b) and seen == [0, 1, 2]
    assert torch.equal(colbert.train_pq(rows[:, :100].float(), dsub=8, iters=1, kernels=kn)[13:], torch.zeros((3, 256, 8), dtype=BF16))
    with pytest.raises(NotImplementedError, match="at most 128"):
        colbert.train_pq(_rows(2, 4, 160), dsub=8, kernels=kn)
    with pytest.raises(ValueError, match="sub_vec_dim"):
        colbert.train_pq(rows, dsub=16, kernels=kn)


def test_abi_surface_and_host_validation():
    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import HipKernels

    assert _lib.version() == 174
    for s in ("dprhot_colbert_pq_encode", "dprhot_colbert_pq_score", "dprhot_colbert_pq_search"):
        assert hasattr(_lib.lib, s) and s in _lib.SIGNATURES
    assert callable(HipKernels.colbert_pq_encode) and callable(HipKernels.colbert_pq_score) and callable(HipKernels.colbert_pq_search)
    lib = _lib.lib
    one = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch
    INVALID, UNSUPPORTED = -1, -3

    def named(defaults, kw):
        assert set(kw) <= set(defaults), kw
        return [kw.get(k, v) for k, v in defaults.items()]

    enc = lambda **kw: lib.dprhot_colbert_pq_encode(*named(dict(vec=one, n=10, dp=128, cb=one, dsub=8, codes=one, st=None), kw))
    score = lambda **kw: lib.dprhot_colbert_pq_score(*named(dict(
        code=one, rows=one, cb=one, dsub=8, blk=one, nb=10, n=100, dp=128, q=one, nq=2, LQ=5, pool=0, b=0, cols=64, S=one, ld=64, st=None), kw))
    search = lambda **kw: lib.dprhot_colbert_pq_search(*named(dict(
        code=one, rows=one, cb=one, dsub=8, blk=one, nb=10, n=100, dp=128, q=one, nq=2, LQ=5, pool=0, b=0, e=100, k=5, chunk=64, vals=one,
        idx=one, first=1, ws=one, wsb=1 << 20, st=None), kw))
    for f, nulls in ((enc, ("vec", "cb", "codes")), (score, ("code", "rows", "cb", "blk", "q", "S")),
                     (search, ("code", "rows", "cb", "blk", "q", "vals", "idx", "ws"))):
        for name in nulls:
            rc = f(**{name: None})
            assert rc == (-4 if name == "ws" else INVALID), (name, rc)
            assert name == "ws" or b"NULL" in lib.dprhot_last_error()
        assert f(dsub=3) == INVALID and b"dsub" in lib.dprhot_last_error()
        assert f(dsub=0) == INVALID and f(dsub=16) == INVALID
        assert f(dp=48) == INVALID and b"multiple of 32" in lib.dprhot_last_error()
        assert f(dp=0) == INVALID
        assert f(dp=160) == UNSUPPORTED and b"dp=160" in lib.dprhot_last_error()
        assert f(dp=768) == UNSUPPORTED
    assert enc(n=-1) == INVALID and enc(n=0, vec=None, codes=None) == 0  # nothing to encode: nothing is launched
    assert lib.dprhot_pq_encode(one, 10, 128, one, 8, one, None) == UNSUPPORTED  # the postings' entry keeps its limit
    for f in (score, search):
        assert f(cb=ctypes.c_void_p(264)) == INVALID and b"aligned" in lib.dprhot_last_error()
        assert f(code=ctypes.c_void_p(264)) == INVALID and f(q=ctypes.c_void_p(8)) == INVALID
        # cb_check's limits
        assert f(LQ=0) == INVALID and f(LQ=513) == INVALID and b"LQ=513" in lib.dprhot_last_error()
        assert f(n=2 ** 31) == INVALID and b"corpus_len" in lib.dprhot_last_error() and f(n=0) == INVALID
        assert f(nb=2 ** 36) == INVALID and b"2^36" in lib.dprhot_last_error() and f(nb=-1) == INVALID
        assert f(pool=2) == INVALID and f(pool=-1) == INVALID and f(nq=0) == INVALID
        assert f(nb=0, code=None, rows=None, **({"S": None} if f is score else {"vals": None})) == INVALID  # (still validated with no block)
    assert score(ld=63) == INVALID and score(cols=0) == INVALID and score(b=-1) == INVALID
    assert score(b=40, cols=64) == INVALID and b"outside the corpus" in lib.dprhot_last_error()
    assert search(k=0) == INVALID and search(k=101) == INVALID and b"topk" in lib.dprhot_last_error()
    assert search(chunk=12) == INVALID and search(chunk=0) == INVALID and search(b=50, e=40) == INVALID and search(e=101) == INVALID
    assert search(wsb=16) == -4 and search(k=5000, n=6000, e=6000, wsb=2 * 64 * 4) == -4


def test_colbert_pq_kernels_never_spill_and_every_instance_is_there():
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
    mine = {k: v for k, v in rows.items() if re.search(r"dprhot\d+cbpq_\w+_kernel", k)}
    # cbpq_score_kernel<DSUB, KS>: DSUB in {2, 4, 8} x KS = dp / 32 in {1, 2, 3, 4}, what cbpq_launch can reach
    want = {f"cbpq_score_kernelILi{dsub}ELi{ks}EEE" for dsub in (2, 4, 8) for ks in (1, 2, 3, 4)}
    assert len(mine) == 12 and all(any(w in k for k in mine) for w in want), sorted(mine)
    for name, r in mine.items():
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert not re.search(r"dprhot\d+cb_\w+_kernel", name)
    assert len([k for k in rows if re.search(r"dprhot\d+cb_\w+_kernel", k)]) == 5  # the dense kernels, as they were
    assert len([k for k in rows if re.search(r"dprhot\d+pq_encode_kernel", k)]) == 3  # the encode entry launches the existing kernels


def test_lossless_grid_meets_its_precondition():
    """The GPU suite's lossless case draws token rows from a grid with at most 256 distinct sub-vectors per subspace; checked here on
    the dense reference alone, and end to end through the stand-in."""
    G = PS
    for dsub in (2, 4, 8):
        q, passages = G.grid_corpus(dsub)
        rows = torch.cat(passages).to(BF16)
        assert torch.equal(rows.float(), torch.cat(passages)) and rows.shape[1] == 128
        sub = rows.float().view(rows.shape[0], 128 // dsub, dsub)
        assert max(torch.unique(sub[:, j], dim=0).shape[0] for j in range(128 // dsub)) <= 256
    kn = PS.ColbertPQKernels()
    q, passages = G.grid_corpus(8)
    lens = [p.shape[0] for p in passages][:6]
    rows = torch.cat(passages[:6])
    dense = colbert.ColBERTIndex(list(range(6)), lens, rows, 6, "cpu", kernels=kn)
    pq = dense.quantize(dsub=8, iters=1, train_size=rows.shape[0])
    assert torch.equal(pq.decode().tok, dense.tok)
