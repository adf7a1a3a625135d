"""Product-quantised postings on the MI355X (csrc/ivf_pq.h through dprhot_pq_encode / dprhot_ivf_pq_score / dprhot_ivf_pq_search;
DESIGN.md section 10.2).  Nothing here has a tolerance but the Lloyd test's 1e-6 (the bf16 rounding of the centroids is not part of
Lloyd's monotonicity argument): the PQ search must equal the dense search over the decoded rows bit for bit, the codes must equal
the numpy restatement of the encode rule (tests/_pq_oracle.py), and grid rows must survive quantisation exactly."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ivf_pack_inputs as I  # noqa: E402
import _pq_oracle as PO  # noqa: E402
from dpr_scale_amd import ivf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
NDOCS, V = 300, 80
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def kn():
    from dpr_scale_amd.hotpath import HipKernels

    assert torch.cuda.is_available(), "needs a HIP device"
    return HipKernels()


def _postings(seed):
    """(post_doc int32 [P], exp_off int64 [V + 1]), P about 5000, sorted by (expert, doc): expert 0 has 200 postings inside doc ids
    0 .. 127 (more than 64 in one 128-doc range: a second trip of the posting loop, and runs of several postings per doc), experts
    70 .. 79 have none."""
    g = np.random.default_rng(seed)
    docs, counts = [], []
    for e in range(V):
        n = 0 if e >= 70 else int(g.integers(30, 110))
        ids = np.sort(g.integers(0, NDOCS, size=n))
        if e == 0:
            ids = np.sort(np.concatenate([g.integers(0, 128, size=200), g.integers(128, NDOCS, size=60)]))
        docs.append(ids)
        counts.append(len(ids))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return torch.from_numpy(np.concatenate(docs).astype(np.int32)), torch.from_numpy(off)


def _queries(seed, d, nq=6):
    """Query dicts: every query lists expert 0 four times (24 entries of one expert in the batch: a second entry group), the batch
    covers experts 1 .. 68 (more than 64 distinct batch experts), expert 75 (in the index's range, no postings) and expert 1000
    (beyond it)."""
    g = torch.Generator().manual_seed(seed)
    vec = lambda: torch.randn(d, generator=g)
    out = []
    for n in range(nq):
        q = {0: [vec() for _ in range(4)]}
        for e in range(1 + n, 69, 3):
            q[e] = [vec()]
        for e in range(1 + 2 * n, 69, 7):
            q.setdefault(e, []).append(vec())
        out.append(q)
    out[1][75] = [vec()]
    out[2][1000] = [vec()]
    assert len(set().union(*out)) > 64 + 2
    return out


def _pq_index(seed, dsub, dp, d, dc, kn):
    g = torch.Generator().manual_seed(seed)
    post_doc, exp_off = _postings(seed)
    P = post_doc.shape[0]
    assert 4500 < P < 6000 and int((post_doc[: int(exp_off[1])] < 128).sum()) > 64
    codes = torch.randint(0, 256, (P, dp // dsub), generator=g).to(torch.uint8)
    codebook = torch.randn(dp // dsub, 256, dsub, generator=g).to(BF16)
    cls = None
    if dc:
        cls = torch.cat([torch.randn(NDOCS, dc, generator=g).to(BF16), torch.zeros((8, dc), dtype=BF16)], 0).to(DEV)
    return ivf.IVFPQIndex.from_packed(post_doc.to(DEV), codes.to(DEV), codebook.to(DEV), exp_off.to(DEV), cls, NDOCS, d, kernels=kn)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dsub,dp,d", [(2, 32, 32), (4, 32, 32), (8, 32, 32), (2, 64, 64), (4, 64, 64), (8, 64, 64), (4, 32, 24)])
def test_search_equals_the_dense_search_over_the_decoded_rows(kn, dsub, dp, d):
    for dc in (0, 16):
        pq = _pq_index(7 + dsub + dp, dsub, dp, d, dc, kn)
        dense = pq.decode()
        assert dense.post_vec.shape == (pq.n_postings, dp) and pq.nbytes < dense.nbytes
        g = torch.Generator().manual_seed(5)
        cls_q = torch.randn(6, dc, generator=g) if dc else []
        qb = ivf.pack_queries(cls_q, _queries(11, d), None).to(DEV)
        assert int((qb.boff[1:] - qb.boff[:-1]).max()) > 16 and qb.bexp.shape[0] > 64 and qb.ent_vec.shape[1] == dp
        for topk in (1, 50):
            want = dense.search_packed(qb, topk)
            assert _same(pq.search_packed(qb, topk), want)
            assert _same(pq.search_packed(qb, topk, chunk=136), dense.search_packed(qb, topk, chunk=136))  # not a multiple of 128
            assert _same(pq.search_packed(qb, topk, chunk=136), want)
            assert _same(pq.search_packed(qb, topk, id_ranges=[(150, NDOCS), (0, 150)], chunk=64), want)
    # dprhot_ivf_pq_score alone, added into a pre-filled S (the last index: no CLS part in these calls)
    S = torch.randn((6, NDOCS), generator=torch.Generator().manual_seed(9)).to(DEV)
    S2 = S.clone()
    kn.ivf_pq_score(pq, qb, 0, NDOCS, S)
    kn.ivf_score(dense, qb, 0, NDOCS, S2)
    assert torch.equal(S, S2) and not torch.equal(S, torch.randn((6, NDOCS), generator=torch.Generator().manual_seed(9)).to(DEV))
    S3 = torch.zeros((6, 104), device=DEV)
    S4 = S3.clone()
    kn.ivf_pq_score(pq, qb, 200, 100, S3)  # a range that starts inside the corpus, ld > cols
    kn.ivf_score(dense, qb, 200, 100, S4)
    assert torch.equal(S3, S4) and bool(S3.any()) and not bool(S3[:, 100:].any())


def test_runs_are_bit_identical_and_independent_of_chunk_and_batch(kn):
    pq = _pq_index(3, 4, 32, 32, 16, kn)
    queries = _queries(13, 32)
    cls_q = torch.randn(6, 16, generator=torch.Generator().manual_seed(2))
    whole = (NDOCS + 7) // 8 * 8
    ref = pq.search(cls_q, queries, None, 50, chunk=whole)
    assert _same(pq.search(cls_q, queries, None, 50, chunk=whole), ref)  # property A
    for chunk in (8, 136):  # property B: the chunk
        assert _same(pq.search(cls_q, queries, None, 50, chunk=chunk), ref), chunk
    for n in (0, 2, 5):  # property B: the other queries of the batch
        v, i = pq.search(cls_q[n:n + 1], queries[n:n + 1], None, 50)
        assert torch.equal(v, ref[0][n:n + 1]) and torch.equal(i, ref[1][n:n + 1]), n
    v, i = pq.search(cls_q[3:], queries[3:], None, 50, chunk=136)
    assert torch.equal(v, ref[0][3:]) and torch.equal(i, ref[1][3:])


def test_wide_k_equals_the_dense_search_and_is_independent_of_the_chunk(kn):
    """k beyond 4096: the chunk driver folds with the HBM-resident selection (dprhot_topk_update_wide), five chunks of 1024 doc ids
    (the last one ragged) against one chunk of the whole corpus, and against the dense search over the decoded rows."""
    ndocs, k = 5003, 4500
    g = np.random.default_rng(61)
    docs = [np.sort(g.integers(0, ndocs, size=int(g.integers(30, 110)))) for _ in range(70)]
    post_doc = torch.from_numpy(np.concatenate(docs).astype(np.int32))
    exp_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64))
    tg = torch.Generator().manual_seed(62)
    codes = torch.randint(0, 256, (post_doc.shape[0], 8), generator=tg).to(torch.uint8)
    codebook = torch.randn(8, 256, 4, generator=tg).to(BF16)
    cls = torch.cat([torch.randn(ndocs, 16, generator=tg).to(BF16), torch.zeros((8, 16), dtype=BF16)], 0)
    pq = ivf.IVFPQIndex.from_packed(post_doc.to(DEV), codes.to(DEV), codebook.to(DEV), exp_off.to(DEV), cls.to(DEV), ndocs, 32, kernels=kn)
    qb = ivf.pack_queries(torch.randn(6, 16, generator=tg), _queries(63, 32), None).to(DEV)
    got = pq.search_packed(qb, k, chunk=1024)
    assert got[0].shape == (6, k) and bool((got[1] >= 0).all()) and bool((got[1] < ndocs).all())
    assert bool((got[0][:, :-1] >= got[0][:, 1:]).all()) and all(len(set(row)) == k for row in got[1].tolist())
    assert _same(got, pq.decode().search_packed(qb, k, chunk=1024))
    assert _same(got, pq.search_packed(qb, k, chunk=5008))


def _encode_between_bands(rows, codebook):
    """dprhot_pq_encode through ctypes alone; the codes sit between two 4 KiB bands that must come back intact."""
    from dpr_scale_amd import _lib

    n, dp = rows.shape
    m, _, dsub = codebook.shape
    raw = torch.full((n * m + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    codes = raw[GUARD:GUARD + n * m]
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    _lib.check(_lib.lib.dprhot_pq_encode(p(rows), n, dp, ctypes.c_void_p(codebook.data_ptr()), dsub, p(codes),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "dprhot_pq_encode")
    torch.cuda.synchronize()
    assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[GUARD + n * m:] == PATTERN).all()), "guard band overwritten"
    return codes.view(n, m).clone()


@pytest.mark.parametrize("dsub,dp", [(2, 32), (4, 32), (8, 32), (4, 64)])
def test_encode_equals_the_oracle(kn, dsub, dp):
    g = torch.Generator().manual_seed(40 + dsub + dp)
    m = dp // dsub
    rows = torch.randn(1000, dp, generator=g).to(BF16)
    codebook = torch.randn(m, 256, dsub, generator=g).to(BF16)
    # planted: an exact two-way tie (centroids 3 and 7 of subspace 1 are mirror images around row 0's sub-vector, everything else is
    # far away: 3 wins), equal centroids (5 and 250 of subspace 0: 5 wins wherever they are nearest), a row of NaNs
    rows[0, dsub:2 * dsub] = 0.5
    sub = rows[0, dsub:2 * dsub].float()
    delta = torch.full((dsub,), 0.25)
    codebook[1] = 100.0
    codebook[1, 3], codebook[1, 7] = (sub + delta).to(BF16), (sub - delta).to(BF16)
    assert torch.equal(codebook[1, 3].float() - sub, sub - codebook[1, 7].float())  # (exact in bf16: the tie is a tie)
    codebook[0, 250] = codebook[0, 5]
    rows[1] = float("nan")
    rows[2, 0] = float("inf")
    want = PO.encode(rows.float().numpy(), codebook.float().numpy())
    assert want[0, 1] == 3 and not want[1].any() and not (want[:, 0] == 250).any()
    got = _encode_between_bands(rows.to(DEV), codebook.to(DEV))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(kn.pq_encode(rows.to(DEV), codebook.to(DEV)), got)
    for n in (0, 1):
        got = _encode_between_bands(rows[:n].to(DEV), codebook.to(DEV))
        assert got.shape == (n, m) and np.array_equal(got.cpu().numpy(), want[:n])
    assert kn.pq_encode(rows[:0].to(DEV), codebook.to(DEV)).shape == (0, m)


def _grid_rows(seed, n, dp, dsub, points):
    """bf16 rows whose sub-vectors come from exactly `points` distinct grid points per subspace (multiples of 1/4, magnitude <= 4);
    every point occurs."""
    g = torch.Generator().manual_seed(seed)
    m = dp // dsub
    rows = torch.empty(n, m, dsub)
    for j in range(m):
        cells = torch.unique(torch.randint(0, 33 ** dsub, (4 * points,), generator=g))  # distinct cells of the 33^dsub grid
        cells = cells[torch.randperm(cells.shape[0], generator=g)[:points]]
        assert cells.shape[0] == points
        pts = torch.stack([(cells // 33 ** t) % 33 for t in range(dsub)], 1).float() * 0.25 - 4.0
        pick = torch.cat([torch.randperm(points, generator=g), torch.randint(0, points, (n - points,), generator=g)])
        rows[:, j] = pts[pick]
    assert float(rows.abs().max()) <= 4.0
    return rows.reshape(n, dp).to(BF16)


@pytest.mark.parametrize("dsub,points", [(2, 256), (4, 256), (8, 256), (4, 40)])
def test_grid_rows_survive_quantisation_exactly(kn, dsub, points):
    post_doc, exp_off = _postings(21)
    P = post_doc.shape[0]
    rows = _grid_rows(50 + dsub, P, 32, dsub, points).to(DEV)
    dense = ivf.IVFIndex.from_packed(post_doc.to(DEV), rows, exp_off.to(DEV), None, NDOCS, 32, kernels=kn)
    codebook = ivf.train_pq(rows, dsub=dsub, iters=3, train_size=P, seed=1, kernels=kn)
    assert codebook.dtype == BF16 and codebook.shape == (32 // dsub, 256, dsub)
    if points < 256:
        assert not bool(codebook[:, points:].any())  # the slots beyond the distinct sub-vectors are zeros
    assert torch.equal(ivf.pq_decode(kn.pq_encode(rows, codebook), codebook).view(torch.int16), rows.view(torch.int16))
    pq = dense.quantize(dsub=dsub, iters=3, train_size=P, seed=1)
    assert type(pq) is ivf.IVFPQIndex and torch.equal(pq.codebook, codebook) and not hasattr(pq, "post_vec")
    assert torch.equal(pq.decode().post_vec.view(torch.int16), rows.view(torch.int16))
    qb = ivf.pack_queries([], _queries(17, 32), None).to(DEV)
    for topk in (1, 50):
        assert _same(pq.search_packed(qb, topk), dense.search_packed(qb, topk))
    given = dense.quantize(dsub=dsub, codebook=codebook)
    assert torch.equal(given.post_code, pq.post_code)


def test_training_is_reproducible_and_lloyd_descends(kn):
    rows = torch.randn(6000, 32, generator=torch.Generator().manual_seed(8)).to(BF16).to(DEV)
    seen = []
    a = ivf.train_pq(rows, dsub=4, iters=6, train_size=4000, seed=3, kernels=kn, on_iteration=lambda i, cb: seen.append((i, cb)))
    b = ivf.train_pq(rows, dsub=4, iters=6, train_size=4000, seed=3, kernels=kn)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert [i for i, _ in seen] == list(range(7)) and torch.equal(seen[-1][1], a)
    assert not torch.equal(a, ivf.train_pq(rows, dsub=4, iters=6, train_size=4000, seed=4, kernels=kn))
    # the error Lloyd's argument is about: the training sample's, after the initialisation and after every iteration
    sample = rows[torch.randperm(6000, generator=torch.Generator().manual_seed(3))[:4000].sort().values.to(DEV)]
    sse = []
    for _, cb in seen:
        dec = ivf.pq_decode(kn.pq_encode(sample, cb), cb)
        sse.append(float(((sample.double() - dec.double()) ** 2).sum()))
    print("total squared error of the sample, initialisation then six Lloyd iterations:", " ".join(f"{e:.6f}" for e in sse))
    for before, after in zip(sse[:-1], sse[1:]):
        assert after <= before * (1 + 1e-6), sse
    assert sse[-1] < sse[0]


def test_round_trips(kn, tmp_path):
    cr = I.gaussian_repr(31, B=200, L=12, K=3, d=32, n_experts=40)
    qr = I.gaussian_repr(32, B=5, L=9, K=3, d=32, n_experts=40)
    g = torch.Generator().manual_seed(33)
    cr["cls_repr"], qr["cls_repr"] = torch.randn(200, 16, generator=g), torch.randn(5, 16, generator=g)
    b = ivf.IndexBuilder(200, kernels=kn)
    b.add(I.to_device(cr, DEV), torch.arange(200))
    train = dict(iters=4, train_size=1000, seed=5)
    pq = b.finish(quantizer="pq", sub_vec_dim=4, **train)
    dense = b.finish()
    want = dense.quantize(dsub=4, **train)
    assert type(pq) is ivf.IVFPQIndex and pq.n_postings == dense.n_postings > 1000

    def same_pq(x, y):
        assert (x.corpus_len, x.d, x.dp, x.dsub, x.dc, x.n_experts, x.n_postings) == (y.corpus_len, y.d, y.dp, y.dsub, y.dc, y.n_experts,
                                                                                     y.n_postings)
        for k in ("post_doc", "post_code", "codebook", "exp_off", "cls"):
            s, t = getattr(x, k).cpu(), getattr(y, k).cpu()
            assert s.dtype == t.dtype and s.shape == t.shape, k
            assert torch.equal(s.view(torch.int16), t.view(torch.int16)) if s.dtype == BF16 else torch.equal(s, t), k
        return True

    assert same_pq(pq, want)
    # save / load_pq_index
    path = pq.save(str(tmp_path / "pq_index.pt"))
    back = ivf.load_pq_index(path, DEV, kernels=kn)
    assert same_pq(back, pq) and back.nbytes == pq.nbytes
    qb = ivf.pack_queries_device(I.to_device(qr, DEV), qr["cls_repr"].to(DEV), kernels=kn)
    assert _same(back.search_packed(qb, 10), pq.search_packed(qb, 10))
    # the drop-in task over the PQ index against the plain task over the decoded index, packing on the device and on the host
    from dpr_scale_amd.task.citadel_retrieval import CITADELPQRetrievalTask, CITADELRetrievalTask

    out = I.to_device(qr, DEV)

    class Enc(torch.nn.Module):
        def forward(self, token_ids, **kw):
            return dict(out)

    batch = {"query_ids": {"input_ids": torch.zeros((5, 10), dtype=torch.long)}, "topic_ids": [f"t{j}" for j in range(5)]}
    base = dict(ctx_embeddings_dir=str(tmp_path), checkpoint_path="", topk=10, transform=None, model=None, datamodule=None, optim=None)
    results = []
    for cls, index in ((CITADELPQRetrievalTask, back), (CITADELRetrievalTask, pq.decode())):
        for device_pack in (True, False):
            task = cls(**base)
            task.device_pack, task.index, task.query_encoder = device_pack, index, Enc()
            results.append(task._eval_step(batch, 0))
    assert results[0] == results[1] == results[2] == results[3]
    assert len(results[0][1][0]) == 10 and len(set(results[0][1][0])) == 10
    # the task's own loader: the saved file when it is there, otherwise the tree quantised -- and written when save_quantized is set
    task = CITADELPQRetrievalTask(**base)
    task.ctxs = range(200)
    assert same_pq(task._load_index(DEV), pq)
    tree = tmp_path / "tree"
    tree.mkdir()
    b.write(str(tree))
    task = CITADELPQRetrievalTask(**{**base, "ctx_embeddings_dir": str(tree)})
    task.ctxs, task.save_quantized = range(200), True
    built = task._load_index(DEV)
    assert type(built) is ivf.IVFPQIndex and built.n_postings == pq.n_postings and os.path.exists(tree / "pq_index.pt")
    assert same_pq(ivf.load_pq_index(str(tree / "pq_index.pt"), DEV), built)
