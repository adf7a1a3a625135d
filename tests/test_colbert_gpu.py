"""ColBERT retrieval on the MI355X (csrc/colbert.h through dprhot_colbert_score / dprhot_colbert_search).

Grid inputs (tests/golden/colbert_*.npz from the reference's training score, and padded batches against hotpath.expert_score_only) must
come out BIT-EQUAL: retrieval score == training score == rerank score.  Gaussian inputs are compared with the float64 oracle on
bf16-rounded operands under a per-cell bound derived from the arithmetic, not measured (as tests/test_ivf_gpu.py does):
  * a dot product of dp exact products accumulated in fp32 is off by at most dp * 2^-23 * sum_k |q_ik c_jk|; the max over a passage's
    tokens and the clamp at 0 do not enlarge an error, so query token i's term is off by at most dp * 2^-23 * max_j sum_k |q_ik c_jk|;
  * pooling the LQ terms in fp32 is off by at most a further (LQ + 1) * 2^-23 * sum_i |term_i| (nothing under max pooling), and
    |term_i| <= max_j sum_k |q_ik c_jk|.
With A[n, doc] = sum_i max_j sum_k |q_ik c_jk|:  bound[n, doc] = (dp + LQ + 1) * 2^-23 * A[n, doc].
`search` is compared with the total-order top-k of the kernel's own `score` matrix with torch.equal: near-ties cannot make it flaky.
Every input is valid; nothing here provokes a fault."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _colbert_oracle as CO  # noqa: E402
from dpr_scale_amd import colbert  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
LENGTHS = [0, 1, 15, 16, 17, 31, 33, 64, 65, 180, 513]


def load(pool):
    z = np.load(os.path.join(ROOT, "tests", "golden", f"colbert_{pool}.npz"))
    return json.loads(str(z["meta"])), z


def corpus(seed, lengths, d, nq, LQ, q_pad=0):
    """Gaussian passages of the given lengths (doc id = position) and queries, bf16-exact fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    passages = [rnd(n, d) for n in lengths]
    q = rnd(nq, LQ, d)
    if q_pad:
        q[0, LQ - q_pad:] = 0.0
    return q, passages


def build(passages, d, chunk=None, order=None):
    order = list(range(len(passages))) if order is None else order
    rows = torch.cat([passages[i] for i in order], 0) if order else torch.zeros(0, d)
    return colbert.ColBERTIndex(order, [passages[i].shape[0] for i in order], rows, len(passages), DEV, chunk=chunk)


def _banded(raws, nbytes):
    raw = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    raws.append((raw, nbytes))
    return raw[GUARD:GUARD + nbytes]


def _check_bands(raws):
    torch.cuda.synchronize()
    for raw, nb in raws:
        assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[GUARD + nb:] == PATTERN).all()), "guard band overwritten"


_p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def bare_search(index, q, pool, k, chunk, id_ranges=None):
    """dprhot_colbert_search through ctypes alone: values, indices and an exactly sized workspace sit between guard bands."""
    from dpr_scale_amd import _lib

    qb = colbert._bf16_padded(q.to(DEV), index.dp)
    nq, LQ, dp = qb.shape
    n = ctypes.c_size_t(0)
    _lib.check(_lib.lib.dprhot_colbert_workspace_bytes(nq, chunk, ctypes.byref(n)))
    nws = n.value
    if k > 4096:
        _lib.check(_lib.lib.dprhot_topk_wide_workspace_bytes(nq, k, ctypes.byref(n)))
        nws += n.value
    raws = []
    values = _banded(raws, nq * k * 4).view(torch.float32).view(nq, k)
    indices = _banded(raws, nq * k * 8).view(torch.int64).view(nq, k)
    ws = _banded(raws, nws)
    first = 1
    for b, e in (id_ranges or [(0, index.corpus_len)]):
        _lib.check(_lib.lib.dprhot_colbert_search(_p(index.tok), _p(index.doc_blk), index.n_blk, index.corpus_len, dp, _p(qb), nq, LQ, pool, b, e, k,
                                                  chunk, _p(values), _p(indices), first, _p(ws), nws,
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "dprhot_colbert_search")
        first = 0
    _check_bands(raws)
    return values.clone(), indices.clone()


def bare_score(index, q, pool, doc_begin, cols):
    """dprhot_colbert_score through ctypes alone into an exactly sized S [nq, cols] between guard bands."""
    from dpr_scale_amd import _lib

    qb = colbert._bf16_padded(q.to(DEV), index.dp)
    nq, LQ, dp = qb.shape
    raws = []
    S = _banded(raws, nq * cols * 4).view(torch.float32).view(nq, cols)
    _lib.check(_lib.lib.dprhot_colbert_score(_p(index.tok), _p(index.doc_blk), index.n_blk, index.corpus_len, dp, _p(qb), nq, LQ, pool, doc_begin,
                                             cols, _p(S), cols, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "dprhot_colbert_score")
    _check_bands(raws)
    return S.clone()


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_golden_bit_equal(pool):
    meta, z = load(pool)
    q = torch.from_numpy(z["q"])
    index = colbert.ColBERTIndex.from_repr(torch.from_numpy(z["c"]), torch.from_numpy(z["att"]), list(range(meta["N"])), meta["corpus_len"], DEV)
    v, i = index.search(q, meta["topk"], query_pool=pool)
    assert v.device.type == "cuda" and v.dtype == torch.float32 and i.dtype == torch.int64
    assert np.array_equal(v.cpu().numpy(), z["top_values"]) and np.array_equal(i.cpu().numpy(), z["top_ids"])
    v, i = bare_search(index, q, CO.POOL[pool], meta["topk"], 8)
    assert np.array_equal(v.cpu().numpy(), z["top_values"]) and np.array_equal(i.cpu().numpy(), z["top_ids"])
    assert np.array_equal(index.score(q, 0, None, pool).cpu().numpy(), z["scores"])
    assert np.array_equal(bare_score(index, q, CO.POOL[pool], 0, meta["corpus_len"]).cpu().numpy(), z["scores"])


@pytest.mark.parametrize("pool", ["sum", "max"])
@pytest.mark.parametrize("nq,LQ,N,LD,d", [(5, 7, 40, 20, 24), (3, 33, 21, 70, 128)])
def test_grid_inputs_equal_the_rerank_score(pool, nq, LQ, N, LD, d):
    from dpr_scale_amd import hotpath

    lengths = np.random.default_rng(N).permutation(np.resize(np.arange(LD), N))
    q, c, att = CO.make_padded(50 + d, nq, LQ, N, LD, d, lengths=lengths, q_pad=2)
    index = colbert.ColBERTIndex.from_repr(c.to(DEV), att.to(DEV), list(range(N)), N)
    S = index.score(q, 0, None, pool)
    want = hotpath.expert_score_only({"expert_repr": q.to(DEV)}, {"expert_repr": c.to(DEV).repeat(nq, 1, 1)}, query_pool=pool)
    assert want.shape == (nq, N) and torch.equal(S, want)
    assert torch.equal(S.cpu().double(), CO.score(q, CO.passages_of(c, att), pool))


def _cycle(n, seed):
    g = np.random.default_rng(seed)
    return [int(x) for x in g.permutation(np.resize(np.array(LENGTHS), n))]


CASES = {  # corpus_len, lengths, LQ, nq, d, chunks, ks
    "one": ([17], 1, 1, 24, (8,), (1,)),
    "seven": (LENGTHS[:7], 16, 3, 32, (8, 64), (1, 7)),
    "nine": ([64, 65, 180, 513, 0, 1, 33, 16, 15], 17, 8, 96, (8, 64), (1, 9)),
    "129": (_cycle(129, 1), 33, 33, 128, (64, 1024), (10, 129)),
    "1000": ([int(x) for x in np.random.default_rng(2).choice(LENGTHS[:9], 1000)], 32, 3, 128, (8, 64, 4096), (10, 1000)),
    "wide-rows": (_cycle(9, 3), 64, 1, 160, (8,), (9,)),       # dp = 160: the any-width instantiation
    "long-query": (LENGTHS[:7], 130, 2, 32, (8,), (7,)),       # 9 fragments per query: one query per workgroup
    "two-pass": (LENGTHS[:7], 260, 2, 32, (8,), (7,)),         # 17 fragments per query: two passes over the run
}


@pytest.mark.parametrize("pool", ["sum", "max"])
@pytest.mark.parametrize("case", list(CASES))
def test_gaussian_within_the_derived_bound_and_search_is_the_top_k_of_score(case, pool):
    lengths, LQ, nq, d, chunks, ks = CASES[case]
    q, passages = corpus(len(lengths) + LQ, lengths, d, nq, LQ, q_pad=1 if LQ > 1 else 0)
    index = build(passages, d)
    S = index.score(q, 0, None, pool)
    assert S.shape == (nq, len(lengths)) and torch.equal(S, index.score(q, 0, None, pool))  # two runs: the same bits
    want = CO.score(q, passages, pool)
    bound = (index.dp + LQ + 1) * 2.0 ** -23 * CO.magnitude(q, passages)
    err = (S.cpu().double() - want).abs()
    print(f"{case}/{pool}: max err {err.max().item():.3e}, max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())
    empty = [j for j, n in enumerate(lengths) if n == 0]
    assert not S[:, empty].any()
    for k in ks:
        tv, ti = CO.topk(S, k)
        for chunk in chunks:
            v, i = index.search(q, k, query_pool=pool, chunk=chunk)
            assert torch.equal(v, tv) and torch.equal(i, ti), (k, chunk)
    v, i = bare_search(index, q, CO.POOL[pool], ks[-1], chunks[0])
    assert torch.equal(v, tv) and torch.equal(i, ti)
    half = max(1, len(lengths) // 2)
    assert torch.equal(bare_score(index, q, CO.POOL[pool], len(lengths) - half, half), S[:, len(lengths) - half:])


def test_wide_selection_over_many_short_passages():
    n, k = 6000, 5000
    lengths = [int(x) for x in np.random.default_rng(5).integers(1, 4, size=n)]
    q, passages = corpus(77, lengths, 32, 2, 4)
    index = build(passages, 32)
    S = index.score(q)
    tv, ti = CO.topk(S, k)
    v, i = index.search(q, k, chunk=2048)
    assert torch.equal(v, tv) and torch.equal(i, ti)
    v, i = bare_search(index, q, 0, k, 4096, id_ranges=[(0, 1000), (1000, n)])
    assert torch.equal(v, tv) and torch.equal(i, ti)


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_a_cell_depends_on_its_query_and_its_passage_only(pool, tmp_path):
    lengths = _cycle(129, 9)
    d, nq, LQ = 96, 6, 40
    q, passages = corpus(404, lengths, d, nq, LQ, q_pad=3)
    index = build(passages, d)
    S = index.score(q, 0, None, pool)
    v, i = index.search(q, 20, query_pool=pool, chunk=8)
    for kw in (dict(chunk=64), dict(chunk=1024), dict(chunk=16, id_ranges=[(77, 129), (0, 30), (30, 77)])):  # chunk, split id range
        v2, i2 = index.search(q, 20, query_pool=pool, **kw)
        assert torch.equal(v, v2) and torch.equal(i, i2), kw
    assert torch.equal(index.score(q, 40, 50, pool), S[:, 40:90])
    # another batch composition: alone, reversed, and among other queries
    assert torch.equal(index.score(q[2:3], 0, None, pool), S[2:3])
    assert torch.equal(index.score(q.flip(0), 0, None, pool), S.flip(0))
    assert torch.equal(index.score(torch.cat([q[4:], torch.ones(9, LQ, d), q[:1]]), 0, None, pool)[[0, 1, 11]], S[[4, 5, 0]])
    # other passages in the index: a sub-corpus in another order of arrival
    sel = list(range(128, 0, -3))
    sub = build([passages[j] for j in sel], d)
    assert torch.equal(sub.score(q, 0, None, pool), S[:, sel])
    shuffled = build(passages, d, order=[int(x) for x in np.random.default_rng(0).permutation(129)])
    assert torch.equal(shuffled.tok, index.tok) and torch.equal(shuffled.doc_blk, index.doc_blk)
    # another rank sharding on disk
    att = [torch.ones(1, p.shape[0]) for p in passages]
    for name, shards in (("one", [list(range(129))]), ("three", [list(range(0, 129, 3)), list(range(2, 129, 3)), list(range(1, 129, 3))])):
        for rank, ids in enumerate(shards):
            b = colbert.TokenIndexBuilder()
            for j in ids:
                if passages[j].shape[0]:
                    b.add(passages[j].unsqueeze(0).to(DEV), att[j], [j])
            b.write(str(tmp_path / name), rank)
        loaded = colbert.load_index(str(tmp_path / name), 129, DEV)
        assert torch.equal(loaded.tok, index.tok) and torch.equal(loaded.score(q, 0, None, pool), S)
        v2, i2 = loaded.search(q, 20, query_pool=pool)
        assert torch.equal(v, v2) and torch.equal(i, i2)


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_semantics(pool):
    u = torch.tensor([1.0, -2.0, 0.5, 3.0] * 8)
    w = torch.tensor([0.5, -1.0, 1.0, 0.25] * 8)
    nan_row = torch.full((32,), float("nan"))
    passages = [
        torch.stack([-u, -2 * u]),         # 0: all negative against u -> 0
        torch.zeros(0, 32),                # 1: empty -> 0
        torch.stack([u]),                  # 2: <u, u>
        torch.stack([w, u, -u]),           # 3: the same best token as 2: a tie
        torch.stack([nan_row, w]),         # 4: the NaN token counts as absent -> as passage 5
        torch.stack([w]),                  # 5
        torch.stack([nan_row]),            # 6: nothing but a NaN token -> 0
    ]
    index = build(passages, 32)
    q = torch.stack([torch.stack([u, torch.zeros(32)]), torch.stack([u, w])])  # query 0: one real token and one padded token
    S = index.score(q, 0, None, pool).cpu()
    uu, uw = float(u @ u), float(u @ w)
    assert uw > 0 and S[0].tolist() == [0.0, 0.0, uu, uu, uw, uw, 0.0]
    assert torch.equal(S.double(), CO.score(q, passages, pool))  # (grid values: exact)
    assert torch.equal(S[0:1], index.score(q[0:1, 0:1], 0, None, pool).cpu())  # the padded query token added 0
    v, i = index.search(q[0:1], 7, query_pool=pool)
    assert i[0].tolist() == [2, 3, 4, 5, 0, 1, 6] and v[0].tolist() == [uu, uu, uw, uw, 0.0, 0.0, 0.0]  # ties to the lower id
    assert not torch.isnan(index.score(q, 0, None, pool)).any()
