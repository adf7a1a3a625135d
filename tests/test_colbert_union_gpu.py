"""The candidate stage of the pruned ColBERT search on the MI355X (csrc/colbert_union.h).

Every comparison is torch.equal / list equality: the lists are integers.  The oracle is `_colbert_cand_standin.union_of_lists` on the
host; hostile inputs (ids outside [0, C), offsets that run backwards or past the end, doc ids outside the corpus) reach it through
`_colbert_union_standin.clean_lists` / `clean_ids`, which restate the header's reading of them as well-formed lists.

The raw entry points run through ctypes alone with cand_off, totals, cand_doc and a workspace of exactly the size asked for between
guard bands, at corpus sizes around every tiling constant of the kernels: the 32-bit bitmap word and the 8192 doc ids of a block of
the count and fill passes (one, two and three blocks per query)."""
import copy
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _capture_cases as CC  # noqa: E402
import _colbert_cand_standin as CS  # noqa: E402
import _colbert_union_standin as US  # noqa: E402
import test_colbert_cand_gpu as CAND  # noqa: E402
import test_stream_capture_gpu as CAP  # noqa: E402
from dpr_scale_amd import colbert  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
WORD, BLK = 32, 8192  # doc ids per bitmap word; per block of the count and the fill pass (UN_BLK_DOCS)
DP = 32

_p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _banded(raws, nbytes, dtype=torch.uint8):
    raw = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    raws.append((raw, nbytes))
    return raw[GUARD:GUARD + nbytes].view(dtype)


def _check_bands(raws):
    torch.cuda.synchronize()
    for raw, nb in raws:
        assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[GUARD + nb:] == PATTERN).all()), "guard band overwritten"


# ---- hand-made inputs ----------------------------------------------------------------------------------------------------------------
def make_case(corpus_len, nq, LQ, nprobe, C, seed=0, hostile=True):
    """(cids int64 [nq, LQ, nprobe], qb bf16 [nq, LQ, 32], cen_off int64 [C + 1], cen_doc int32) on the host.  Lists overlap across
    tokens and centroids (ids are drawn from few centroids, doc ids from a corpus the lists cover several times at small sizes), some
    are empty, and both ends of the corpus (0 and corpus_len - 1, the last bit of the last word) are listed.  hostile: doc ids < 0 and
    >= corpus_len inside cen_doc, a pair of cen_off that runs backwards, one that points past n_list and a negative one; probed ids
    >= C and < 0; a NaN token with ids -1; a token of -0.0 only; a query of padding only in the middle and one at the end."""
    rng = np.random.default_rng(1000 * seed + corpus_len % 997 + 7 * nq + LQ + nprobe)
    per_list = []
    for c in range(C):
        n = 0 if c % 5 == 3 else int(rng.integers(1, 24))
        docs = sorted(set(int(v) for v in rng.integers(0, corpus_len, size=n)))
        if c % 4 == 0:
            docs = sorted(set(docs + [0, corpus_len - 1]))
        if c % 6 == 1 and corpus_len > BLK:  # a run across a block boundary, every bit of two neighbouring words
            docs = sorted(set(docs + list(range(BLK - WORD, BLK + WORD))))
        if hostile and c % 3 == 2:
            docs = [-1] + docs + [corpus_len, corpus_len + 7, -(2 ** 31), 2 ** 31 - 1]
        per_list.append(docs)
    off = np.cumsum([0] + [len(x) for x in per_list]).astype(np.int64)
    flat = np.array([j for x in per_list for j in x], dtype=np.int64)
    if hostile:
        off[C] += 1000                    # the last list points past n_list
        if C >= 8:
            off[2] = off[4] + 1           # list 1 grows into its neighbours, list 2 runs backwards: empty
            off[6] = -3                   # a negative offset: clamped to 0 (list 5 empty, list 6 from the start)
    cids = rng.integers(0, C, size=(nq, LQ, nprobe)).astype(np.int64)
    q = rng.standard_normal((nq, LQ, DP)).astype(np.float32)
    qb = torch.from_numpy(q).to(torch.bfloat16)
    cids = torch.from_numpy(cids)
    if hostile and cids.numel() >= 8:     # (a single probe stays as it is: the smallest shapes must still mark something)
        cids[0, 0, 0] = C                 # ids >= C and < 0: skipped
        cids[nq - 1, LQ - 1, nprobe - 1] = C + 12345
        cids[nq // 2, LQ // 2, 0] = -7
    if hostile and LQ > 1:
        qb[0, LQ - 1] = -0.0              # -0.0 only: not live
        qb[0, 1] = float("nan")           # a NaN token is live; the probe gives it -1
        cids[0, 1] = -1
        qb[0, 0, 1:] = 0                  # one non-zero feature is enough
    if hostile and nq >= 3:
        qb[1] = 0                         # padding only, in the middle
        qb[nq - 1] = 0                    # padding only, last
        qb[2, 0] = -0.0                   # (and a -0.0 token where LQ = 1)
    return cids, qb, torch.from_numpy(off), torch.from_numpy(flat).to(torch.int32)


def oracle(case, corpus_len):
    cids, qb, cen_off, cen_doc = case
    C = cen_off.shape[0] - 1
    off, docs = US.clean_lists(cen_off.tolist(), cen_doc.tolist(), C, corpus_len)
    return CS.union_of_lists(US.clean_ids(cids, C), US.live_tokens(qb), off, docs)


def bare_union(case, corpus_len, capacity=None, ws_byte=PATTERN):
    """dprhot_colbert_union_count then _fill through ctypes alone: (cand_off, totals, cand_doc) as host lists.  `capacity` (default: the
    n_cand the count reports, read on the host) is the length cand_doc is allocated with; every buffer sits between guard bands and
    cand_doc starts filled with -1."""
    from dpr_scale_amd import _lib

    cids, qb, cen_off, cen_doc = (t.to(DEV).contiguous() for t in case)
    nq, LQ, nprobe = cids.shape
    C, n_list = cen_off.shape[0] - 1, cen_doc.shape[0]
    nws = _lib.colbert_union_workspace_bytes(nq, corpus_len)
    raws = []
    cand_off, totals, ws = _banded(raws, (nq + 1) * 8, torch.int64), _banded(raws, 16, torch.int64), _banded(raws, nws)
    ws.fill_(ws_byte)
    _lib.check(_lib.lib.dprhot_colbert_union_count(_p(cids), _p(qb), DP, nq, LQ, nprobe, C, _p(cen_off), _p(cen_doc), n_list, corpus_len,
                                                   _p(cand_off), _p(totals), _p(ws), nws, _stream()), "dprhot_colbert_union_count")
    n_cand = int(totals[0])
    cap = n_cand if capacity is None else capacity
    cand_doc = _banded(raws, cap * 4, torch.int32)
    cand_doc.fill_(-1)
    _lib.check(_lib.lib.dprhot_colbert_union_fill(nq, corpus_len, _p(cand_off), _p(cand_doc), cap, _p(ws), nws, _stream()),
               "dprhot_colbert_union_fill")
    _check_bands(raws)
    return cand_off.tolist(), totals.tolist(), cand_doc.tolist()


def _sizes(off):
    return [b - a for a, b in zip(off, off[1:])]


CORPUS_LENS = [1, WORD - 1, WORD, WORD + 1, BLK - 1, BLK, BLK + 1, 2 * BLK - 1, 2 * BLK, 2 * BLK + 1, 3 * BLK - 1, 3 * BLK, 3 * BLK + 1]
_SHAPES = [(nq, LQ, nprobe) for nq in (1, 2, 33) for LQ in (1, 16, 33) for nprobe in (1, 4)]  # 18
_CS = (4, 9, 16, 64)
# every corpus size with a shape of the cycle, then every shape at a block, a word and one (two blocks per query)
CASES = [(n, *_SHAPES[(5 * i) % 18], _CS[i % 4]) for i, n in enumerate(CORPUS_LENS)]
CASES += [(BLK + WORD + 1, *s, _CS[i % 4]) for i, s in enumerate(_SHAPES)]


@pytest.mark.parametrize("corpus_len,nq,LQ,nprobe,C", CASES)
def test_count_and_fill_equal_the_union_of_lists(corpus_len, nq, LQ, nprobe, C):
    case = make_case(corpus_len, nq, LQ, nprobe, C)
    off, docs = oracle(case, corpus_len)
    sizes = _sizes(off)
    assert sum(sizes) > 0
    got = bare_union(case, corpus_len)
    assert got[0] == off and got[1] == [sum(sizes), max(sizes)] and got[2] == docs
    # two runs, and a run over a scribbled workspace, are bit-identical
    assert bare_union(case, corpus_len) == got
    assert bare_union(case, corpus_len, ws_byte=0x3C) == got
    assert bare_union(case, corpus_len, ws_byte=0xFF) == got
    # a longer cand_doc keeps its tail; a shorter one is cut at the capacity (its guard band is checked by bare_union)
    n = len(docs)
    assert bare_union(case, corpus_len, capacity=n + 5)[2] == docs + [-1] * 5
    for cap in sorted({0, 1, n // 2, max(n - 1, 0)}):
        assert bare_union(case, corpus_len, capacity=cap)[2] == docs[:cap], cap


def test_well_formed_lists_give_the_same_as_hostile_ones_cleaned():
    """The same shape without a hostile entry: every list, every id and every token is used."""
    for corpus_len, nq, LQ, nprobe, C in ((2 * BLK + 1, 2, 16, 4, 16), (WORD + 1, 33, 1, 1, 4)):
        case = make_case(corpus_len, nq, LQ, nprobe, C, seed=1, hostile=False)
        off, docs = CS.union_of_lists(case[0], US.live_tokens(case[1]), case[2].tolist(), case[3].tolist())
        got = bare_union(case, corpus_len)
        assert got[0] == off and got[2] == docs and len(docs) > 0 and got[1] == [len(docs), max(_sizes(off))]


def test_no_list_entries_at_all_and_a_null_cen_doc():
    cids, qb, _, _ = make_case(BLK + 1, 2, 16, 4, 9, hostile=False)
    case = (cids, qb, torch.zeros(10, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    assert bare_union(case, BLK + 1) == ([0, 0, 0], [0, 0], [])
    hostile = (cids, qb, torch.tensor([0, 5, -2, 3, 2 ** 40, 1, 0, 0, 9, 9], dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    assert bare_union(hostile, BLK + 1, capacity=3) == ([0, 0, 0], [0, 0], [-1, -1, -1])


# ---- an index from build_centroids, dense and residual ---------------------------------------------------------------------------------
class WithoutUnion:
    """A kernel set that hides the colbert_union_* methods of the one it wraps: what a kernel set written before them looks like."""

    def __init__(self, kn):
        self._kn = kn

    def __getattr__(self, name):
        if name.startswith("colbert_union"):
            raise AttributeError(name)
        return getattr(self._kn, name)


@functools.lru_cache(maxsize=None)
def pruned_index(shape, kind):
    """(q, index with 16 grid centroids over the corpus of tests/test_colbert_cand_gpu.py, the same index on the torch route)."""
    q, _, index = CAND.corpus(shape, 5)
    dense = colbert.ColBERTIndex.from_packed(index.tok, index.doc_blk, CAND.NP, index.d)
    cen = torch.from_numpy(np.random.default_rng(8).integers(-4, 5, size=(16, index.d)).astype(np.float32) / 4.0)
    dense.build_centroids(16, centroids=cen)
    new = dense if kind == "dense" else dense.compress(2)
    old = copy.copy(new)
    old.kn = WithoutUnion(new._kernels())
    assert hasattr(new._kernels(), "colbert_union_count") and not hasattr(old._kernels(), "colbert_union_count")
    return q, new, old


def _same_union(got, want):
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and all(type(v) is int for v in got[2:])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:] == want[2:]


@pytest.mark.parametrize("batches", [1, 3])
@pytest.mark.parametrize("shape,kind", [("d24", "dense"), ("d128", "dense"), ("d24", "residual"), ("d128", "residual")])
def test_union_and_search_pruned_equal_the_torch_route(shape, kind, batches, monkeypatch):
    from dpr_scale_amd import _lib

    q, new, old = pruned_index(shape, kind)
    if batches == 3:
        monkeypatch.setattr(colbert, "UNION_WS_BYTES", 2 * _lib.colbert_union_workspace_bytes(1, CAND.NP))
    assert len(new._union_batches(5)) == batches
    qb = new._queries(q)
    for nprobe in (1, 2, 16):
        cids = new._probe(qb, nprobe)
        got = new._union(qb, cids)
        _same_union(got, new._union_torch(qb, cids))
        _same_union(old._union(qb, cids), got)
        off, docs = CS.union_of_lists(cids.cpu(), (q != 0).any(2), new.cen_off.tolist(), new.cen_doc.tolist())
        assert got[0].tolist() == off and got[1].tolist() == docs and got[2] == len(docs) and got[3] == max(_sizes(off))
        a, b = new.candidates(q, nprobe)
        assert torch.equal(a, got[0]) and torch.equal(b, got[1])
    for pool in ("sum", "max"):
        for ndocs in (None, 12):
            v, i = new.search_pruned(q, 10, 2, query_pool=pool, ndocs=ndocs)
            ov, oi = old.search_pruned(q, 10, 2, query_pool=pool, ndocs=ndocs)
            assert torch.equal(CAP.bits(v), CAP.bits(ov)) and torch.equal(i, oi), (pool, ndocs)
    assert new.latency["candidate_time"] > 0
    # a batch of padding only
    z = torch.zeros(2, 3, new.d)
    a, b = new.candidates(z, 2)
    assert a.tolist() == [0, 0, 0] and b.numel() == 0 and b.dtype == torch.int32


# ---- capture and side stream: count + fill at a fixed capacity ------------------------------------------------------------------------
CAP_SHAPE = dict(corpus_len=2 * BLK + 1, nq=5, LQ=7, nprobe=2, C=9)
CAPACITY = 480
SYMBOLS = ("dprhot_colbert_union_count", "dprhot_colbert_union_fill")


def _capture_build():
    """A and B differ in structure: B probes other ids, its query 2 becomes empty (padding only), query 0 -- empty in A -- gets
    tokens, and list 1 grows by what list 0 loses (other offsets over the same doc ids).  cand_doc has a fixed capacity between the two
    totals: it cuts the longer set of lists, and behind the shorter one the entries keep the sentinel."""
    kn = CC.kernels()[0]
    n, nq = CAP_SHAPE["corpus_len"], CAP_SHAPE["nq"]
    cids_a, q_a, off_a, doc = make_case(**CAP_SHAPE, seed=2, hostile=False)
    cids_b, q_b, _, _ = make_case(**CAP_SHAPE, seed=3, hostile=False)
    q_a[0] = 0
    q_b[2] = 0
    off_b = off_a.clone()
    off_b[1] = max(int(off_a[1]) - 3, 0)
    off_b[5] = int(off_a[6])
    A = [CC.dv(cids_a), CC.dv(q_a), CC.dv(off_a), CC.dv(doc)]
    B = [CC.dv(cids_b), CC.dv(q_b), CC.dv(off_b), CC.dv(doc.flip(0).contiguous())]
    cand_off, totals = CC.empty((nq + 1,), torch.int64), CC.empty((2,), torch.int64)
    cand_doc = CC.empty((CAPACITY,), torch.int32)

    def fn(x):
        I = CC._ns(cen_off=x[2], cen_doc=x[3], corpus_len=n)
        ws = kn.colbert_union_workspace(nq, n, x[0])
        kn.colbert_union_count(I, x[0], x[1], cand_off, totals, ws)
        kn.colbert_union_fill(I, cand_off, cand_doc, ws)
        return ()

    return CC.Built(A, B, fn, outs=[cand_off, totals, cand_doc], ws=lambda: [kn._workspace(A[0].device, 1)])


UNION_CASE = CC.Case("colbert_union", SYMBOLS, _capture_build)


@CAP.ends_the_session_on_a_device_fault
def test_side_stream_and_replay_equal_the_eager_call():
    assert UNION_CASE.name not in [c.name for c in CC.CASES]  # a row of this file's own: the table keeps its pinned length
    built = UNION_CASE.build()
    # the two input sets really differ in structure, and the capacity cuts one of them
    na, nb = (oracle([t.cpu() for t in s], CAP_SHAPE["corpus_len"]) for s in (built.A, built.B))
    sa, sb = _sizes(na[0]), _sizes(nb[0])
    assert sa != sb and sa[0] == 0 and sb[0] > 0 and sb[2] == 0 and sa[2] > 0
    assert min(len(na[1]), len(nb[1])) < CAPACITY < max(len(na[1]), len(nb[1])), (len(na[1]), len(nb[1]))
    CAP.helper(UNION_CASE)
    assert set(SYMBOLS) == CAP.REPLAYED[UNION_CASE.name]  # the symbols the row declares are the ones the recorder saw
    # and the row computes the oracle's answer for B, cut at the capacity, the entries behind the lists untouched
    CAP._fill(built.outs, CC.SENTINEL)
    built.fn(built.B)
    torch.cuda.synchronize()
    cand_off, totals, cand_doc = built.outs
    assert cand_off.tolist() == nb[0] and totals.tolist() == [len(nb[1]), max(sb)]
    keep = min(len(nb[1]), CAPACITY)
    assert cand_doc[:keep].tolist() == nb[1][:keep] and bool((cand_doc[keep:].view(torch.uint8) == CC.SENTINEL).all())
