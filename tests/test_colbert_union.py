"""The candidate stage of the pruned ColBERT search on kernels, without a GPU: the ABI of
include/dprhot_union.h -- exported, bound in a table of its own, validated on the host -- and the routing of
`_CentroidPruning._union` between the kernels and `_union_torch`, on CPU stand-ins."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _colbert_cand_standin as CS  # noqa: E402
import _colbert_oracle as CO  # noqa: E402
import _colbert_union_standin as US  # noqa: E402
from dpr_scale_amd import _lib, colbert  # noqa: E402

HEADER = os.path.join(ROOT, "include", "dprhot_union.h")
REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
NQ, LQ, N, LD, D, C = 5, 6, 30, 40, 20, 16
_ONE = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dprhot_[a-z0-9_]+)\s*\(", src)))


def test_every_prototype_is_exported_and_bound_in_a_table_of_its_own():
    syms = declared_symbols()
    assert syms == ["dprhot_colbert_union_count", "dprhot_colbert_union_fill", "dprhot_colbert_union_workspace_bytes"]
    assert sorted(_lib.UNION_SIGNATURES) == syms
    for s in syms:
        fn = getattr(_lib.lib, s)  # exported
        assert s not in _lib.SIGNATURES
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.UNION_SIGNATURES[s][1]
    assert _lib.version() == 174
    # the prototypes and the table agree in their number of arguments
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in syms:
        args = re.search(rf"\b{s}\s*\(([^)]*)\)", src).group(1)
        assert len(args.split(",")) == len(_lib.UNION_SIGNATURES[s][1]), s


def test_limits_are_refused_on_the_host():
    lib = _lib.lib
    out = ctypes.c_size_t(0)
    wsb = lib.dprhot_colbert_union_workspace_bytes
    for bad, word in (((0, 100), b"nq="), ((65536, 100), b"nq="), ((2, 0), b"corpus_len"), ((2, 2 ** 31), b"corpus_len")):
        assert wsb(*bad, ctypes.byref(out)) == -1 and word in lib.dprhot_last_error(), bad
    assert wsb(2, 100, None) == -1 and b"NULL" in lib.dprhot_last_error()

    good = dict(cids=_ONE, q=_ONE, dp=32, nq=2, LQ=5, nprobe=2, C=8, off=_ONE, doc=_ONE, nl=50, n=100, co=_ONE, tot=_ONE, ws=_ONE, wsb=1 << 20,
                st=None)
    count = lambda **bad: lib.dprhot_colbert_union_count(*{**good, **bad}.values())
    for bad, word in ((dict(nq=0), b"nq="), (dict(nq=65536), b"nq="), (dict(LQ=0), b"LQ="), (dict(LQ=513), b"LQ="), (dict(nprobe=0), b"nprobe"),
                      (dict(C=0), b"C="), (dict(n=0), b"corpus_len"), (dict(n=2 ** 31), b"corpus_len"), (dict(nl=-1), b"n_list"),
                      (dict(nl=2 ** 40), b"n_list"), (dict(dp=0), b"dp="), (dict(dp=40), b"dp="), (dict(cids=None), b"NULL"),
                      (dict(q=None), b"NULL"), (dict(off=None), b"NULL"), (dict(doc=None), b"NULL"), (dict(co=None), b"NULL"),
                      (dict(tot=None), b"NULL"), (dict(ws=ctypes.c_void_p(260)), b"aligned")):
        assert count(**bad) == -1 and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())
    assert _lib.colbert_union_workspace_bytes(2, 100) <= 1 << 20
    for bad in (dict(ws=None), dict(wsb=_lib.colbert_union_workspace_bytes(2, 100) - 1)):
        assert count(**bad) == -4, bad
        err = lib.dprhot_last_error()
        assert b"colbert_union_count needs" in err and b"dprhot_colbert_union_workspace_bytes" in err, err
    assert count(nq=65535, LQ=512, nprobe=300, wsb=1 << 40) == -3 and b"too many" in lib.dprhot_last_error()

    good = dict(nq=2, n=100, co=_ONE, doc=_ONE, nc=10, ws=_ONE, wsb=1 << 20, st=None)
    fill = lambda **bad: lib.dprhot_colbert_union_fill(*{**good, **bad}.values())
    for bad, word in ((dict(nq=0), b"nq="), (dict(nq=65536), b"nq="), (dict(n=0), b"corpus_len"), (dict(n=2 ** 31), b"corpus_len"),
                      (dict(nc=-1), b"n_cand"), (dict(nc=2 ** 40), b"n_cand"), (dict(co=None), b"NULL"), (dict(doc=None), b"NULL"),
                      (dict(ws=ctypes.c_void_p(264)), b"aligned")):
        assert fill(**bad) == -1 and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())
    for bad in (dict(ws=None), dict(wsb=16)):
        assert fill(**bad) == -4, bad
        err = lib.dprhot_last_error()
        assert b"colbert_union_fill needs" in err and b"dprhot_colbert_union_workspace_bytes" in err, err
    assert fill(nc=0, doc=None) == 0  # a capacity of nothing: validated, nothing launched


def test_the_workspace_grows_with_both_sizes():
    f = _lib.colbert_union_workspace_bytes
    assert f(1, 1) >= 4 and f(1, 1) % 16 == 0
    sizes = (1, 31, 32, 33, 8191, 8192, 8193, 16385, 10 ** 6, 2 ** 31 - 1)
    for nq in (1, 2, 33, 65535):
        row = [f(nq, n) for n in sizes]
        assert row == sorted(row) and all(b >= nq * ((n + 7) // 8) for b, n in zip(row, sizes))
    for n in sizes:
        col = [f(nq, n) for nq in (1, 2, 3, 33, 1024, 65535)]
        assert col == sorted(col) and len(set(col)) == len(col)
    assert f(5, 10 ** 6) <= 5 * f(1, 10 ** 6)  # what _union_batches relies on


def grid_index(kernels, seed=3):
    lengths = np.random.default_rng(seed).permutation(np.resize(np.array([0, 1, 5, 15, 16, 17, 31, 33, 39]), N))
    q, c, att = CO.make_padded(seed, NQ, LQ, N, LD, D, lengths=lengths, q_pad=2)
    index = colbert.ColBERTIndex.from_repr(c, att, list(range(N)), N, "cpu", kernels=kernels)
    cen = torch.from_numpy(np.random.default_rng(seed + 1).integers(-4, 5, size=(C, D)).astype(np.float32) / 4.0)
    index.build_centroids(C, centroids=cen)
    return index, q


class Spy(US.ColbertUnionKernels):
    def __init__(self):
        super().__init__()
        self.calls = []

    def colbert_union_workspace(self, nq, corpus_len, like):
        self.calls.append(("workspace", nq))
        return super().colbert_union_workspace(nq, corpus_len, like)

    def colbert_union_count(self, index, cids, qb, cand_off, totals, ws):
        self.calls.append(("count", int(qb.shape[0])))
        return super().colbert_union_count(index, cids, qb, cand_off, totals, ws)

    def colbert_union_fill(self, index, cand_off, cand_doc, ws):
        self.calls.append(("fill", int(cand_off.shape[0]) - 1))
        return super().colbert_union_fill(index, cand_off, cand_doc, ws)


def _expected(index, q, nprobe):
    return CS.union_of_lists(index.probe(q, nprobe), (q != 0).any(2), index.cen_off.tolist(), index.cen_doc.tolist())


@pytest.mark.parametrize("nprobe", [1, 2, C])
def test_candidates_run_the_union_methods_and_equal_the_union_of_lists(nprobe):
    kn = Spy()
    index, q = grid_index(kn)
    cand_off, cand_doc = index.candidates(q, nprobe)
    assert kn.calls == [("workspace", NQ), ("count", NQ), ("fill", NQ)]
    assert cand_off.dtype == torch.int64 and cand_off.shape == (NQ + 1,) and cand_doc.dtype == torch.int32
    off, docs = _expected(index, q, nprobe)
    assert cand_off.tolist() == off and cand_doc.tolist() == docs and len(docs) > 0
    # all four return values are those of the definition
    qb = index._queries(q)
    got, want = index._union(qb, index.probe(q, nprobe)), index._union_torch(qb, index.probe(q, nprobe))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:] == want[2:]
    assert all(type(v) is int for v in got[2:])


def test_five_queries_in_three_batches(monkeypatch):
    kn = Spy()
    index, q = grid_index(kn)
    monkeypatch.setattr(colbert, "UNION_WS_BYTES", 2 * _lib.colbert_union_workspace_bytes(1, N))
    assert index._union_batches(NQ) == [(0, 2), (2, 4), (4, 5)]
    qb, cids = index._queries(q), index.probe(q, 2)
    got = index._union(qb, cids)
    assert [c for c in kn.calls if c[0] == "count"] == [("count", 2), ("count", 2), ("count", 1)]
    assert [c for c in kn.calls if c[0] == "fill"] == [("fill", 2), ("fill", 2), ("fill", 1)]
    want = index._union_torch(qb, cids)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:] == want[2:]
    off, docs = _expected(index, q, 2)
    assert got[0].tolist() == off and got[1].tolist() == docs
    # a bound below one query's state still lets every query through, one at a time
    monkeypatch.setattr(colbert, "UNION_WS_BYTES", 1)
    assert index._union_batches(NQ) == [(n, n + 1) for n in range(NQ)]
    v, i = index.search_pruned(q, 4, 2)
    monkeypatch.undo()
    v1, i1 = index.search_pruned(q, 4, 2)
    assert torch.equal(v, v1) and torch.equal(i, i1)


def test_a_kernel_set_without_the_union_methods_keeps_the_torch_route(monkeypatch):
    index, q = grid_index(CS.ColbertCandKernels())
    assert not hasattr(index._kernels(), "colbert_union_count")
    seen = []
    torch_route = colbert._CentroidPruning._union_torch
    monkeypatch.setattr(colbert._CentroidPruning, "_union_torch", lambda self, qb, cids: seen.append(1) or torch_route(self, qb, cids))
    new, _ = grid_index(US.ColbertUnionKernels())
    for nprobe in (1, 3):
        cand_off, cand_doc = index.candidates(q, nprobe)
        assert len(seen) == 1
        seen.clear()
        off, docs = _expected(index, q, nprobe)
        assert cand_off.tolist() == off and cand_doc.tolist() == docs
        a, b = new.candidates(q, nprobe)
        assert not seen and torch.equal(a, cand_off) and torch.equal(b, cand_doc)


def test_the_standin_reads_hostile_inputs_as_the_header_says():
    """ids outside [0, C), a NaN and a -0.0 token, offsets that run backwards or past the end, doc ids outside the corpus, and the
    capacity rule -- by hand."""
    kn = US.ColbertUnionKernels()
    idx = type("I", (), {})()
    idx.cen_off = torch.tensor([0, 3, 2, 9, 4], dtype=torch.int64)       # lists: [0, 3), [3, 2) -> empty, [2, 6) clamped, [6, 4) -> empty
    idx.cen_doc = torch.tensor([5, -1, 7, 1, 9, 2], dtype=torch.int32)   # corpus of 8: -1 and 9 are skipped
    idx.corpus_len = 8
    qb = torch.ones(3, 2, 32, dtype=torch.bfloat16)
    qb[0, 1] = -0.0
    qb[1, 0] = float("nan")
    qb[2] = 0
    cids = torch.tensor([[[0], [2]], [[2], [-1]], [[0], [2]]])
    cids[1, 1, 0] = 7
    cand_off, totals, ws = torch.empty(4, dtype=torch.int64), torch.empty(2, dtype=torch.int64), kn.colbert_union_workspace(3, 8, qb)
    kn.colbert_union_count(idx, cids, qb, cand_off, totals, ws)
    assert cand_off.tolist() == [0, 2, 5, 5] and totals.tolist() == [5, 3]
    full = torch.full((7,), -9, dtype=torch.int32)
    kn.colbert_union_fill(idx, cand_off, full, ws)
    assert full.tolist() == [5, 7, 1, 2, 7, -9, -9]
    short = torch.full((3,), -9, dtype=torch.int32)
    kn.colbert_union_fill(idx, cand_off, short, ws)
    assert short.tolist() == [5, 7, 1]


def test_union_kernels_never_spill():
    text = open(REPORT).read()
    blocks = re.findall(r"Function Name: (\S*un_(?:clear|mark|count|offsets|fill)_kernel\S*).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", text, flags=re.S)
    assert len({b[0] for b in blocks}) == 5, sorted({b[0] for b in blocks})
    for name, s, v in blocks:
        assert (int(s), int(v)) == (0, 0), name
