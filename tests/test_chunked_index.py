"""What IVFIndex and ColBERTIndex take from their common base (dpr_scale_amd/_chunked.py), on the CPU stand-ins: the chunk size and the
walk over disjoint doc-id ranges that starts the top-k state exactly once."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _colbert_oracle as CO  # noqa: E402
from _ivf_standin import IvfKernels  # noqa: E402
from dpr_scale_amd import colbert, ivf  # noqa: E402
from dpr_scale_amd._chunked import ChunkedIndex  # noqa: E402

_BF16 = torch.bfloat16


def _ivf_index(corpus_len, chunk, kernels):
    g = torch.Generator().manual_seed(3)
    P = 12
    docs = torch.randperm(min(corpus_len, 40), generator=g)[:min(corpus_len, P)]
    experts = torch.arange(docs.shape[0]) % 3
    vecs = torch.randint(-4, 5, (docs.shape[0], 8), generator=g).float() / 4.0
    return ivf.IVFIndex(experts, docs, vecs, None, corpus_len, "cpu", chunk=chunk, kernels=kernels)


def _colbert_index(corpus_len, chunk, kernels):
    g = torch.Generator().manual_seed(4)
    n = min(corpus_len, 9)
    ids = torch.randperm(min(corpus_len, 40), generator=g)[:n]
    lens = torch.arange(n) % 4 + 1
    rows = torch.randint(-4, 5, (int(lens.sum()), 8), generator=g).float() / 4.0
    return colbert.ColBERTIndex(ids, lens, rows, corpus_len, "cpu", chunk=chunk, kernels=kernels)


# the rule: min(8 MiB of fp32 scores per pass, at least 1024 ids, at most 262144) unless a chunk was given; never beyond the corpus
# rounded up to 8; a multiple of 8, at least 8
@pytest.mark.parametrize("nq,corpus_len,chunk,want", [(1, 5, None, 8), (4, 2003, None, 2008), (4096, 10 ** 6, None, 1024), (3, 2003, 100, 96),
                                                      (3, 2003, 8, 8)])
def test_default_chunk_is_one_rule(nq, corpus_len, chunk, want):
    a, b = _ivf_index(corpus_len, chunk, IvfKernels()), _colbert_index(corpus_len, chunk, CO.ColbertKernels())
    assert type(a).default_chunk is type(b).default_chunk is ChunkedIndex.default_chunk
    assert a.default_chunk(nq) == b.default_chunk(nq) == want


class _Recorder:
    """A kernel object that passes everything on and keeps the `first` flag of every *_search call."""

    def __init__(self, inner):
        self.inner, self.firsts = inner, []

    def __getattr__(self, name):
        f = getattr(self.inner, name)
        if not name.endswith("_search"):
            return f

        def search(*args):
            self.firsts.append(bool(args[-3]))  # (..., values, indices, first, chunk, ws)
            return f(*args)

        return search


def test_disjoint_ranges_start_the_state_once():
    ranges = [(0, 11), (11, 37)]
    kn = _Recorder(IvfKernels())
    index = _ivf_index(37, 16, kn)
    emb = [{0: [torch.ones(8)], 2: [torch.full((8,), 0.5)]}, {1: [torch.ones(8)]}]
    got = index.search([], emb, None, 5, id_ranges=ranges)
    assert kn.firsts == [True, False]
    want = index.search([], emb, None, 5)
    assert kn.firsts == [True, False, True]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert set(index.latency) == {"encode_time", "search_time"}

    kn = _Recorder(CO.ColbertKernels())
    index = _colbert_index(37, 16, kn)
    q = torch.randint(-4, 5, (2, 3, 8), generator=torch.Generator().manual_seed(5)).float() / 4.0
    got = index.search(q, 5, id_ranges=ranges)
    assert kn.firsts == [True, False]
    want = index.search(q, 5)
    assert kn.firsts == [True, False, True]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert set(index.latency) == {"encode_time", "search_time"}
    for index in (_ivf_index(37, None, IvfKernels()), _colbert_index(37, None, CO.ColbertKernels())):
        with pytest.raises(ValueError, match="topk=38"):
            index._fold(1, 38, None, None, None, None)
