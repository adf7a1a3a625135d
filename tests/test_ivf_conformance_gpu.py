"""IVF scoring conformance on the MI355X: ivf_score_kernel (csrc/ivf.h) and ivf_pq_score_kernel (csrc/ivf_pq.h) against the fp64
oracle (tests/_ivf_oracle.py) on the case table of tests/_ivf_cases.py, whose CPU half (tests/test_ivf_conformance.py) shows that the
table tells a faithful plan from nine defective ones.

Grid cases have NO tolerance: the inputs are chosen so that fp32 accumulation is exact in any order (asserted by the table's
loader), so every word of the window `S [nq, ld]` is compared as an int32 -- a cell the oracle gives a contribution must hold
prefill + oracle, every other word (cells without a contribution, the ld - cols padding) its prefilled bit pattern, -0.0 and NaN
payloads included ("a zero contribution is skipped, never added"), and the 4096-byte bands around S must come back intact.  The
PQ kernel is held to the oracle over `decode()` first and to the dense kernel second.  Gaussian inputs are held to the bound of
tests/test_ivf_gpu.py's docstring, (max(dp, dc) + m + 1) * 2^-23 * A, and to nothing new."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ivf_cases as C  # noqa: E402
import _ivf_oracle as O  # noqa: E402
import _topk_oracle as TO  # noqa: E402
from _ivf_standin import unpack_index  # noqa: E402
from dpr_scale_amd import ivf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def kn():
    from dpr_scale_amd.hotpath import HipKernels

    assert torch.cuda.is_available(), "needs a HIP device"
    return HipKernels()


def _dense(case, kn, cls_doc=None, chunk=None):
    ex, docs, rows = C.flat(case)
    cd = None if cls_doc is None else torch.from_numpy(cls_doc)
    return ivf.IVFIndex(torch.from_numpy(ex), torch.from_numpy(docs), torch.from_numpy(rows), cd, case.corpus_len, DEV, chunk=chunk, kernels=kn)


def _pq(name, kn, cls_rows=None):
    dsub, codebook, codes, post_doc, off = C.pq_form(name)
    case = C.load(name).case
    dev = lambda x: torch.from_numpy(x).to(DEV)
    return ivf.IVFPQIndex.from_packed(dev(post_doc), dev(codes), torch.from_numpy(codebook).to(BF16).to(DEV), dev(off), cls_rows, case.corpus_len,
                                      case.d, kernels=kn)


def _run(score, pre):
    """`score(S)` on S [nq, ld] fp32 holding the words `pre`, between two guard bands: the words afterwards."""
    nq, ld = pre.shape
    raw = torch.full((2 * GUARD + nq * ld * 4,), PATTERN, dtype=torch.uint8, device=DEV)
    S = raw[GUARD:GUARD + nq * ld * 4].view(torch.int32).view(nq, ld)
    S.copy_(torch.from_numpy(pre.view(np.int32)))
    score(S.view(torch.float32))
    torch.cuda.synchronize()
    assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[GUARD + nq * ld * 4:] == PATTERN).all()), "guard band overwritten"
    return S.cpu().numpy().view(np.uint32)


def _check(got, want, contributed, note):
    bad = np.argwhere((got != want) & contributed)
    assert not len(bad), (note, "contributed cells differ", bad[:5].tolist(), [hex(x) for x in (got[tuple(bad[0])], want[tuple(bad[0])])])
    bad = np.argwhere((got != want) & ~contributed)
    assert not len(bad), (note, "words without a contribution changed", bad[:5].tolist())


@pytest.mark.parametrize("name", C.NAMES)
def test_dense_kernel_equals_the_oracle_bit_for_bit(kn, name):
    L = C.load(name)
    case = L.case
    index = _dense(case, kn)
    qb = ivf.pack_queries([], case.queries, None, d=case.d).to(DEV)
    assert index.dp == (case.d + 31) // 32 * 32 == qb.ent_vec.shape[1]
    pre, want, contributed = C.window(L)
    got = _run(lambda S: kn.ivf_score(index, qb, case.doc_begin, case.cols, S), pre)
    _check(got, want, contributed, case.note)


@pytest.mark.parametrize("name", C.PQ_NAMES)
def test_pq_kernel_equals_the_oracle_over_the_decoded_rows(kn, name):
    L = C.load(name)
    case = L.case
    pq = _pq(name, kn)
    dense = pq.decode()
    host = types.SimpleNamespace(post_doc=dense.post_doc.cpu(), post_vec=dense.post_vec.cpu(), exp_off=dense.exp_off.cpu(), n_experts=dense.n_experts)
    S = O.score_matrix(unpack_index(host), case.queries, case.corpus_len, bf16=True)  # the oracle over decode()
    assert C.check_exact(S, allow_inf=name.startswith("F-")) and np.array_equal(S, L.S)
    qb = ivf.pack_queries([], case.queries, None, d=case.d).to(DEV)
    pre, want, contributed = C.window(L, S)
    got = _run(lambda W: kn.ivf_pq_score(pq, qb, case.doc_begin, case.cols, W), pre)
    _check(got, want, contributed, case.note)
    # and only then: the dense kernel over the decoded rows
    assert np.array_equal(got, _run(lambda W: kn.ivf_score(dense, qb, case.doc_begin, case.cols, W), pre))


# ---- search: case G with its CLS part, and a ninth query whose CLS vector is NaN -----------------------------------------------------
@pytest.fixture(scope="module")
def g_search():
    L = C.load("G-zipf")
    cq, cd = C.cls_of("G-zipf")
    cq = np.concatenate([cq, np.full((1, cq.shape[1]), np.nan, dtype=np.float32)])
    queries = list(L.case.queries) + [L.case.queries[0]]
    S = O.score_matrix(L.case.postings, queries, L.case.corpus_len, cq, cd, bf16=True)
    assert C.check_exact(S[:-1]) and np.isnan(S[-1]).all()
    return L.case, queries, cq, cd, S


@pytest.mark.parametrize("chunk", [136, 2008])
@pytest.mark.parametrize("k", [1, 100])
@pytest.mark.parametrize("engine", ["dense", "pq"])
def test_search_equals_the_oracle_topk_bit_for_bit(kn, g_search, engine, k, chunk):
    case, queries, cq, cd, S = g_search
    index = _dense(case, kn, cls_doc=cd)
    if engine == "pq":
        index = _pq("G-zipf", kn, cls_rows=index.cls)
    v, i = index.search(torch.from_numpy(cq), queries, None, k, chunk=chunk)
    v, i = v.cpu().numpy(), i.cpu().numpy()
    want_v, want_i = O.topk(S[:-1], k)  # score descending, ties (the grid gives many) by lower doc id
    assert np.array_equal(i[:-1], want_i) and np.array_equal(v[:-1].view(np.uint32), want_v.astype(np.float32).view(np.uint32))
    # the NaN row by the fold's documented rule: a NaN is never selected, the unfilled tail is -inf / -1 -- and the rule as a whole
    assert (i[-1] == -1).all() and np.isneginf(v[-1]).all()
    ref_v, ref_i = TO.fold(None, S.astype(np.float32), 0, k)
    assert np.array_equal(i, ref_i) and np.array_equal(v.view(np.uint32), ref_v.view(np.uint32))


# ---- Gaussian values: the existing derived bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("shape", ["G", "A129"])
def test_gaussian_within_the_existing_derived_bound(kn, shape, d):
    case = C.shape_g("gauss", d=d, seed=21, name=f"gauss-{d}") if shape == "G" else C.shape_a(129, "gauss", d=d, seed=31)
    index = _dense(case, kn)
    nq = len(case.queries)
    S, A, m = O.score_matrix(case.postings, case.queries, case.corpus_len, bf16=True, return_abs=True)
    bound = (index.dp + m + 1) * 2.0 ** -23 * A
    Sg = torch.zeros((nq, case.ld), device=DEV)
    kn.ivf_score(index, ivf.pack_queries([], case.queries, None).to(DEV), 0, case.cols, Sg)
    got = Sg.cpu().numpy().astype(np.float64)
    err = np.abs(got[:, : case.cols] - S)
    worst = float((err / np.maximum(bound, 1e-300))[bound > 0].max())
    print(f"[ivf-gauss] shape {shape} d={d} matrix: worst error / bound = {worst:.4f}")
    assert (err <= bound).all() and not got[:, case.cols:].any() and not got[:, : case.cols][bound == 0].any()
    if shape == "G":  # and through the search, with the CLS part: max(dp, dc) + m + 1
        cq, cd = C._CLS[f"gauss-{d}"]
        S, A, m = O.score_matrix(case.postings, case.queries, case.corpus_len, cq, cd, bf16=True, return_abs=True)
        index = _dense(case, kn, cls_doc=cd)
        bound = (max(index.dp, index.dc) + m + 1) * 2.0 ** -23 * A
        v, i = index.search(torch.from_numpy(cq), case.queries, None, 100)
        v, i = v.cpu().numpy().astype(np.float64), i.cpu().numpy()
        worst = 0.0
        for n in range(nq):
            assert len(set(i[n].tolist())) == 100 and i[n].min() >= 0 and i[n].max() < case.corpus_len and (np.diff(v[n]) <= 0).all()
            err = np.abs(v[n] - S[n, i[n]])
            worst = max(worst, float((err / bound[n, i[n]]).max()))
            assert (err <= bound[n, i[n]]).all(), (n, float(err.max()))
            rest = np.setdiff1d(np.arange(case.corpus_len), i[n])
            assert (S[n, rest] <= v[n, -1] + bound[n, rest] + bound[n, i[n][-1]]).all()
        print(f"[ivf-gauss] shape {shape} d={d} search with CLS (dc={index.dc}): worst error / bound = {worst:.4f}")
