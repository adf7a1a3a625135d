"""The inverted-index conformance table on the CPU (tests/_ivf_cases.py; the GPU half is tests/test_ivf_conformance_gpu.py).

  1. The fp64 oracle (tests/_ivf_oracle.py) is pinned against a triple Python loop over (query, entry, posting), also on the rule for
     NaN and +-inf products ("Limits").
  2. The table is shown to discriminate.  `emulate` restates the PLAN of ivf_score_kernel (csrc/ivf.h) in numpy on the PACKED layout
     -- pd, eoff, bexp, boff, eq; 128-doc ranges; trips of 64 batch experts; groups of 16 entries; slices of 64 postings; the
     per-group table and its flush by the first posting of a doc's run -- in fp64 arithmetic, with a `defect=` switch.  The faithful
     emulator must equal the oracle on every case, every word of the window and around it; every defect of DEFECTS must fail at
     least one case, and the test prints which (as test_injected_bug_is_far_outside_the_bounds does for the training step)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ivf_cases as C  # noqa: E402
import _ivf_oracle as O  # noqa: E402
from _ivf_standin import IvfKernels  # noqa: E402
from dpr_scale_amd import ivf  # noqa: E402

DEFECTS = {
    "experts_first_64": "only the first 64 batch experts",
    "entries_first_16": "only the first 16 entries of an expert",
    "postings_first_64": "only the first 64 postings of an (expert, range) pair",
    "flush_per_slice": "run ownership restarted at every multiple of 64: an entry is added once per slice its run touches",
    "k_step_0_only": "only K step 0",
    "sum_over_run": "sum instead of max over a doc's run",
    "range_end_inclusive": "the range's end taken inclusively",
    "range_begin_exclusive": "the range's begin taken exclusively",
    "nan_propagates": "a NaN product poisons its doc's run, a non-finite maximum adds 0 (the oracle's rule before this suite)",
}
SLACK = 256  # words around the emulated window: a store outside it must show, not fault


def emulate(pd, pv, eoff, ev, eq, bexp, boff, nq, D0, cols, ld, defect=None):
    """The words of S [nq, ld] (between SLACK words on either side, all starting from 0) after ivf_score_kernel's plan; fp64."""
    assert defect is None or defect in DEFECTS
    pd, eoff, eq, bexp, boff = (np.asarray(x, dtype=np.int64) for x in (pd, eoff, eq, bexp, boff))
    pv, ev = np.asarray(pv, dtype=np.float64), np.asarray(ev, dtype=np.float64)
    V, nb, dp = len(eoff) - 1, len(bexp), pv.shape[1]
    kdim = 32 if defect == "k_step_0_only" else dp
    old = defect == "nan_propagates"
    empty = -np.inf if old else 0.0
    buf = np.zeros(SLACK + nq * ld + SLACK)
    for t0 in range(0, cols, C.T):  # one wave
        d0, d1 = D0 + t0, D0 + min(t0 + C.T, cols)
        M = np.full((C.ROWS, C.T), empty)
        for b0 in range(0, nb, 64):
            if defect == "experts_first_64" and b0:
                break
            for l in range(min(64, nb - b0)):  # (the live lanes in ascending order)
                x = bexp[b0 + l]
                if not 0 <= x < V:
                    continue
                seg = pd[eoff[x]:eoff[x + 1]]
                s = eoff[x] + np.searchsorted(seg, d0, "right" if defect == "range_begin_exclusive" else "left")
                e = eoff[x] + np.searchsorted(seg, d1, "right" if defect == "range_end_inclusive" else "left")
                pc = int(e - s)
                if pc <= 0:
                    continue
                docs = pd[s:e]
                dl = docs - d0
                inside = (dl >= 0) & (dl < C.T)  # the kernel's `(unsigned)dl >= IVF_T` guard
                e0, e1 = boff[b0 + l], boff[b0 + l + 1]
                for eg in range(e0, e1, C.ROWS):
                    if defect == "entries_first_16" and eg > e0:
                        break
                    ne = min(C.ROWS, e1 - eg)
                    with np.errstate(invalid="ignore"):
                        prod = ev[eg:eg + ne, :kdim] @ pv[s:e, :kdim].T  # [ne, pc]

                    def fold(c0, c1):
                        cs = np.arange(c0, c1)[inside[c0:c1]]
                        r, c = np.meshgrid(np.arange(ne), cs, indexing="ij")
                        v = prod[r, c]
                        keep = np.ones_like(v, dtype=bool) if old else v > 0
                        (np.add if defect == "sum_over_run" else np.maximum).at(M, (r[keep], dl[c][keep]), v[keep])

                    def flush(c0, c1, restart):
                        cs = np.arange(c0, c1)
                        owner = np.array([c == restart or docs[c - 1] != docs[c] for c in cs], dtype=bool) & inside[c0:c1]
                        cs = cs[owner]
                        for r in range(ne):
                            got = M[r, dl[cs]]
                            M[r, dl[cs]] = empty
                            if old:
                                got = np.where(np.isfinite(got) & (got > 0), got, 0.0)
                            q = eq[eg + r]
                            if not 0 <= q < nq:
                                continue
                            nz = got != 0  # a zero contribution is skipped, never added
                            np.add.at(buf, SLACK + q * ld + (docs[cs] - D0)[nz], got[nz])

                    last = min(pc, C.SLICE) if defect == "postings_first_64" else pc
                    if defect == "flush_per_slice":
                        for c0 in range(0, pc, C.SLICE):
                            fold(c0, min(c0 + C.SLICE, pc))
                            flush(c0, min(c0 + C.SLICE, pc), c0)
                    else:
                        for c0 in range(0, last, C.SLICE):
                            fold(c0, min(c0 + C.SLICE, last))
                        flush(0, pc, 0)
    return buf


def _packed(case):
    """The device layout through the project's own packers, on the CPU."""
    ex, docs, rows = C.flat(case)
    index = ivf.IVFIndex(torch.from_numpy(ex), torch.from_numpy(docs), torch.from_numpy(rows), None, case.corpus_len, "cpu", kernels=IvfKernels())
    qb = ivf.pack_queries([], case.queries, None, d=case.d)
    return index, qb


def _emulated(L, defect=None):
    index, qb = _packed(L.case)
    case = L.case
    return emulate(index.post_doc.numpy(), index.post_vec.float().numpy(), index.exp_off.numpy(), qb.ent_vec.float().numpy(), qb.ent_q.numpy(),
                   qb.bexp.numpy(), qb.boff.numpy(), qb.nq, case.doc_begin, case.cols, case.ld, defect)


def _expected(L):
    case = L.case
    nq = len(case.queries)
    want = np.zeros(SLACK + nq * case.ld + SLACK)
    win = want[SLACK:SLACK + nq * case.ld].reshape(nq, case.ld)
    win[:, : case.cols] = L.S[:, case.doc_begin:case.doc_begin + case.cols]
    return want


# ---- 1. the oracle ---------------------------------------------------------------------------------------------------------------------
def _triple_loop(postings, queries, corpus_len):
    """score and m by the definition, one product at a time, in Python floats (fp64)."""
    S = [[0.0] * corpus_len for _ in queries]
    m = [[0] * corpus_len for _ in queries]
    for n, by_expert in enumerate(queries):
        for e, vecs in by_expert.items():
            if e not in postings:
                continue
            ids, rows = postings[e]
            for u in vecs:
                best = {}
                for doc, v in zip(ids, rows):
                    p = 0.0
                    for a, b in zip(u.tolist(), v.tolist()):
                        p += a * b
                    best[int(doc)] = max(best.get(int(doc), 0.0), p if p > 0 else 0.0)  # (neither operand is ever a NaN)
                for doc, c in best.items():
                    S[n][doc] += c
                    m[n][doc] += 1
    return np.array(S), np.array(m)


def _tiny(which):
    if which == "non_finite":  # one expert, a query of 32 ones
        ones = np.ones(32, dtype=np.float32)
        first = lambda x: np.concatenate([[x], ones[1:]]).astype(np.float32)
        rows = np.stack([ones * np.nan, 3 * ones, first(np.inf), first(-np.inf), first(-np.inf), 0.5 * ones, -ones, ones * np.nan])
        return {0: (np.array([1, 1, 3, 4, 5, 5, 6, 7]), rows)}, [{0: [torch.ones(32)]}], 9
    g = np.random.default_rng(3 if which == "grid" else 4)
    val = (lambda *s: (g.integers(-8, 9, size=s) / 4.0).astype(np.float32)) if which == "grid" else (lambda *s: g.standard_normal(s).astype(np.float32))
    post = {e: (np.sort(g.integers(0, 7, size=n)), val(n, 4)) for e, n in ((0, 6), (2, 3), (5, 1))}
    queries = [{0: [torch.from_numpy(val(4)), torch.from_numpy(val(4))], 5: [torch.from_numpy(val(4))]}, {},
               {2: [torch.from_numpy(val(4))], 9: [torch.from_numpy(val(4))]}]
    return post, queries, 7


@pytest.mark.parametrize("which", ["grid", "gauss", "non_finite"])
def test_oracle_equals_the_triple_loop(which):
    post, queries, ndocs = _tiny(which)
    S, _, m = O.score_matrix(post, queries, ndocs, return_abs=True)
    S2, m2 = _triple_loop(post, queries, ndocs)
    assert np.array_equal(m, m2)
    if which == "gauss":  # (numpy's dot product may add in another order than the loop: a few fp64 ulps)
        assert np.allclose(S, S2, rtol=1e-13, atol=0)
    else:
        assert np.array_equal(S, S2)
    if which == "non_finite":
        # doc 1 {NaN row, 3 ones}: the NaN is absent, 96 is added.  doc 3 +inf.  doc 4 -inf alone: 0.  doc 5 {-inf, 0.5 ones}: 16.
        # doc 6 negative: 0.  doc 7 NaN alone: 0.  All six HAVE a posting.
        assert S[0].tolist() == [0, 96, 0, np.inf, 0, 16, 0, 0, 0] and m[0].tolist() == [0, 1, 0, 1, 1, 1, 1, 1, 0]
    print(f"oracle == triple loop on {which}: {S.shape[0]} x {S.shape[1]} cells")


# ---- 2. the table ----------------------------------------------------------------------------------------------------------------------
def test_the_table_holds_the_shapes_it_names():
    fam = lambda f: [n for n in C.NAMES if n.startswith(f)]
    assert [len(fam(f)) for f in "ABCDEFG"] == [5, 5, 6, 20, 12, 6, 1] and len(C.NAMES) == 55 and len(C.PQ_NAMES) == 29
    # A: the batch's distinct experts; B: entries of the one expert; C: postings of expert 7 inside docs 128 .. 255 and its runs
    for nb in C.A_NB:
        case = C.load(f"A-nb{nb}").case
        experts = sorted(set().union(*case.queries))
        assert len(experts) == nb and (nb < 63 or {2, 3}.issubset(experts)) and (nb in (1, 65) or experts[-1] == 1000)
        if nb >= 65:
            assert experts[64] == 64 and [e for e, (ids, _) in case.postings.items() if 299 in ids] == [64]
            assert C.load(f"A-nb{nb}").S[1, 299] > 0 and C.load(f"A-nb{nb}").m[1, 299] == 1
    for ne in C.B_COUNTS:
        _, qb = _packed(C.load(f"B-ne{ne}").case)
        assert qb.n_entries == ne and qb.bexp.tolist() == [3]
        if ne >= 17:
            assert qb.ent_q[15] == qb.ent_q[16] and qb.ent_q[14] == qb.ent_q[15]
    for pc, runs in C.C_RUNS.items():
        ids = C.load(f"C-pc{pc}").case.postings[7][0]
        inside = ids[(ids >= 128) & (ids < 256)]
        assert len(inside) == pc and [int((inside == d).sum()) for d in np.unique(inside)] == runs
    S = C.load("C-pc200").S  # the winners: 1.5 * 2, 1 * 2, 2 * 2 on every run but the last, whose cells get nothing from e0, e1, e2
    docs = np.unique(C.load("C-pc200").case.postings[7][0])
    docs = docs[(docs >= 128) & (docs < 256)]
    assert S[0, docs].tolist() == [3, 3, 3, 0] and S[2, docs].tolist() == [4, 4, 4, 0]
    for name in fam("D"):
        case = C.load(name).case
        ids = case.postings[4][0]
        for x in (case.doc_begin - 1, case.doc_begin, case.doc_begin + case.cols - 1, case.doc_begin + case.cols):
            assert x < 0 or x in ids
        assert case.ld % 8 == 0 and case.ld - case.cols in (range(24, 32) if name.endswith("wide") else range(0, 8))
    assert [(C.load(f"E-d{d}").case.d + 31) // 32 * 32 for d in C.E_D] == [32, 32, 64, 64, 96, 128]
    assert np.isinf(C.load("F-pos_inf").S[0, 3]) and not C.load("F-neg_inf").S[0, 3] and C.load("F-inf_times_zero").S[0, 3] == 7.75
    assert C.load("F-nan_beside_positive").S[0, 1] == 64 and not C.load("F-nan_alone").S[:, 1].any() and C.load("F-nan_alone").m[0, 1] == 1
    L = C.load("G-zipf")
    cq, cd = C.cls_of("G-zipf")
    assert L.S.shape == (8, 2003) and cq.shape == (8, 24) and cd.shape == (2003, 24) and C.check_exact(L.S + cq.astype(np.float64) @ cd.T)
    assert sum(len(v[0]) for v in L.case.postings.values()) < 16000


def test_the_prefill_has_both_kinds_of_cell_and_the_special_patterns():
    for name in ("A-nb129", "D-0+1-wide", "F-pos_inf", "G-zipf"):
        L = C.load(name)
        pre, want, contributed = C.window(L)
        assert pre.dtype == np.uint32 and pre.shape == (len(L.case.queries), L.case.ld) and contributed.any() and not contributed.all()
        assert np.array_equal(pre[~contributed], want[~contributed]) and not (pre[contributed] == want[contributed]).any()
        assert not contributed[:, L.case.cols:].any()
        if name == "G-zipf":
            assert set(C.PREFILL_BITS) <= set(pre[~contributed].tolist())
    pre, want, contributed = C.window(C.load("F-pos_inf"))
    assert want[0, 3] == 0x7F800000 and contributed[0, 3]


@pytest.mark.parametrize("name", C.PQ_NAMES)
def test_pq_form_holds_the_rows_exactly(name):
    dsub, codebook, codes, post_doc, off = C.pq_form(name)  # (asserts decode == rows, bit for bit as bf16)
    fin = codebook[np.isfinite(codebook)]
    assert codes.dtype == np.uint8 and codebook.shape == (codes.shape[1], 256, dsub) and np.array_equal(np.round(fin * 4), fin * 4)
    index, _ = _packed(C.load(name).case)
    assert np.array_equal(index.post_doc.numpy(), post_doc) and np.array_equal(index.exp_off.numpy(), off)
    dec = ivf.pq_decode(torch.from_numpy(codes), torch.from_numpy(codebook).to(torch.bfloat16))
    assert torch.equal(dec.view(torch.int16), index.post_vec.view(torch.int16))


# ---- 3. the emulator and its defects ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_faithful_emulator_equals_the_oracle(name):
    L = C.load(name)
    assert np.array_equal(_emulated(L), _expected(L)), L.case.note


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_defect_is_killed_by_the_table(defect):
    killers = [n for n in C.NAMES if not np.array_equal(_emulated(C.load(n), defect), _expected(C.load(n)), equal_nan=True)]
    print(f"[ivf-defect] {defect} ({DEFECTS[defect]}): killed by {len(killers)} of {len(C.NAMES)} cases: {' '.join(killers)}")
    assert killers, defect
