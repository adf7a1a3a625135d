"""SPAR retrieval on the MI355X (csrc/spar.h through dprhot_spar_score / dprhot_spar_search).

Grid inputs (tests/_spar_oracle.py) must come out BIT-EQUAL to the float64 oracle.  Gaussian inputs (bf16-rounded operands) are held
against it under a per-cell bound derived from the arithmetic, not measured: a dot product of d exact bf16 products accumulated in fp32
in any order is off by at most d * 2^-23 * sum_k |q_k c_k|, the fma rounds once more (at most 2^-23 of a result that |acc1| + |lam|
|acc2| bounds), so  bound = 2^-23 * ((d1 + 1) * A1 + |lam| * (d2 + 1) * A2)  with A = |Q| |C|^T.
`search` is compared with the total-order top-k of the kernel's own `score` matrix with torch.equal: near-ties cannot make it flaky.
Outputs and an exactly sized workspace sit between 4 KiB guard bands.  Every input is valid; nothing here provokes a fault."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _spar_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5


def _banded(raws, nbytes):
    raw = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    raws.append((raw, nbytes))
    return raw[GUARD:GUARD + nbytes]


def _check_bands(raws):
    torch.cuda.synchronize()
    for raw, nb in raws:
        assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[GUARD + nb:] == PATTERN).all()), "guard band overwritten"


_p = lambda t: ctypes.c_void_p(t.data_ptr())
_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_bf16(x):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()
    assert torch.equal(t.float().cpu(), torch.from_numpy(np.asarray(x, dtype=np.float32))) or np.isnan(x).any(), "inputs must be bf16-exact"
    return t


def _lam(lams):
    return (ctypes.c_float * len(lams))(*lams), len(lams)


def bare_score(Q1, Q2, C1, C2, lams, doc_begin, cols, ld=None):
    """dprhot_spar_score through ctypes alone into S [W * nq, ld] between guard bands; the padding columns keep their fill pattern."""
    from dpr_scale_amd import _lib

    ld = (cols + 7) // 8 * 8 if ld is None else ld
    nq, (lam, W) = Q1.shape[0], _lam(lams)
    raws = []
    S = _banded(raws, W * nq * ld * 4).view(torch.float32).view(W * nq, ld)
    _lib.check(_lib.lib.dprhot_spar_score(_p(Q1), _p(Q2), nq, Q1.shape[1], Q2.shape[1], _p(C1), _p(C2), C1.shape[0], lam, W, doc_begin, cols,
                                          _p(S), ld, _stream()), "dprhot_spar_score")
    _check_bands(raws)
    assert bool((S[:, cols:].contiguous().view(torch.uint8) == PATTERN).all()), "padding columns written"
    return S[:, :cols].clone()


def bare_search(Q1, Q2, C1, C2, lams, k, chunk, id_ranges=None):
    """dprhot_spar_search through ctypes alone: values, indices and an exactly sized workspace sit between guard bands."""
    from dpr_scale_amd import _lib

    nq, n, (lam, W) = Q1.shape[0], C1.shape[0], _lam(lams)
    nb = ctypes.c_size_t(0)
    _lib.check(_lib.lib.dprhot_spar_workspace_bytes(nq, W, chunk, ctypes.byref(nb)))
    nws = nb.value
    if k > 4096:
        _lib.check(_lib.lib.dprhot_topk_wide_workspace_bytes(W * nq, k, ctypes.byref(nb)))
        nws += nb.value
    raws = []
    values = _banded(raws, W * nq * k * 4).view(torch.float32).view(W * nq, k)
    indices = _banded(raws, W * nq * k * 8).view(torch.int64).view(W * nq, k)
    ws = _banded(raws, nws)
    first = 1
    for b, e in (id_ranges or [(0, n)]):
        _lib.check(_lib.lib.dprhot_spar_search(_p(Q1), _p(Q2), nq, Q1.shape[1], Q2.shape[1], _p(C1), _p(C2), n, lam, W, b, e, k, chunk,
                                               _p(values), _p(indices), first, _p(ws), nws, _stream()), "dprhot_spar_search")
        first = 0
    _check_bands(raws)
    return values.clone(), indices.clone()


def want_topk(S, k):
    v, i = SO.topk(S.cpu().numpy(), k)
    return torch.from_numpy(v).to(DEV), torch.from_numpy(i).to(DEV)


# ---------------------------------------------------------------- score ----------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 19])
@pytest.mark.parametrize("d1,d2", [(32, 32), (96, 160), (256, 64)])
def test_score_grid_inputs_bit_equal_to_the_oracle(d1, d2, W):
    rng = np.random.default_rng(1000 * d1 + d2 + W)
    n, doc_begin = 1040, 37
    q1, q2, c1, c2 = SO.grid(rng, 130, d1), SO.grid(rng, 130, d2), SO.grid(rng, n, d1), SO.grid(rng, n, d2)
    lams = SO.grid_lams(W)
    want = SO.score(q1, q2, c1, c2, lams)  # [W, 130, n] float64, computed once per case
    C1, C2 = dev_bf16(c1), dev_bf16(c2)
    for nq in (1, 33, 130):
        Q1, Q2 = dev_bf16(q1[:nq]), dev_bf16(q2[:nq])
        for cols in (1, 7, 8, 129, 1000):
            ld = (cols + 7) // 8 * 8 + 8  # ld > cols
            S = bare_score(Q1, Q2, C1, C2, lams, doc_begin, cols, ld).cpu().numpy().reshape(W, nq, cols)
            assert np.array_equal(S.astype(np.float64), want[:, :nq, doc_begin:doc_begin + cols]), (nq, cols)


def test_score_gaussian_within_the_derived_bound():
    d1, d2, nq, cols, doc_begin = 768, 1024, 130, 520, 9
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float().numpy()
    q1, q2, c1, c2 = rnd(nq, d1), rnd(nq, d2), rnd(doc_begin + cols, d1), rnd(doc_begin + cols, d2)
    lams = [0.0, -1.5, 3.0]
    S = bare_score(dev_bf16(q1), dev_bf16(q2), dev_bf16(c1), dev_bf16(c2), lams, doc_begin, cols)
    S = S.cpu().numpy().reshape(3, nq, cols).astype(np.float64)
    err = np.abs(S - SO.score(q1, q2, c1[doc_begin:], c2[doc_begin:], lams))
    bound = SO.bound(q1, q2, c1[doc_begin:], c2[doc_begin:], lams)
    print(f"max err {err.max():.3e}, max err / bound {(err / bound).max():.4f}")
    assert bool((err <= bound).all())
    # two runs and another window: the same bits (a cell depends on its rows and its weight only)
    S2 = bare_score(dev_bf16(q1), dev_bf16(q2), dev_bf16(c1), dev_bf16(c2), lams, doc_begin + 100, 77)
    assert np.array_equal(S2.cpu().numpy().reshape(3, nq, 77).astype(np.float64), S[:, :, 100:177])


# ---------------------------------------------------------------- search ---------------------------------------------------------------
def _gauss_case(seed, nq, n, d1=64, d2=32):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float().numpy()
    return rnd(nq, d1), rnd(nq, d2), rnd(n, d1), rnd(n, d2)


def _lams(W):
    return [1.0] if W == 1 else [round(0.1 * (w + 1), 2) for w in range(W - 2)] + [0.0, -0.5]


_SEARCH = {}  # W -> (device operands, lams, the kernel's own score matrix): computed once, shared, never changed


def _search_case(W):
    if W not in _SEARCH:
        ops = [dev_bf16(x) for x in _gauss_case(11 + W, 5, 1000)]
        _SEARCH[W] = (ops, _lams(W), bare_score(*ops, _lams(W), 0, 1000))
    return _SEARCH[W]


@pytest.mark.parametrize("W", [1, 19])
@pytest.mark.parametrize("k", [1, 100, 1000])  # (1000 == n)
@pytest.mark.parametrize("chunk", [64, 256, 1000])
def test_search_is_the_top_k_of_its_own_scores(chunk, k, W):
    ops, lams, S = _search_case(W)
    tv, ti = want_topk(S, k)
    v, i = bare_search(*ops, lams, k, chunk)
    assert torch.equal(v, tv) and torch.equal(i, ti)


@pytest.mark.parametrize("W", [1, 19])
def test_search_folds_disjoint_id_ranges_from_separate_calls(W):
    ops, lams, S = _search_case(W)
    tv, ti = want_topk(S, 100)
    for ranges in ([(0, 333), (333, 1000)], [(613, 1000), (0, 613)]):
        v, i = bare_search(*ops, lams, 100, 256, id_ranges=ranges)
        assert torch.equal(v, tv) and torch.equal(i, ti), ranges


@pytest.mark.parametrize("k,chunk", [(1500, 512), (5000, 2048)])
def test_search_beyond_the_candidate_merge_runs_on_the_chunk_driver(k, chunk):
    n = 2000 if k == 1500 else 6000
    ops = [dev_bf16(x) for x in _gauss_case(k, 3, n, 32, 32)]
    lams = [0.5, 2.0]
    S = bare_score(*ops, lams, 0, n)
    tv, ti = want_topk(S, k)
    v, i = bare_search(*ops, lams, k, chunk, id_ranges=[(0, 700), (700, n)])
    assert torch.equal(v, tv) and torch.equal(i, ti)


@pytest.mark.parametrize("W", [1, 19])
def test_search_when_every_later_column_qualifies(W):
    """Scores rise with the passage id: every column of every filtered chunk beats its row's k-th entry, the candidate lists fill to
    `cols` (what the workspace is sized for)."""
    n, nq = 1000, 4
    c1 = np.zeros((n, 32), dtype=np.float32)
    c1[:, 0], c1[:, 1] = np.arange(n) // 8, (np.arange(n) % 8) / 8.0  # score j / 8, exact in bf16
    q1 = np.zeros((nq, 32), dtype=np.float32)
    q1[:, :2] = 32 * (np.arange(nq)[:, None] + 1)  # steps of 4 (i + 1) per id; the lexical part below moves a score by at most 1
    rng = np.random.default_rng(3)
    q2, c2 = SO.grid(rng, nq, 32), np.zeros((n, 32), dtype=np.float32)
    c2[:, 0] = (np.arange(n) % 5) / 8.0 - 0.25
    ops, lams = [dev_bf16(x) for x in (q1, q2, c1, c2)], SO.grid_lams(W)
    S = bare_score(*ops, lams, 0, n)
    assert np.array_equal(S.cpu().numpy().astype(np.float64).reshape(W, nq, n), SO.score(q1, q2, c1, c2, lams))
    for k, chunk in ((1, 64), (100, 64), (100, 256), (1000, 256)):
        tv, ti = want_topk(S, k)
        v, i = bare_search(*ops, lams, k, chunk)
        assert torch.equal(v, tv) and torch.equal(i, ti), (k, chunk)
    assert ti[0, 0].item() == n - 1


def test_search_exact_ties_go_to_the_lower_id():
    rng = np.random.default_rng(5)
    n, nq, W = 1000, 6, 3
    pick = rng.integers(0, 5, size=n)  # five distinct passages, each about 200 times
    c1, c2 = SO.grid(rng, 5, 32)[pick], SO.grid(rng, 5, 64)[pick]
    q1, q2 = SO.grid(rng, nq, 32), SO.grid(rng, nq, 64)
    ops, lams = [dev_bf16(x) for x in (q1, q2, c1, c2)], SO.grid_lams(W)
    S = bare_score(*ops, lams, 0, n)
    assert np.array_equal(S.cpu().numpy().astype(np.float64).reshape(W, nq, n), SO.score(q1, q2, c1, c2, lams))
    for k, chunk in ((10, 64), (300, 64), (300, 256), (1000, 1000)):
        tv, ti = want_topk(S, k)
        v, i = bare_search(*ops, lams, k, chunk)
        assert torch.equal(v, tv) and torch.equal(i, ti), (k, chunk)
    assert bool((ti[:, 1:] > ti[:, :-1]).logical_or(tv[:, 1:] < tv[:, :-1]).all())  # inside a tied group the ids ascend


def test_search_never_selects_a_nan():
    q1, q2, c1, c2 = _gauss_case(23, 4, 1000)
    bad = [0, 63, 64, 500, 999]
    c2[bad] = np.nan
    ops, lams = [dev_bf16(x) for x in (q1, q2, c1, c2)], [1.0, 0.0]
    S = bare_score(*ops, lams, 0, 1000)
    assert bool(torch.isnan(S[:, bad]).all()) and int(torch.isnan(S).sum()) == S.shape[0] * len(bad)
    for k, chunk in ((100, 64), (1000, 64), (1000, 256), (1000, 1000)):
        tv, ti = want_topk(S, k)
        v, i = bare_search(*ops, lams, k, chunk)
        assert torch.equal(v, tv) and torch.equal(i, ti), (k, chunk)
        assert not torch.isnan(v).any() and not bool(torch.isin(i, torch.tensor(bad, device=DEV)).any())
    assert bool((i[:, -len(bad):] == -1).all()) and bool(torch.isinf(v[:, -len(bad):]).all())  # k = n: the tails stay unfilled


def test_one_weight_of_one_equals_the_dense_search_on_concatenated_operands():
    """W = 1, lam = 1 on grid inputs: every sum is exact, so the new path and the one it generalises agree bit for bit."""
    from dpr_scale_amd import hotpath

    rng = np.random.default_rng(9)
    n, nq, k, chunk = 1000, 33, 100, 256
    q1, q2, c1, c2 = SO.grid(rng, nq, 96), SO.grid(rng, nq, 32), SO.grid(rng, n, 96), SO.grid(rng, n, 32)
    ops = [dev_bf16(x) for x in (q1, q2, c1, c2)]
    v, i = bare_search(*ops, [1.0], k, chunk)
    kn = hotpath.default_kernels()
    Q, C = torch.cat([ops[0], ops[1]], 1).contiguous(), torch.cat([ops[2], ops[3]], 1).contiguous()
    dv = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    di = torch.empty((nq, k), dtype=torch.int64, device=DEV)
    kn.search(Q, C, 0, dv, di, True, chunk, kn.search_workspace(nq, chunk, Q))
    assert torch.equal(v, dv) and torch.equal(i, di)


# ---------------------------------------------------------------- the Python layer on the device ----------------------------------------
@pytest.mark.parametrize("pooling", ["concat", "sum", "mean"])
def test_run_spar_retrieval_reproduces_the_reference_on_the_device(pooling, tmp_path):
    """tests/golden/spar_*.npz (the reference's own script, scripts/make_spar_golden.py) under the rule of the CPU test: scores exactly,
    ids exactly where a score is unique within its list, tied groups as sets."""
    import _spar_fixture as SF
    from conftest import load_golden
    from dpr_scale_amd import spar

    meta, z = load_golden(f"spar_{pooling}")
    kw = SF.write_inputs(tmp_path, z["p1"], z["p2"], list(z["q1"]), list(z["q2"]))
    out = tmp_path / "out"
    spar.run_spar_retrieval(output_dir=str(out), weights=meta["weights"], topk=meta["topk"], pooling=pooling, device=DEV, **kw)
    for s, recs in enumerate(SF.read_outputs(out, kw["output_filenames"])):
        assert [r["id"] for r in recs] == meta["question_ids"][s]
        SF.same_ranking([[c["score"] for c in r["ctxs"]] for r in recs], [[int(c["id"]) - 1 for c in r["ctxs"]] for r in recs],
                        z["scores"][s], z["rows"][s])


def test_spar_index_search_reproduces_the_concat_fixture_for_both_weights_in_one_pass(tmp_path):
    import _spar_fixture as SF
    from conftest import load_golden
    from dpr_scale_amd import spar

    meta, z = load_golden("spar_concat")
    index = spar.SparIndex(torch.from_numpy(z["p1"]), torch.from_numpy(z["p2"]), DEV, chunk=64)
    assert index.c1.is_cuda and index.c1.dtype == torch.bfloat16
    for s in range(len(meta["weights"])):
        v, i = index.search(z["q1"][s], z["q2"][s], meta["weights"], meta["topk"])  # both weights at once; dataset s was run with weight s
        assert v.shape == (2, meta["nq"], meta["topk"]) and v.is_cuda and i.dtype == torch.int64
        SF.same_ranking(v[s].cpu().numpy(), i[s].cpu().numpy(), z["scores"][s], z["rows"][s])
        s1, s2 = index.partial_scores(z["q1"][s], z["q2"][s], i)
        assert torch.equal(v, s1 + torch.tensor(meta["weights"], device=DEV).view(-1, 1, 1) * s2)  # grid inputs: exact
    kw = SF.write_inputs(tmp_path, z["p1"], z["p2"], list(z["q1"]), list(z["q2"]))
    loaded = spar.SparIndex.from_dirs(kw["ctx_embeddings_dir_1"], kw["ctx_embeddings_dir_2"], DEV)
    assert torch.equal(loaded.c1, index.c1) and torch.equal(loaded.c2, index.c2)
