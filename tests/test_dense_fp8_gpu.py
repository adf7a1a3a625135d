"""The fp8 dense index on the MI355X (csrc/dense_fp8.h through dprhot_fp8_encode / dprhot_dense_fp8_score / dprhot_dense_fp8_search).

The encoder must reproduce the oracle of tests/_fp8_oracle.py byte for byte.  One-hot code rows pin the operand map of
v_mfma_f32_16x16x32_fp8_fp8 (which lane holds which row and which features) with exact data; code values from a grid of integers and
halves must score BIT-EQUAL to the float64 oracle and to the bf16 `sim` kernel over decode().  Gaussian rows are held under a bound derived
from the arithmetic, not measured: dp exact products summed in fp32 in any order, rounded to nearest or truncated, are off by at most
2^-23 * (dp + 1) * sum_t |q_t c_t|; the two scale multiplies are by powers of two.  `search` is compared with the total-order top-k of
the kernel's own `score` matrix with torch.equal: near-ties cannot make it flaky.  Outputs and an exactly sized workspace sit between
4 KiB guard bands.  Every input is valid; nothing here provokes a fault.  No shape is larger than (129, 5000, 768)."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _fp8_oracle as FO  # noqa: E402
import _topk_oracle as TO  # noqa: E402

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


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return (t if dtype is None else t.to(dtype)).contiguous()


def bare_encode(x):
    """dprhot_fp8_encode through ctypes alone: rows fp32 or bf16 on the device -> (codes, scale) between guard bands."""
    from dpr_scale_amd import _lib

    n, d = x.shape
    dp = FO.padded_width(d)
    raws = []
    codes = _banded(raws, n * dp).view(n, dp)
    scale = _banded(raws, n * 4).view(torch.float32)
    _lib.check(_lib.lib.dprhot_fp8_encode(_p(x), int(x.dtype == torch.bfloat16), n, d, dp, _p(codes), _p(scale), _stream()), "dprhot_fp8_encode")
    _check_bands(raws)
    return codes.clone(), scale.clone()


def bare_score(Qc, qs, Cc, cs, doc_begin, cols, ld=None):
    """dprhot_dense_fp8_score through ctypes alone into S [nq, ld] between guard bands; the padding columns keep their fill pattern."""
    from dpr_scale_amd import _lib

    ld = (cols + 7) // 8 * 8 if ld is None else ld
    nq = Qc.shape[0]
    raws = []
    S = _banded(raws, nq * ld * 4).view(torch.float32).view(nq, ld)
    _lib.check(_lib.lib.dprhot_dense_fp8_score(_p(Qc), _p(qs), nq, _p(Cc), _p(cs), Cc.shape[0], Qc.shape[1], doc_begin, cols, _p(S), ld, _stream()),
               "dprhot_dense_fp8_score")
    _check_bands(raws)
    assert bool((S[:, cols:].contiguous().view(torch.uint8) == PATTERN).all()), "padding columns written"
    return S[:, :cols].clone()


def bare_search(Qc, qs, Cc, cs, k, chunk, id_ranges=None):
    """dprhot_dense_fp8_search through ctypes alone: values, indices and an exactly sized workspace sit between guard bands."""
    from dpr_scale_amd import _lib

    nq, n = Qc.shape[0], Cc.shape[0]
    nb = ctypes.c_size_t(0)
    _lib.check(_lib.lib.dprhot_dense_fp8_workspace_bytes(nq, chunk, ctypes.byref(nb)))
    nws = nb.value
    if k > 4096:
        _lib.check(_lib.lib.dprhot_topk_wide_workspace_bytes(nq, k, ctypes.byref(nb)))
        nws += nb.value
    raws = []
    values = _banded(raws, nq * k * 4).view(torch.float32).view(nq, k)
    indices = _banded(raws, nq * k * 8).view(torch.int64).view(nq, k)
    ws = _banded(raws, nws)
    first = 1
    for b, e in (id_ranges or [(0, n)]):
        _lib.check(_lib.lib.dprhot_dense_fp8_search(_p(Qc), _p(qs), nq, _p(Cc), _p(cs), n, Qc.shape[1], b, e, k, chunk, _p(values), _p(indices), first,
                                                    _p(ws), nws, _stream()), "dprhot_dense_fp8_search")
        first = 0
    _check_bands(raws)
    return values.clone(), indices.clone()


def want_topk(S, k):
    v, i = TO.fold(None, S.cpu().numpy(), 0, k)
    return torch.from_numpy(v).to(DEV), torch.from_numpy(i).to(DEV)


def same_bits(got, want64):
    """got fp32 (device) against the float64 oracle rounded once to fp32: the same bit patterns."""
    return np.array_equal(got.cpu().numpy().view(np.uint32), np.asarray(want64).astype(np.float32).view(np.uint32))


# ---------------------------------------------------------------- encode ---------------------------------------------------------------
def _encode_rows(n, d, seed):
    """Gaussian rows over 60 binades of row scale, the edge rows of the rule in front where they fit."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * np.exp2(rng.integers(-30, 31, size=(n, 1)))).astype(np.float32)
    edges = FO.edge_rows(d)
    if n >= len(edges):
        x[:len(edges)] = edges
    else:
        x[:] = edges[3:3 + n]  # (n == 1: the row of rounding midpoints)
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [32, 100, 768])
@pytest.mark.parametrize("n", [1, 1003])
def test_encode_equals_the_oracle(n, d, dtype):
    x = torch.from_numpy(_encode_rows(n, d, 100 * d + n)).to(dtype)
    want_c, want_s = FO.encode(x.float().numpy())
    codes, scale = bare_encode(x.to(DEV).contiguous())
    assert torch.equal(codes.cpu(), torch.from_numpy(want_c))
    assert torch.equal(scale.cpu().view(torch.int32), torch.from_numpy(want_s).view(torch.int32))  # (bit patterns: a NaN scale compares too)
    if n > 1:
        assert int(np.isnan(want_s).sum()) == 2 and int((want_c == 0x7E).sum()) > 0 and int((want_c == 0x80).sum()) > 0


# ---------------------------------------------------------------- the operand map ------------------------------------------------------
_HOT = [0x7E, 0xFE, 0x01, 0x80, 0x38, 0xB4, 0x45, 0x2A, 0x81, 0x5D, 0xC7, 0x08]  # 448, -448, 2^-9, -0, 1, -1.5, ...


@pytest.mark.parametrize("d", [32, 96, 160, 768])
def test_one_hot_rows_pin_the_operand_map(d):
    """Query row i has its only non-zero at feature (7 i + 3) mod d, passage row j at (5 j + 1) mod d: a cell is non-zero exactly where
    the two meet, so a wrong k order in either operand, or rows and columns swapped, moves the non-zeros.  The queries come in batches of
    at most 128 rows (no shape beyond 129 queries) that together hit every feature."""
    n = max(d + 5, 133)
    cc = np.zeros((n, d), dtype=np.uint8)
    j = np.arange(n)
    cc[j, (5 * j + 1) % d] = np.array(_HOT, dtype=np.uint8)[(j + 5) % len(_HOT)]
    cs = np.exp2(((2 * j) % 9) - 3).astype(np.float32)
    Cc, cs_d = dev(cc), dev(cs)
    hit = np.zeros(d, dtype=bool)
    for i0 in range(0, d, 128):
        i = np.arange(i0, min(i0 + 128, d))
        qc = np.zeros((len(i), d), dtype=np.uint8)
        qc[np.arange(len(i)), (7 * i + 3) % d] = np.array(_HOT, dtype=np.uint8)[i % len(_HOT)]
        qs = np.exp2((i % 9) - 3).astype(np.float32)
        hit[(7 * i + 3) % d] = True
        want = FO.score(qc, qs, cc, cs)
        got = bare_score(dev(qc), dev(qs), Cc, cs_d, 0, n)
        assert np.array_equal(got.cpu().numpy() != 0, want != 0), (d, i0)  # the zero pattern first: it names the map, not the arithmetic
        assert same_bits(got, want), (d, i0)
    assert hit.all()


# ---------------------------------------------------------------- exact scores ---------------------------------------------------------
_GRID_CODES = np.array([c for c in range(256) if not np.isnan(FO.TABLE[c]) and abs(FO.TABLE[c]) <= 4 and FO.TABLE[c] * 2 == round(FO.TABLE[c] * 2)],
                       dtype=np.uint8)  # the integers and halves in [-4, 4], -0 among them


def _grid_case(seed, nq, n, d):
    rng = np.random.default_rng(seed)
    qc, cc = _GRID_CODES[rng.integers(0, len(_GRID_CODES), (nq, d))], _GRID_CODES[rng.integers(0, len(_GRID_CODES), (n, d))]
    qs, cs = np.exp2(rng.integers(-3, 6, nq)).astype(np.float32), np.exp2(rng.integers(-3, 6, n)).astype(np.float32)
    return qc, qs, cc, cs


@pytest.mark.parametrize("nq,n,d", [(1, 8, 32), (17, 130, 96), (129, 1003, 160), (16, 256, 768)])
def test_grid_codes_score_bit_equal_to_the_oracle_and_to_the_bf16_sim(nq, n, d):
    from dpr_scale_amd import hotpath

    assert len(_GRID_CODES) == 18
    qc, qs, cc, cs = _grid_case(nq + n + d, nq, n, d)
    want = FO.score(qc, qs, cc, cs)  # every sum is exact in fp32: computed once
    Qc, qs_d, Cc, cs_d = dev(qc), dev(qs), dev(cc), dev(cs)
    got = bare_score(Qc, qs_d, Cc, cs_d, 0, n)
    assert same_bits(got, want)
    for doc_begin, cols in ((0, 1), (3, 5), (n // 2, n - n // 2)):
        assert same_bits(bare_score(Qc, qs_d, Cc, cs_d, doc_begin, cols, (cols + 7) // 8 * 8 + 8), want[:, doc_begin:doc_begin + cols])
    # the old path over the decoded rows: a true bf16 corpus (zero rows behind n up to the multiple of 8 that dprhot_sim_fwd takes)
    n8 = (n + 7) // 8 * 8
    Qb = dev(FO.decode(qc, qs).astype(np.float32), torch.bfloat16)
    Cb = torch.zeros((n8, d), dtype=torch.bfloat16, device=DEV)
    Cb[:n] = dev(FO.decode(cc, cs).astype(np.float32), torch.bfloat16)
    assert np.array_equal(Qb.double().cpu().numpy(), FO.decode(qc, qs))
    old = hotpath.default_kernels().sim(Qb, Cb)[:, :n]
    assert torch.equal(old.contiguous().view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("nq", [31, 32, 33])
def test_both_sides_of_the_short_query_tile_give_the_same_bits(nq):
    """At most 32 queries run on the 32-row tile, more on the 128-row tile: a score's bits do not depend on which."""
    qc, qs, cc, cs = _grid_case(77, 33, 261, 96)
    g = torch.Generator().manual_seed(nq)
    qg, cg = bare_encode(torch.randn(33, 96, generator=g).to(DEV)), bare_encode(torch.randn(261, 96, generator=g).to(DEV))
    assert same_bits(bare_score(dev(qc[:nq]), dev(qs[:nq]), dev(cc), dev(cs), 0, 261), FO.score(qc[:nq], qs[:nq], cc, cs))
    long = bare_score(*qg, *cg, 0, 261)                                 # 33 queries: the 128-row tile
    short = bare_score(qg[0][:nq].contiguous(), qg[1][:nq].contiguous(), *cg, 0, 261)
    assert torch.equal(short.view(torch.int32), long[:nq].contiguous().view(torch.int32))
    tv, ti = want_topk(short, 50)
    v, i = bare_search(qg[0][:nq].contiguous(), qg[1][:nq].contiguous(), *cg, 50, 64)
    assert torch.equal(v, tv) and torch.equal(i, ti)


def test_gaussian_scores_stay_within_the_derived_bound():
    """Section 13's bound, 2^-23 (dp + 1) sum_t |q_t c_t|.  On the MI355X the largest error is 0.058 of it.  The bound holds through its
    factor dp + 1: the unit's accumulation is coarser than a chain of fp32 additions and its error does not grow with dp (DESIGN.md
    section 14 has the figures; at dp = 96 the same formula would be exceeded, which is why no other width asserts it)."""
    nq, n, d = 64, 1000, 768
    g = torch.Generator().manual_seed(7)
    q, c = torch.randn(nq, d, generator=g), torch.randn(n, d, generator=g) * torch.exp2(torch.randint(-3, 4, (n, 1), generator=g).float())
    Qc, qs = bare_encode(q.to(DEV))
    Cc, cs = bare_encode(c.to(DEV))
    S = bare_score(Qc, qs, Cc, cs, 0, n).cpu().numpy().astype(np.float64)
    ops = [t.cpu().numpy() for t in (Qc, qs, Cc, cs)]
    err = np.abs(S - FO.score(*ops))
    bound = FO.bound(*ops)
    print(f"max err {err.max():.3e}, max err / bound {(err / bound).max():.4f}")
    assert bool((err <= bound).all())
    # another window: the same bits (a cell depends on its two code rows and its two scales only)
    S2 = bare_score(Qc, qs, Cc, cs, 100, 77).cpu().numpy().astype(np.float64)
    assert np.array_equal(S2, S[:, 100:177])


# ---------------------------------------------------------------- search ---------------------------------------------------------------
def _gauss_ops(seed, nq, n, d=64):
    g = torch.Generator().manual_seed(seed)
    q, c = torch.randn(nq, d, generator=g), torch.randn(n, d, generator=g)
    return [*bare_encode(q.to(DEV)), *bare_encode(c.to(DEV))]


_SEARCH = {}  # nq -> (device operands, the kernel's own score matrix): computed once, shared, never changed


def _search_case(nq):
    if nq not in _SEARCH:
        ops = _gauss_ops(11 + nq, nq, 1003)
        _SEARCH[nq] = (ops, bare_score(*ops, 0, 1003))
    return _SEARCH[nq]


@pytest.mark.parametrize("nq", [1, 129])
@pytest.mark.parametrize("k", [1, 100, 1003])  # (1003 == n)
@pytest.mark.parametrize("chunk", [64, 256, 1000])
def test_search_is_the_top_k_of_its_own_scores(chunk, k, nq):
    ops, S = _search_case(nq)
    tv, ti = want_topk(S, k)
    v, i = bare_search(*ops, k, chunk)
    assert torch.equal(v, tv) and torch.equal(i, ti)


@pytest.mark.parametrize("nq", [1, 129])
def test_search_folds_disjoint_id_ranges_from_separate_calls(nq):
    ops, S = _search_case(nq)
    tv, ti = want_topk(S, 100)
    for ranges in ([(0, 333), (333, 1003)], [(613, 1003), (0, 613)]):
        v, i = bare_search(*ops, 100, 256, id_ranges=ranges)
        assert torch.equal(v, tv) and torch.equal(i, ti), ranges


@pytest.mark.parametrize("k,chunk", [(1500, 512), (5000, 2048)])
def test_search_beyond_the_candidate_merge_runs_on_the_chunk_driver(k, chunk):
    n = 2000 if k == 1500 else 5000
    ops = _gauss_ops(k, 3, n, 32)
    S = bare_score(*ops, 0, n)
    tv, ti = want_topk(S, k)
    v, i = bare_search(*ops, k, chunk, id_ranges=[(0, 700), (700, n)])
    assert torch.equal(v, tv) and torch.equal(i, ti)


def test_search_when_every_later_column_qualifies():
    """Scores rise with the passage id: every column of every filtered chunk beats its row's k-th entry, the candidate lists fill to
    `cols` (what the workspace is sized for).  Passage j is (j >> 8, (j >> 4) & 15, j & 15, 0 ...), query i is (i + 1) * (256, 16, 1,
    0 ...): e4m3 with a row scale holds both without loss, the score (i + 1) * j is exact."""
    n, nq = 1000, 4
    j = np.arange(n)
    c = np.zeros((n, 32), dtype=np.float32)
    c[:, 0], c[:, 1], c[:, 2] = j >> 8, (j >> 4) & 15, j & 15
    q = np.zeros((nq, 32), dtype=np.float32)
    q[:, :3] = (np.arange(nq)[:, None] + 1) * np.array([256.0, 16.0, 1.0])
    ops = [*bare_encode(dev(q)), *bare_encode(dev(c))]
    S = bare_score(*ops, 0, n)
    assert np.array_equal(S.cpu().numpy().astype(np.float64), (np.arange(nq)[:, None] + 1.0) * j[None, :])
    for k, chunk in ((1, 64), (100, 64), (100, 256), (1000, 256)):
        tv, ti = want_topk(S, k)
        v, i = bare_search(*ops, k, chunk)
        assert torch.equal(v, tv) and torch.equal(i, ti), (k, chunk)
    assert ti[0, 0].item() == n - 1


def test_search_exact_ties_go_to_the_lower_id():
    rng = np.random.default_rng(5)
    n, nq = 1000, 6
    pick = rng.integers(0, 5, size=n)  # five distinct passages, each about 200 times
    c, q = FO.grid(rng, 5, 64)[pick], FO.grid(rng, nq, 64)
    ops = [*bare_encode(dev(q)), *bare_encode(dev(c))]
    S = bare_score(*ops, 0, n)
    assert np.array_equal(S.cpu().numpy().astype(np.float64), q.astype(np.float64) @ c.astype(np.float64).T)  # the grid is held without loss
    for k, chunk in ((10, 64), (300, 64), (300, 256), (1000, 1000)):
        tv, ti = want_topk(S, k)
        v, i = bare_search(*ops, k, chunk)
        assert torch.equal(v, tv) and torch.equal(i, ti), (k, chunk)
    assert bool((ti[:, 1:] > ti[:, :-1]).logical_or(tv[:, 1:] < tv[:, :-1]).all())  # inside a tied group the ids ascend


def test_search_never_selects_a_nan_scale_or_a_nan_code():
    g = torch.Generator().manual_seed(23)
    q, c = torch.randn(4, 64, generator=g), torch.randn(1000, 64, generator=g)
    bad_scale, bad_code = [0, 63, 500], [64, 999]
    c[bad_scale, 5] = float("nan")  # the encoder's answer to a non-finite row: scale NaN, codes 0x00
    Qc, qs = bare_encode(q.to(DEV))
    Cc, cs = bare_encode(c.to(DEV))
    assert bool(torch.isnan(cs[bad_scale]).all()) and not bool(Cc[bad_scale].any())
    Cc[64, 17], Cc[999, 63] = 0x7F, 0xFF  # a NaN code under a finite scale
    bad = bad_scale + bad_code
    S = bare_score(Qc, qs, Cc, cs, 0, 1000)
    assert bool(torch.isnan(S[:, bad]).all()) and int(torch.isnan(S).sum()) == S.shape[0] * len(bad)
    for k, chunk in ((100, 64), (1000, 64), (1000, 256), (1000, 1000)):
        tv, ti = want_topk(S, k)
        v, i = bare_search(Qc, qs, Cc, cs, k, chunk)
        assert torch.equal(v, tv) and torch.equal(i, ti), (k, chunk)
        assert not torch.isnan(v).any() and not bool(torch.isin(i, torch.tensor(bad, device=DEV)).any())
    assert bool((i[:, -len(bad):] == -1).all()) and bool(torch.isinf(v[:, -len(bad):]).all())  # k = n: the tails stay unfilled


# ---------------------------------------------------------------- the Python layer on the device ----------------------------------------
def test_dense_fp8_index_end_to_end_from_pickles_with_and_without_refine(tmp_path):
    from dpr_scale_amd import dense_fp8

    n, d, nq, k = 300, 96, 5, 10
    g = torch.Generator().manual_seed(31)
    p, q = torch.randn(n, d, generator=g), torch.randn(nq, d, generator=g)
    for s, (a, b) in enumerate(((0, 120), (120, 250), (250, 300))):
        with open(tmp_path / f"reps_{s:04d}.pkl", "wb") as f:
            pickle.dump(p[a:b].clone(), f, protocol=4)
    index = dense_fp8.DenseFP8Index.from_dirs(str(tmp_path), DEV, chunk=64, keep_exact=True)
    want_c, want_s = FO.encode(p.numpy())
    assert index.codes.is_cuda and index.corpus_len == n and index.nbytes == n * (d + 4)
    assert torch.equal(index.codes.cpu(), torch.from_numpy(want_c)) and torch.equal(index.scale.cpu(), torch.from_numpy(want_s))
    assert np.array_equal(index.decode().double().cpu().numpy(), FO.decode(want_c, want_s))
    S = index.score(q)
    qc, qs = FO.encode(q.numpy())
    err = np.abs(S.double().cpu().numpy() - FO.score(qc, qs, want_c, want_s))
    A = FO.bound(qc, qs, want_c, want_s) / (2.0 ** -23 * (index.dp + 1))  # sum_t |q_t c_t| on the decoded operands
    print(f"max err / sum |q c| at dp = {index.dp}: 2^{np.log2((err / A).max()):.1f}")  # (a figure for DESIGN.md section 14, no bound: see there)
    v, i = index.search(q, k)
    tv, ti = want_topk(S.contiguous(), k)
    assert torch.equal(v, tv) and torch.equal(i, ti)
    index.head = 72  # the head of an empty state as a range of its own (few queries): the same result
    assert all(torch.equal(a, b) for a, b in zip(index.search(q, k), (tv, ti)))
    index.head = dense_fp8.HEAD_IDS
    # refine: the fp8 top 4 k re-scored on the exact rows; ids against float64 (Gaussian gaps are far above fp32 rounding), values
    # within the fp32 dot product's bound
    rv, ri = index.search(q, k, refine=4)
    _, cand = index.search(q, 4 * k)
    for row in range(nq):
        ids = np.sort(cand[row].cpu().numpy())
        s = p[ids].double().numpy() @ q[row].double().numpy()
        order = np.lexsort((ids, -s))[:k]
        assert ri[row].tolist() == ids[order].tolist()
        tol = 2.0 ** -23 * (d + 1) * (p[ids[order]].double().abs().numpy() @ q[row].double().abs().numpy())
        assert bool((np.abs(rv[row].double().cpu().numpy() - s[order]) <= tol).all())
    exact = want_topk((q.to(DEV) @ p.to(DEV).T).contiguous(), k)[1]
    found = lambda ids: float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(ids.cpu(), exact.cpu())]))
    print(f"share of the fp32 top-{k}: fp8 {found(i):.3f}, refine=4 {found(ri):.3f}")
    assert found(ri) >= found(i)
    plain = dense_fp8.DenseFP8Index.from_codes(index.codes, index.scale, d)
    assert all(torch.equal(a, b) for a, b in zip(plain.search(q, k), (v, i)))
    with pytest.raises(ValueError, match="exact_rows"):
        plain.search(q, k, refine=2)
