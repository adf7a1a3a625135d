"""tests/_topk_oracle.py tied down on the CPU: the reference of the GPU conformance suite (test_topk_conformance_gpu.py) against
torch's stable sort and the project's present oracle where no NaN is involved, against itself when folded in pieces, and its NaN rule
and input generators by direct inspection.  The CPU-side folds (oracle.topk_merge and the stand-in kernels' topk_update_wide built on it,
which CorpusSearch reaches beyond k = 4096) are held to the same reference here."""
import numpy as np
import pytest
import torch

import _topk_oracle as T
from oracle import inbatch_oracle as O

BIG = (1 << 33) + 5


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])


def _nan_free(rows, cols, seed, mode):
    """The generator's modes without their NaNs (specials: each NaN pattern replaced by a subnormal; constant: the NaN row by -0)."""
    S = T.adversarial(rows, cols, seed, mode).copy()
    u = S.view(np.uint32)
    u[np.isnan(S)] = np.uint32(0x80000001) if mode == "specials" else np.uint32(0x80000000)
    assert not np.isnan(S).any()
    return S


@pytest.mark.parametrize("mode", ["gauss", "levels", "constant", "specials"])
@pytest.mark.parametrize("k", [1, 7, 300, 1500])
def test_reference_without_nan_is_the_stable_sort_prefix_and_the_present_oracle(mode, k):
    rows, cols = 6, 1200
    S = _nan_free(rows, cols, 11 + k, mode)
    v, i = T.fold(None, S, 0, k)
    m = min(k, cols)
    order = torch.sort(torch.from_numpy(S), dim=1, descending=True, stable=True).indices[:, :m].numpy()
    assert np.array_equal(i[:, :m], order) and np.array_equal(_bits(v[:, :m]), _bits(np.take_along_axis(S, order, axis=1)))
    assert np.all(i[:, m:] == -1) and np.all(_bits(v[:, m:]) == _bits(np.float32(-np.inf)))
    edges = [0, cols // 5, cols // 5 + 1, cols // 2, cols]
    st = None
    for a, b in zip(edges[:-1], edges[1:]):
        st = O.topk_merge(st, S[:, a:b], BIG + a, k)
        assert _same(st, T.fold(None, S[:, :b], BIG, k)), (a, b)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("k", [1, 40, 257, 1300])
def test_reference_folded_in_pieces_is_the_fold_of_the_whole(mode, k):
    rows, cols = 7, 1237
    S = T.adversarial(rows, cols, 5 + k, mode, k=min(k, cols - 40))
    whole = T.fold(None, S, BIG, k)
    for edges in ([0, cols], [0, cols // 5, cols // 5 + 1, cols // 2, cols], list(range(0, cols, 150)) + [cols]):
        assert _same(T.fold_pieces(S, edges, BIG, k), whole), edges
    # ... and in any order of the pieces (ids are what they are): the back half first
    st = T.fold(None, S[:, cols // 2:], BIG + cols // 2, k)
    assert _same(T.fold(st, S[:, :cols // 2], BIG, k), whole)


def test_reference_drops_every_nan_ties_the_zeroes_and_keeps_bit_patterns():
    pos, neg, sig, ones = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    S = np.array([[1.0, pos, 3.0, -np.inf, 2.0, neg, sig, ones],
                  [-0.0, 0.0, pos, -0.0, 1e-45, -1e-45, neg, 0.0]], dtype=np.float32)
    v, i = T.fold(None, S, 10, 6)
    assert i.tolist() == [[12, 14, 10, 13, -1, -1], [14, 10, 11, 13, 17, 15]]
    assert v[0].tolist() == [3.0, 2.0, 1.0, -np.inf, -np.inf, -np.inf]
    assert _bits(v[1]).tolist() == _bits(np.array([1e-45, -0.0, 0.0, -0.0, 0.0, -1e-45])).tolist()  # the zeroes in id order, signs kept
    # a state carries its unfilled slots and an (illegal) NaN of its own nowhere
    v2, i2 = T.fold((np.array([[5.0, pos, -np.inf]], np.float32), np.array([[3, 4, -1]], np.int64)), np.array([[neg, 5.0]], np.float32), 0, 3)
    assert i2.tolist() == [[1, 3, -1]] and v2.tolist() == [[5.0, 5.0, -np.inf]]


def test_generators_hold_what_they_promise():
    rows, cols, k = 6, 4000, 300
    S = T.adversarial(rows, cols, 3, "specials")
    u = S.view(np.uint32)
    for bits in T.SPECIAL_BITS:
        share = float((u == bits).mean())
        assert 0.01 < share < 0.03, (hex(bits), share)
    S = T.adversarial(rows, cols, 3, "nan_rows", k=k)
    assert (~np.isnan(S)).sum(axis=1).tolist() == [k + 40, k, k - 1, 5, 0, cols]
    assert (S.view(np.uint32) == 0x7FC00000).any() and (S.view(np.uint32) == 0xFFC00000).any()
    S = T.adversarial(rows, cols, 3, "constant")
    assert all(len(np.unique(S[r].view(np.uint32))) == 1 for r in range(rows))
    assert np.isnan(S[2]).all() and np.isneginf(S[1]).all() and np.isneginf(S[5]).all()
    S = T.adversarial(rows, cols, 3, "levels")
    assert np.array_equal(S, np.floor(S)) and S.min() == 0 and S.max() <= 4 and all(len(np.unique(S[r])) <= 5 for r in range(rows))
    v, i = T.fold(None, S, 0, k)
    assert all((S[r] == v[r, -1]).sum() > 100 for r in range(rows))  # ties by the hundred at the k-th score
    assert np.array_equal(T.adversarial(rows, cols, 3, "gauss"), T.adversarial(rows, cols, 3, "gauss"))


@pytest.mark.parametrize("mode", T.MODES)
def test_stand_in_wide_fold_follows_the_reference(mode):
    """OracleKernels.topk_update_wide (the fold CorpusSearch calls beyond k = 4096 on the stand-in kernels) and oracle.topk_merge: a NaN
    score is dropped, not sorted first (torch.sort) or taken when there is room (lexsort); unfilled slots stay last as -inf / -1; ties
    go to the lower id.  The error words stay zero."""
    from _oracle_kernels import OracleKernels

    rows, cols, k = 6, 900, 130
    S = T.adversarial(rows, cols, 17, mode, k=k)
    edges = [0, 100, 101, 450, cols]  # a first piece smaller than k
    kn = OracleKernels()
    values, indices = torch.full((rows, k), 7.0), torch.full((rows, k), 7, dtype=torch.int64)  # (a first call ignores what it finds)
    ws = kn.topk_wide_workspace(rows, k, values)
    st = None
    for a, b in zip(edges[:-1], edges[1:]):
        kn.topk_update_wide(torch.from_numpy(S[:, a:]), b - a, BIG + a, values, indices, a == 0, ws)  # (only `cols` columns are read)
        st = O.topk_merge(st, S[:, a:b], BIG + a, k)
        want = T.fold(None, S[:, :b], BIG, k)
        assert _same((values.numpy(), indices.numpy()), want), (mode, b, "OracleKernels.topk_update_wide")
        assert _same(st, want), (mode, b, "oracle.topk_merge")
        assert not bool(kn.topk_wide_errors(ws, rows).any())


def test_stand_in_search_beyond_the_streaming_kernel_drops_a_diverged_passage():
    """The whole stand-in path at k > 4096 (CorpusSearch._fold_wide on OracleKernels.topk_update_wide): one NaN passage, one NaN query."""
    from _oracle_kernels import OracleKernels
    from dpr_scale_amd.hotpath import CorpusSearch

    rng = np.random.default_rng(2)
    q = rng.integers(-2, 3, (4, 8)).astype(np.float32)
    c = rng.integers(-2, 3, (300, 8)).astype(np.float32)
    q[1] = np.nan
    c[77] = np.nan
    k = 4100
    s = CorpusSearch(torch.from_numpy(q), k, chunk=128, kernels=OracleKernels())
    s.add(torch.from_numpy(c[:130]), 0)
    s.add(torch.from_numpy(c[130:]), 130)
    v, i = s.result()
    with np.errstate(invalid="ignore"):
        S = (q.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)
    assert _same((v.numpy(), i.numpy()), T.fold(None, S, 0, k))
    assert (i[1] == -1).all() and torch.isneginf(v[1]).all() and not (i == 77).any() and int((i[0] >= 0).sum()) == 299
