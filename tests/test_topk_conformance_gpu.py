"""One contract, four engines: the per-row top-k fold every retrieval path ends in (include/dprhot.h) -- topk_stream_kernel of
csrc/rowwise.h in its three instantiations (k <= 256, <= 1024, <= 4096: dprhot_topk_update) and the HBM-resident selection of
csrc/wideselect.h (dprhot_topk_update_wide, any k) -- against the one reference of tests/_topk_oracle.py, against each other where
both take the same k, through the bare ABI between guard bands, and through CorpusSearch.  Order: score descending, id ascending; a
NaN score is never selected; unfilled slots are -inf / -1; the state after any sequence of updates is the fold of the concatenation.

Everything is compared bit for bit (values as int32, ids as int64), after every update, not only the last one.  The inputs
(_topk_oracle.adversarial): Gaussian scores, a few integer levels (thousands of ties, also at the k-th score), constant rows (all
-inf, all NaN, +0, -0), special values written as bit patterns (NaN of both signs and odd payloads, infinities, signed zeroes,
subnormals, the largest finite values), and rows with exactly k + 40 / k / k - 1 / 5 / 0 / all values that are not NaN.  The fold
schedules: one piece; pieces with a single-column one and -- for large k -- a first one smaller than k, cut out of a WIDER matrix
(row stride beyond the chunk, chunk not at the matrix's first column, +inf all around it); pieces of 1500 columns (for k >= 4097 the
state stays partly unfilled over several updates) with ids beyond 2^33."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _topk_oracle as T

pytestmark = pytest.mark.gpu

ROWS = 6
BIG = (1 << 33) + 5
LDS_K = [1, 256, 257, 1024, 1025, 4096]  # every boundary of launch_topk (csrc/dprhot.hip)
# one block of 4096, a ragged second block, two full blocks, ... five blocks: three merge passes with a ragged last run
WIDE_K = [1, 300, 4096, 4097, 8192, 8193, 12289, 17000]
PAD_L, PAD_R = 13, 11  # columns of +inf around the scores in the wider matrix: a read outside the chunk would win


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def kn():
    from dpr_scale_amd.hotpath import default_kernels

    return default_kernels()


def _cols(k):
    return max(20000, k + 3000)


def _schedules(cols):
    """(name, piece edges, col_offset, cut out of a wider matrix)"""
    return [("one piece", [0, cols], 0, False),
            ("ragged pieces of a wider matrix", [0, cols // 5, cols // 5 + 1, cols // 2, cols], 7, True),
            ("pieces of 1500", list(range(0, cols, 1500)) + [cols], BIG, False)]


@functools.lru_cache(maxsize=None)
def _scores(mode, k, rows=ROWS, cols=None):
    S = T.adversarial(rows, cols or _cols(k), 1000 * T.MODES.index(mode) + k, mode, k=k)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def _reference(mode, k):
    """Per schedule: the state after every piece, by the reference fold carried from piece to piece (computed once per input; shared
    by the engines)."""
    S = _scores(mode, k)
    out = {}
    for name, edges, off, _ in _schedules(S.shape[1]):
        st, states = None, []
        for a, b in zip(edges[:-1], edges[1:]):
            st = T.fold(st, S[:, a:b], off + a, k)
            states.append(st)
        out[name] = states
    return out


def _device_matrix(S, wider, dev):
    """The scores on the device, contiguous -- or inside a wider matrix of +inf; returns (matrix, first column of the scores)."""
    if not wider:
        return torch.tensor(S).to(dev), 0
    M = torch.full((S.shape[0], PAD_L + S.shape[1] + PAD_R), float("inf"), dtype=torch.float32)
    M[:, PAD_L:PAD_L + S.shape[1]] = torch.tensor(S)
    return M.to(dev), PAD_L


def _fold_on_gpu(kn, engine, S, edges, off, wider, k, dev):
    """The state (values as int32 bits, ids) after every piece.  The state buffers start as garbage: `first` must not read them."""
    M, c0 = _device_matrix(S, wider, dev)
    rows = S.shape[0]
    v = torch.full((rows, k), 123.0, dtype=torch.float32, device=dev)
    i = torch.full((rows, k), 77, dtype=torch.int64, device=dev)
    ws = kn.topk_wide_workspace(rows, k, M) if engine == "wide" else None
    states, first = [], True
    for a, b in zip(edges[:-1], edges[1:]):
        chunk = M[:, c0 + a:]
        assert chunk.stride(0) == M.shape[1] and (not wider or chunk.stride(0) > b - a)
        if engine == "wide":
            kn.topk_update_wide(chunk, b - a, off + a, v, i, first, ws)
        else:
            kn.topk_update(chunk, b - a, off + a, v, i, first)
        first = False
        states.append((v.cpu().view(torch.int32).clone(), i.cpu().clone()))
    if ws is not None:
        assert not bool(kn.topk_wide_errors(ws, rows).any())
    return states


def _where(got, want):
    bad = torch.nonzero((got[0] != want[0]) | (got[1] != want[1]))
    if bad.numel() == 0:
        return "equal"
    r, s = bad[0].tolist()
    f = lambda bits: f"{int(bits) & 0xffffffff:#010x}"  # noqa: E731
    return (f"{bad.shape[0]} slots differ, first at row {r} slot {s}: got ({f(got[0][r, s])}, {int(got[1][r, s])}), "
            f"want ({f(want[0][r, s])}, {int(want[1][r, s])})")


def _assert_states(got, want, what):
    assert len(got) == len(want)
    for piece, (g, w) in enumerate(zip(got, want)):
        w = (torch.from_numpy(w[0]).view(torch.int32), torch.from_numpy(w[1])) if isinstance(w[0], np.ndarray) else w
        assert torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]), f"{what}, after piece {piece}: {_where(g, w)}"


def _assert_nan_rows_shape(S, k, off, state, what):
    """As test_topk_never_selects_nan_whatever_the_start_up_path: m = min(n, k) real entries, then -1 / -inf."""
    St = torch.tensor(S)
    v, i = state[0].view(torch.float32), state[1]
    for r, n in enumerate(T.nan_keep(k, S.shape[1])):
        assert int((~torch.isnan(St[r])).sum()) == n
        order = torch.sort(torch.nan_to_num(St[r], nan=float("-inf")), descending=True, stable=True).indices[:min(n, k)]
        m = order.numel()
        assert torch.equal(i[r, :m], order + off) and torch.equal(v[r, :m], St[r, order]), (what, r)
        assert torch.all(i[r, m:] == -1) and torch.all(v[r, m:] == float("-inf")), (what, r)


def _engine_against_reference(kn, engine, mode, k, dev):
    S = _scores(mode, k)
    ref = _reference(mode, k)
    for name, edges, off, wider in _schedules(S.shape[1]):
        got = _fold_on_gpu(kn, engine, S, edges, off, wider, k, dev)
        what = f"{engine} engine, k={k}, {mode}, {name}"
        _assert_states(got, ref[name], what)
        if mode == "nan_rows":
            _assert_nan_rows_shape(S, k, off, got[-1], what)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("k", LDS_K)
def test_lds_engines_equal_the_reference(k, mode, kn, dev):
    _engine_against_reference(kn, "lds", mode, k, dev)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("k", WIDE_K)
def test_wide_engine_equals_the_reference(k, mode, kn, dev):
    _engine_against_reference(kn, "wide", mode, k, dev)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("k", LDS_K)
def test_wide_engine_equals_the_lds_engines_bit_for_bit(k, mode, kn, dev):
    """ "The same update for ANY k": at a k both take, the two entry points leave the same bits after every update."""
    S = _scores(mode, k)
    for name, edges, off, wider in _schedules(S.shape[1]):
        lds = _fold_on_gpu(kn, "lds", S, edges, off, wider, k, dev)
        wide = _fold_on_gpu(kn, "wide", S, edges, off, wider, k, dev)
        _assert_states(wide, lds, f"wide against lds, k={k}, {mode}, {name}")


@pytest.mark.parametrize("mode", ["specials", "levels"])
def test_wide_engine_on_many_rows_with_a_state_that_never_fills(mode, kn, dev):
    rows, cols, k = 130, 3000, 5000
    S = _scores(mode, k, rows, cols)
    edges = [0, 1700, cols]
    want, st = [], None
    for a, b in zip(edges[:-1], edges[1:]):
        st = T.fold(st, S[:, a:b], BIG + a, k)
        want.append(st)
    assert (want[-1][1][:, cols:] == -1).all()
    _assert_states(_fold_on_gpu(kn, "wide", S, edges, BIG, False, k, dev), want, f"wide engine, {rows} rows, {mode}")


GUARD = 4096
PATTERN = 0xA5


def _banded(nbytes, dev):
    raw = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=dev)
    return raw, raw[GUARD:GUARD + nbytes]


def test_wide_entry_point_through_the_bare_abi_stays_between_its_guard_bands(kn, dev):
    """values, indices and a workspace of EXACTLY dprhot_topk_wide_workspace_bytes bytes between 4 KiB bands (as test_guard_bands.py),
    called through ctypes: special values, two pieces, a row stride beyond the chunk; the records' error word (word 5) stays 0."""
    rows, k, cols = ROWS, 8193, 12000
    S = _scores("specials", k, rows, cols)
    M, c0 = _device_matrix(S, True, dev)
    need = ctypes.c_size_t(0)
    assert kn.lib.dprhot_topk_wide_workspace_bytes(rows, k, ctypes.byref(need)) == 0
    bufs = [_banded(rows * k * 4, dev), _banded(rows * k * 8, dev), _banded(need.value, dev)]
    (_, vb), (_, ib), (_, ws) = bufs
    assert all(b.data_ptr() % 16 == 0 for _, b in bufs)
    edges = [0, 5000, cols]  # the first piece is smaller than k
    want, st = [], None
    for n, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        chunk = M[:, c0 + a:]
        rc = kn.lib.dprhot_topk_update_wide(ctypes.c_void_p(chunk.data_ptr()), rows, b - a, M.shape[1], BIG + a, k, ctypes.c_void_p(vb.data_ptr()),
                                            ctypes.c_void_p(ib.data_ptr()), 1 if n == 0 else 0, ctypes.c_void_p(ws.data_ptr()), need.value, None)
        assert rc == 0
        torch.cuda.synchronize()
        st = T.fold(st, S[:, a:b], BIG + a, k)
        got = (vb.view(torch.int32).view(rows, k).cpu(), ib.view(torch.int64).view(rows, k).cpu())
        _assert_states([got], [st], f"bare ABI, piece {n}")
        assert not bool(ws[: rows * 32].view(torch.int32).view(rows, 8)[:, 5].any())
    for name, (raw, inner) in zip(("values", "indices", "workspace"), bufs):
        n = inner.numel()
        assert bool((raw[:GUARD] == PATTERN).all()), f"bytes BEFORE {name} were overwritten"
        assert bool((raw[GUARD + n:] == PATTERN).all()), f"bytes BEHIND {name} were overwritten"


# ---- the consumers: CorpusSearch over a corpus in which one embedding has diverged -------------------------------------------------
NAN_QUERY, ZERO_QUERY, NAN_PASSAGE = 2, 5, 1234


@pytest.fixture(scope="module")
def diverged(kn, dev):
    from dpr_scale_amd.hotpath import sim_score

    g = torch.Generator().manual_seed(9)
    q = torch.randn(9, 32, generator=g)
    c = torch.randn(9000, 32, generator=g)
    c[100:140] = c[60:100]  # duplicated passages: exact ties
    q[NAN_QUERY] = float("nan")
    q[ZERO_QUERY] = 0.0  # every score of this query ties: the ids alone decide
    c[NAN_PASSAGE] = float("nan")
    q, c = q.to(dev), c.to(dev)
    S = sim_score(q, c, kernels=kn).cpu().numpy()
    assert np.isnan(S[NAN_QUERY]).all() and np.isnan(S[:, NAN_PASSAGE]).all() and np.isnan(S).sum() == 9000 + 9 - 1
    assert (np.delete(S[ZERO_QUERY], NAN_PASSAGE) == 0).all()
    return q, c, S


@pytest.mark.parametrize("k", [100, 1500, 5000])  # dprhot_search (GEMM filter epilogue); dprhot_topk_update; dprhot_topk_update_wide
def test_corpus_search_with_a_diverged_query_and_passage_equals_the_reference(k, diverged, kn):
    from dpr_scale_amd.hotpath import CorpusSearch

    q, c, S = diverged
    s = CorpusSearch(q, k, chunk=2048, kernels=kn)
    s.add(c[:5003], 0)       # a ragged shard (5003 = 625 * 8 + 3) ...
    s.add(c[5003:], 5003)    # ... and the rest (3997)
    v, i = s.result()
    got = (v.cpu().view(torch.int32), i.cpu())
    _assert_states([got], [T.fold(None, S, 0, k)], f"CorpusSearch k={k}")
    assert bool((got[1][NAN_QUERY] == -1).all()) and bool(torch.isneginf(v[NAN_QUERY]).all())
    assert not bool((got[1] == NAN_PASSAGE).any())
    zero_ids = [j for j in range(k + 1) if j != NAN_PASSAGE][:k]
    assert got[1][ZERO_QUERY].tolist() == zero_ids
