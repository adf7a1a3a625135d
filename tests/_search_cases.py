"""The dense-search conformance table: named cases for every filter form of dprhot_search, and their fp64 oracle.  numpy only.

Inputs.  Every finite operand is a multiple of 1/4 with magnitude at most 2 (bf16-exact) and d <= 768, so every product is a multiple of
1/16 and every partial sum of absolute products stays below 2^24 / 16: fp32 accumulation is exact in any order, for any tile and any K
split.  `load` asserts that per case (the matmul of the absolute values, in sixteenths; the integers are far below 2^53, so fp64 holds
them exactly).  All comparisons are therefore bit for bit -- values as int32, ids as int64 -- with no tolerance.

Oracle.  Q.double() @ C.double().T, folded piece by piece with tests/_topk_oracle.fold: score descending, id ascending, NaN never
selected, -inf / -1 where unfilled.  The result does not depend on the pieces; they are the expected steps all the same, so that the
state after every CALL is at hand.

A case names the options it sets, the form (include/dprhot.h, dprhot_search_plan) every one of its launches must report, its shards in
increasing id order and the orders they are searched in ("inc"; "dec": decreasing id order, where the tie branch `col_offset + n < ti`
of the filter decides).  Designed cases also carry `counts`: the candidates each row must leave per filtered step, written down from
the construction, not computed."""
import contextlib
import functools
from dataclasses import dataclass, field

import numpy as np

from _topk_oracle import fold

TILES = {0: (128, 128, 64), 1: (64, 128, 64), 2: (64, 64, 64), 3: (32, 64, 64), 4: (32, 64, 256), 5: (32, 32, 256)}  # BM, BN, BK
FORM_BIG, FORM_8P, FORM_DMA = 6, 7, 8
HEAD_MAX = 65536    # an empty state starts from at most this many columns
NUM_WG = 256        # workgroups of the two persistent 256 x 256 kernels
TK_NSORT = {False: 256, True: 2048}  # longest candidate list merged without streaming: k <= 256, k > 256


@dataclass
class Case:
    name: str
    note: str
    options: dict
    form: int
    k: int
    chunk: int
    Q: np.ndarray                 # [nq, d] fp32
    shards: list                  # [(id_offset, C [n, d] fp32)] in increasing id order
    orders: dict                  # name -> shard indices in call order
    counts: dict = field(default_factory=dict)  # order -> per call, per step: None (head / not designed) or [nq] candidate counts

    @property
    def nq(self):
        return self.Q.shape[0]

    @property
    def d(self):
        return self.Q.shape[1]


def expected_steps(n, chunk, first):
    """Column counts of the launches over a shard of n rows: an empty state starts from a head of min(chunk, 65536) columns, and every
    chunk behind it is as long as everything before it (in whole groups of 8), between the head's length and `chunk`."""
    out, j0 = [], 0
    while j0 < n:
        if not first:
            step = chunk
        elif j0 == 0:
            step = min(chunk, HEAD_MAX)
        else:
            step = min(chunk, max(j0 // 8 * 8, min(chunk, HEAD_MAX)))
        out.append(min(step, n - j0))
        j0 += out[-1]
    return out


def plan(case, order):
    """Per call of `order`: [(j0, cols, head, form)] -- what dprhot_search_plan must report."""
    calls = []
    for c, si in enumerate(case.orders[order]):
        j0, steps = 0, []
        for cols in expected_steps(case.shards[si][1].shape[0], case.chunk, c == 0):
            steps.append((j0, cols, c == 0 and j0 == 0, case.form))
            j0 += cols
        calls.append(steps)
    return calls


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def _grid(rng, *shape):
    return (rng.integers(-8, 9, size=shape) / 4.0).astype(np.float32)


def _rows_with_sum(t, d):
    """[len(t), d] rows of multiples of 1/4 in [-2, 2] whose sums are t (multiples of 1/4, |t| <= 2 d)."""
    t = np.asarray(t, dtype=np.float64)
    assert np.all(np.abs(t) <= 2 * d) and np.array_equal(t * 4, np.round(t * 4))
    out, rem = np.zeros((len(t), d)), t.copy()
    for i in range(d):
        out[:, i] = np.clip(rem, -2, 2)
        rem -= out[:, i]
    assert not rem.any()
    return out.astype(np.float32)


def _diag(L, d):
    """Q [nq, d], C [n, d] with Q C^T == L exactly: row r of Q is 2 at dim r, column j of C holds L[r, j] / 2 there (L: multiples of
    1/2 in [-4, 4], nq <= d) -- every row's scores are chosen directly."""
    L = np.asarray(L, dtype=np.float64)
    nq, n = L.shape
    assert nq <= d and np.all(np.abs(L) <= 4) and np.array_equal(L * 2, np.round(L * 2))
    Q, C = np.zeros((nq, d), np.float32), np.zeros((n, d), np.float32)
    Q[np.arange(nq), np.arange(nq)] = 2
    C[:, :nq] = (L / 2).T
    return Q, C


def _twins(rng, nq, d, chunk, base, k=20):
    """Shard A: 2 * chunk rows at id `base`; shard B: chunk + 8 rows behind it.  B holds grid rows of the full range, A rows within
    [-1/2, 1/2], whose scores stay below B's best, and two copies of one row of B: the row that is query 0's k-th best in B (one copy
    per chunk of A).  Searched in decreasing id order the k-th best of the state after B therefore meets a score EQUAL to the
    threshold with a lower id in A's first chunk -- it must be taken, and it displaces the k-th best -- and the same score with a
    HIGHER id than the new k-th best in A's second chunk, which must be refused.  Both decisions are the id compare of the filter
    (`col_offset + n < ti`), and both change the state if made wrongly."""
    Q, B = _grid(rng, nq, d), _grid(rng, chunk + 8, d)
    A = (rng.integers(-2, 3, size=(2 * chunk, d)) / 4.0).astype(np.float32)
    s = Q[0].astype(np.float64) @ B.astype(np.float64).T
    kth = np.lexsort((np.arange(len(s)), -s))[k - 1]
    assert s[kth] > 0
    A[Q[0].astype(np.float64) @ A.astype(np.float64).T >= s[kth]] *= -1  # (query 0: nothing else of A reaches the threshold)
    A[5] = A[chunk + 3] = B[kth]
    return Q, [(base, A), (base + 2 * chunk, B)]


def _copies(rng, nq, d, chunk, base):
    """Shard A: 2 * chunk grid rows at id `base`; shard B: chunk + 8 rows behind it, copies of A's first rows (every score of B ties
    with one of A)."""
    A = _grid(rng, 2 * chunk, d)
    return _grid(rng, nq, d), [(base, A), (base + 2 * chunk, A[:chunk + 8].copy())]


_BUILDERS = {}


def _case(name):
    def reg(fn):
        _BUILDERS[name] = fn
        return fn
    return reg


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (1 << 32)


# register-staged tiles 0..5 and tile 0 on LDS-DMA: nq in {1, BM, BM + 1}, chunk one 8-column group past a multiple of BN,
# d in {BK, BK + 8, a partial-only K step}
def _tile_family():
    for t, (bm, bn, bk) in TILES.items():
        for nq in (1, bm, bm + 1):
            for dd in (bk, bk + 8, 8 if bk == 64 else 72):
                forms = [("reg", {"tile": t, "g128_dma": 0} if t == 0 else {"tile": t}, t)]
                if t == 0:  # g128_dma = 1: LDS-DMA where the launch qualifies (d % 64 == 0, at least 8 rows), else register-staged after all
                    forms.append(("dma", {"tile": 0, "g128_dma": 1}, FORM_DMA if dd % 64 == 0 and nq >= 8 else 0))
                for tag, opts, form in forms:
                    name = f"T{t}{tag}-nq{nq}-d{dd}"

                    def build(name=name, opts=opts, form=form, nq=nq, dd=dd, bn=bn):
                        Q, shards = _twins(np.random.default_rng(_seed(name)), nq, dd, 2 * bn + 8, 1000)
                        return Case(name, f"options {opts}: form {form}", opts, form, 20, 2 * bn + 8, Q, shards, {"inc": [0, 1], "dec": [1, 0]})
                    _BUILDERS[name] = build
        if t == 0:
            for dd in (128, 192):  # more than one whole K step on LDS-DMA
                name = f"T0dma-nq129-d{dd}"

                def build(name=name, dd=dd):
                    Q, shards = _twins(np.random.default_rng(_seed(name)), 129, dd, 264, 1000)
                    return Case(name, "tile 0 on LDS-DMA, several K steps", {"tile": 0, "g128_dma": 1}, FORM_DMA, 20, 264, Q, shards,
                                {"inc": [0, 1], "dec": [1, 0]})
                _BUILDERS[name] = build


# the two 256 x 256 kernels (big_min = 1): d = 192 -> gemm256_kernel<EpiFilter, PERSIST>, d = 128 / 256 -> gemm8p_kernel<Epi8Filter>
def _big_family():
    for dd, form in ((192, FORM_BIG), (128, FORM_8P), (256, FORM_8P)):
        for nq in (129, 256, 257):  # the M - 1 clamp of a ragged row tile, a full one, a second row tile of one row
            name = f"B{form}-d{dd}-nq{nq}"

            def build(name=name, dd=dd, form=form, nq=nq):
                Q, shards = _twins(np.random.default_rng(_seed(name)), nq, dd, 264, 1000)
                return Case(name, "one tile per workgroup, ragged last column tile", {"big_min": 1}, form, 20, 264, Q, shards,
                            {"inc": [0, 1], "dec": [1, 0]})
            _BUILDERS[name] = build
    # more tiles than workgroups: a first call on a 512-row shard, then first = 0 on one chunk.  129 x 65800: 1 x 258 tiles, two
    # workgroups filter two tiles each (the same row block); 640 x 21768: 3 x 86 = 258 tiles, and the second tile of both such workgroups
    # lies in the third row block (128 rows), their first in row block 0 (tile numbers 32 apart, row blocks fastest: 32 % 3 != 0)
    for dd, form in ((192, FORM_BIG), (128, FORM_8P)):
        for nq, n in ((129, 65800), (640, 21768)):
            name = f"B{form}-d{dd}-nq{nq}-258tiles"

            def build(name=name, dd=dd, form=form, nq=nq, n=n):
                rng = np.random.default_rng(_seed(name))
                Q = _grid(rng, nq, dd)
                # (rows of the third row block score a quarter as widely as those of the first: thresholds taken from there refuse
                #  nearly everything, also what belongs in the result)
                Q[512:] = (rng.integers(-2, 3, size=Q[512:].shape) / 4.0).astype(np.float32)
                return Case(name, "258 tiles on 256 workgroups, ragged last column tile", {"big_min": 1}, form, 20, n, Q,
                            [(0, _grid(rng, 512, dd)), (512, _grid(rng, n, dd))], {"inc": [0, 1]})
            _BUILDERS[name] = build


@_case("S-default-chunk")
def _s_default():
    rng = np.random.default_rng(11)
    return Case("S-default-chunk", "CorpusSearch's default chunk: steps 65536, 65536, 131072, 8", {}, 3, 20, 262144, _grid(rng, 8, 64),
                [(0, _grid(rng, 262152, 64))], {"inc": [0]})


@_case("S-chunk8-k20")
def _s_chunk8():
    rng = np.random.default_rng(12)
    A = _grid(rng, 40, 64)
    return Case("S-chunk8-k20", "chunk = 8 < k: filtering starts on a partly unfilled state (ti < 0)", {}, 3, 20, 8, _grid(rng, 3, 64),
                [(0, A), (40, A[:24].copy())], {"inc": [0, 1], "dec": [1, 0]})


@_case("S-three-shards")
def _s_three():
    rng = np.random.default_rng(13)
    A = _grid(rng, 144, 64)
    base = (1 << 33) + 8
    return Case("S-three-shards", "first = 0 continuation, ids beyond 2^33, twins across the shards", {}, 3, 20, 72, _grid(rng, 5, 64),
                [(base, A), (base + 1000, A[:80].copy()), (base + 5000, A[40:112].copy())], {"inc": [0, 1, 2], "dec": [2, 1, 0]})


# ---- designed scores ---------------------------------------------------------------------------------------------------------------
_RAMP_Q = (2.0, 1.0, 0.25, -2.0, -0.25, 0.0)


def _ramp(name, k):
    """792 columns whose row sums rise by 1/4 per id; row r of Q is the constant _RAMP_Q[r]: strictly increasing scores (every score
    passes: cnt == cols), strictly decreasing (nothing passes behind the head), constant (all ties)."""
    C = _rows_with_sum((np.arange(792) - 396) / 4.0, 64)
    Q = np.repeat(np.array(_RAMP_Q, np.float32)[:, None], 64, axis=1)
    up = np.array([264 if q > 0 else 0 for q in _RAMP_Q])       # later ids score higher
    low_first = np.array([264 if q <= 0 else 0 for q in _RAMP_Q])  # lower ids score higher, or tie and win on the id
    zero, every = np.zeros(len(_RAMP_Q), int), np.full(len(_RAMP_Q), 264)
    if k <= 264:
        counts = {"inc": [[None, up], [up]],                   # shard A = ids 0..527 (head + one chunk), then B = 528..791
                  "dec": [[None], [low_first, zero]]}          # B is the head; A's first chunk beats it or wins the ties, its second cannot
    else:  # the head leaves the state partly unfilled: the chunk behind it passes whole, whatever it scores
        # (dec, k = 300: after B and A's first chunk the k-th best is one of the 36 best of the lower-ranking of the two, and every score
        #  of A's second chunk ranks ahead of it in each of the three orders)
        assert 264 < k <= 528
        counts = {"inc": [[None, every], [up]], "dec": [[None], [every, every]]}
    return Case(name, "rank-1 ramp: all pass / none pass / all ties, per row", {}, 3, k, 264, Q, [(0, C[:528]), (528, C[528:])],
                {"inc": [0, 1], "dec": [1, 0]}, counts)


_case("D-ramp-k20")(lambda: _ramp("D-ramp-k20", 20))
_case("D-ramp-k300")(lambda: _ramp("D-ramp-k300", 300))


@_case("D-levels")
def _d_levels():
    rng = np.random.default_rng(21)
    nlev = np.array([1, 2, 3, 4, 5, 2])[:, None]
    L = np.floor(rng.random((6, 792)) * nlev) / 2.0  # a few levels per row: hundreds of ties, also at the k-th score
    Q, C = _diag(L, 64)
    return Case("D-levels", "1-5 score levels per row, a tie at the k-th score", {}, 3, 20, 264, Q, [(7, C[:528]), (535, C[528:])],
                {"inc": [0, 1], "dec": [1, 0]})


# per-row candidate counts against a warm state: the head's columns all score 0 (the state is k zeros with ids 0..k-1), the next chunk
# holds exactly c_r scores above 0 at scattered columns (1/2, the last of them 1) and -1/2 elsewhere
CNT = {1: (520, (0, 1, 255, 256, 257, 511, 512)),          # k + cnt = 256, 257 (cnt = TK_NSORT), 258 (TK_NSORT + 1), 512, 513
       256: (264, (0, 1, 255, 256, 257)),                  # k + cnt = 256, 257, 511, 512 (cnt = TK_NSORT), 513 (TK_NSORT + 1)
       257: (2056, (0, 1, 255, 256, 2048, 2049)),          # the 4096-slot instantiation: k + cnt = 512, 513; cnt = TK_NSORT, TK_NSORT + 1
       1024: (2056, (0, 1, 2048, 2049))}


def _cnt(k):
    chunk, want = CNT[k]
    rng = np.random.default_rng(30 + k)
    L = np.zeros((len(want), 2 * chunk))
    L[:, chunk:] = -0.5
    for r, c in enumerate(want):
        at = np.sort(rng.permutation(chunk)[:c])
        L[r, chunk + at] = 0.5
        L[r, chunk + at[-1:]] = 1.0  # the candidate of the highest column is the best: a list cut short by columns loses it
    Q, C = _diag(L, 64)
    return Case(f"D-cnt-k{k}", f"candidate counts {want} against a warm state", {}, 3, k, chunk, Q, [(0, C)], {"inc": [0]},
                {"inc": [[None, np.array(want)]]})


for _k in CNT:
    _case(f"D-cnt-k{_k}")(functools.partial(_cnt, _k))


# ---- non-finite operands -----------------------------------------------------------------------------------------------------------
@_case("N-nan-corpus-rows")
def _n_nan_corpus():
    rng = np.random.default_rng(41)
    Q, shards = _copies(rng, 4, 64, 72, 1000)
    shards[0][1][[0, 5, 71, 72, 100, 143]] = np.nan  # in the head and in the filtered chunk
    shards[1][1][[3, 79]] = np.nan
    return Case("N-nan-corpus-rows", "NaN passages are never selected", {}, 3, 20, 72, Q, shards, {"inc": [0, 1], "dec": [1, 0]})


@_case("N-nan-few-left")
def _n_nan_few():
    rng = np.random.default_rng(42)
    C = _grid(rng, 32, 64)
    C[rng.permutation(32)[:14]] = np.nan  # 18 real candidates for k = 20: the tail stays -inf / -1
    return Case("N-nan-few-left", "fewer real candidates than k", {}, 3, 20, 16, _grid(rng, 4, 64), [(0, C[:16]), (16, C[16:])],
                {"inc": [0, 1], "dec": [1, 0]})


@_case("N-nan-query-row")
def _n_nan_query():
    rng = np.random.default_rng(43)
    Q, shards = _copies(rng, 4, 64, 72, 1000)
    Q[1] = np.nan
    return Case("N-nan-query-row", "a NaN query: its whole row stays -inf / -1", {}, 3, 20, 72, Q, shards, {"inc": [0, 1], "dec": [1, 0]})


@_case("N-inf")
def _n_inf():
    rng = np.random.default_rng(44)
    Q, shards = _copies(rng, 4, 64, 8, 1000)  # chunk = 8 < k: -inf scores meet unfilled slots
    Q[:, 0] = [1, -1, 0, 2]                    # +inf passages score +inf, -inf, NaN (0 * inf), +inf
    for _, C in shards:
        C[:, 0] = np.abs(C[:, 0])
    shards[0][1][[1, 2, 9, 12], 0] = [np.inf, -np.inf, np.inf, -np.inf]
    shards[1][1][[0, 3, 11], 0] = [-np.inf, np.inf, np.inf]
    # (k = 30 of 32 passages: -inf scores with real ids end up in the state; the NaN row keeps an unfilled tail)
    return Case("N-inf", "+inf and -inf scores, -inf against unfilled slots", {}, 3, 30, 8, Q, shards, {"inc": [0, 1], "dec": [1, 0]})


_tile_family()
_big_family()
NAMES = sorted(_BUILDERS)
LARGE = [n for n in NAMES if n.endswith("258tiles") or n == "S-default-chunk"]


# ---- loading: exactness, scores, oracle states --------------------------------------------------------------------------------------
@dataclass
class Loaded:
    case: Case
    S: list        # per shard: [nq, n] fp32, the exact scores
    states: dict   # order -> per call (values [nq, k] fp32, ids [nq, k] int64) after the call


def check_exact(Q, C):
    """Finite operands on the quarter grid within [-2, 2], d <= 768, every sum of absolute products below 2^24 sixteenths."""
    d = Q.shape[1]
    assert d <= 768 and C.shape[1] == d
    a, b = (np.where(np.isfinite(x), np.abs(x), 0).astype(np.float64) * 4 for x in (Q, C))
    assert np.array_equal(a, np.round(a)) and np.array_equal(b, np.round(b)) and a.max(initial=0) <= 8 and b.max(initial=0) <= 8
    assert float((a @ b.T).max(initial=0)) < 2 ** 24
    return True


def scores(Q, C):
    with np.errstate(invalid="ignore"):
        S = Q.astype(np.float64) @ C.astype(np.float64).T
    S32 = S.astype(np.float32) + np.float32(0)  # (a sum that starts from +0 is never -0, whatever the products' signs)
    fin = np.isfinite(S)
    assert np.array_equal(S32[fin].astype(np.float64), S[fin])
    return S32


@functools.lru_cache(maxsize=3)
def load(name):
    case = _BUILDERS[name]()
    assert case.name == name and case.chunk % 8 == 0 and all(C.shape[0] % 8 == 0 for _, C in case.shards)
    assert all(a + A.shape[0] <= b for (a, A), (b, _) in zip(case.shards[:-1], case.shards[1:])), "shards in increasing, disjoint id order"
    for _, C in case.shards:
        check_exact(case.Q, C)
    S = [scores(case.Q, C) for _, C in case.shards]
    states = {}
    for order, seq in case.orders.items():
        st, out = None, []
        for call, si in zip(plan(case, order), seq):
            for j0, cols, _, _ in call:
                st = fold(st, S[si][:, j0:j0 + cols], case.shards[si][0] + j0, case.k)
            out.append(st)
        states[order] = out
    return Loaded(case, S, states)


# ---- the library side: options and the plan query (host code only) -----------------------------------------------------------------
@contextlib.contextmanager
def options(case):
    """The case's options set in the library; what they were before is restored on the way out."""
    from dpr_scale_amd import _lib

    saved = {o: _lib.get_option(o) for o in case.options}
    try:
        for o, v in case.options.items():
            _lib.set_option(o, v)
        yield
    finally:
        for o, v in saved.items():
            _lib.set_option(o, v)


def check_plan(case):
    """dprhot_search_plan reports the table's forms and steps for every call of every order (under the options in force)."""
    from dpr_scale_amd import _lib

    for order, seq in case.orders.items():
        for c, (want, si) in enumerate(zip(plan(case, order), seq)):
            got = _lib.search_plan(case.nq, case.shards[si][1].shape[0], case.d, case.k, case.chunk, c == 0)
            assert got == want, (case.name, order, c, got, want)
