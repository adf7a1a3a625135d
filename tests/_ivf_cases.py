"""TEST-ONLY case table of the inverted-index scorers (csrc/ivf.h, csrc/ivf_pq.h), importable without a GPU.

A case is a function returning a `Case`: (postings, queries, corpus_len, d, doc_begin, cols, ld, seed, note) in the unpacked form
of tests/_ivf_oracle.py -- postings {expert: (ids int64 [n], rows fp32 [n, d])}, queries [{expert: [vector, ...]}, ...] -- plus the
window `S [nq, ld]` takes doc ids doc_begin .. doc_begin + cols of, and the seed of the window's prefill.

Every value is GRID-VALUED: a multiple of 1/4 in [-2, 2], exact in bf16.  With dp <= 128 a dot product is a multiple of 1/16 of
magnitude at most 2^9, and with at most 64 entries per query every cell s of the score matrix satisfies 16 (|s| + 2) < 2^24 (the 2
is the prefill), so fp32 accumulation is exact in any order and a kernel must equal the fp64 oracle BIT FOR BIT.  `load` asserts
that condition on the oracle's output of every case: it is a condition on the inputs, not a tolerance.  (Family F adds NaN and
+-inf operands; the only non-finite cell value is +inf.)

Families, each aimed at one line of ivf_score_kernel (names in NAMES; `shape_*` build them):
  A  batch experts, `b0 += 64`            nb in {1, 63, 64, 65, 129}
  B  entry groups, `eg += 16`             ne in {1, 15, 16, 17, 33} entries of one expert
  C  postings of one (expert, range), `c0 += 64`, and a doc's run across slice positions 63|64 and 127|128
  D  the doc window (doc_begin, cols, ld) and postings on every edge of it and of its 128-doc ranges
  E  width, `k += 32`: d in {20, 32, 40, 64, 96, 128}; and the PQ shapes (dp, dsub) in {32, 64} x {2, 4, 8}
  F  NaN, +inf, -inf, inf x 0
  G  the Zipf layout of tests/test_ivf_gpu.py's synth, grid-valued, with a CLS part
`pq_form(name)` gives a case as 8-bit codes over a grid codebook that holds its rows exactly (random posting rows are put together
from pools of 8-feature pieces so that every subspace of 2, 4 or 8 features has at most 256 distinct sub-vectors)."""
import functools
from typing import NamedTuple

import numpy as np
import torch

import _ivf_oracle as O

T, ROWS, SLICE = 128, 16, 64  # csrc/ivf.h: doc ids per wave, entries per MFMA step, postings per MFMA step
MAX_ENTRIES = 64               # per query, in this table


class Case(NamedTuple):
    postings: dict
    queries: list
    corpus_len: int
    d: int
    doc_begin: int
    cols: int
    ld: int
    seed: int
    note: str


class _Values:
    """The value source of one case: `rows(n)` posting rows, `vec()` a query vector.  grid: multiples of 1/4 in [lo / 4, hi / 4], rows
    put together from a pool of `pool` 8-feature pieces per block of 8 features; gauss: standard normal."""

    def __init__(self, seed, d, values="grid", lo=-8, hi=8, pool=160):
        self.g, self.d, self.kind, self.lo, self.hi = np.random.default_rng(seed), d, values, lo, hi
        self.nblk = (d + 7) // 8
        self.pool = self.g.integers(lo, hi + 1, size=(self.nblk, pool, 8)) / 4.0

    def rows(self, n):
        if self.kind == "gauss":
            return self.g.standard_normal((n, self.d)).astype(np.float32)
        pick = self.g.integers(0, self.pool.shape[1], size=(n, self.nblk))
        return self.pool[np.arange(self.nblk)[None, :], pick].reshape(n, self.nblk * 8)[:, : self.d].astype(np.float32)

    def vec(self):
        if self.kind == "gauss":
            return self.g.standard_normal(self.d).astype(np.float32)
        return (self.g.integers(self.lo, self.hi + 1, size=self.d) / 4.0).astype(np.float32)


def _t(v):
    return torch.from_numpy(np.asarray(v, dtype=np.float32).copy())


# ---- A: batch experts -----------------------------------------------------------------------------------------------------------------
A_NB = (1, 63, 64, 65, 129)


def shape_a(nb, values="grid", d=32, seed=100):
    """Index of experts 0 .. 139, three postings each (expert 3: an empty list inside the index; expert 2: all postings in docs
    128 .. 255, so two of the three waves find nothing of it), 300 docs.  The batch's nb distinct experts in ascending order: expert
    1000 lies beyond the index (always the last one), and the 65th, expert 64, is the only contributor to cell (query 1, doc 299):
    no other expert has doc 299, and its posting there is the query's own vector."""
    V, ndocs, nq = 140, 300, 3
    val = _Values(seed + nb, d, values)
    g = val.g
    post = {}
    for e in range(V):
        if e == 3:
            continue
        if e == 2:
            ids = np.sort(g.integers(128, 256, size=3))
        elif e == 64:
            ids = np.array([10, 140, 299])
        else:
            ids = np.sort(g.integers(0, 299, size=3))
        post[e] = (ids.astype(np.int64), val.rows(3))
    experts = {1: [64], 63: list(range(62)) + [1000], 64: list(range(63)) + [1000], 65: list(range(65)),
               129: list(range(128)) + [1000]}[nb]
    assert len(experts) == nb
    queries = [{} for _ in range(nq)]
    for e in experts:
        for n in [e % 3] + ([(e + 1) % 3] if e % 5 == 0 else []):
            queries[n].setdefault(e, []).append(_t(val.vec()))
    if 64 in experts:
        u = queries[64 % 3][64][0].numpy().copy()
        if not u.any():
            u[0] = 1.0
            queries[64 % 3][64][0] = _t(u)
        post[64][1][2] = u
    return Case(post, queries, ndocs, d, 0, ndocs, 304, 1000 + nb, f"{nb} batch experts over an index of {V}")


# ---- B: entry groups ------------------------------------------------------------------------------------------------------------------
B_COUNTS = {1: (0, 1, 0), 15: (5, 5, 5), 16: (5, 6, 5), 17: (4, 13, 0), 33: (10, 12, 11)}


def shape_b(ne):
    """One expert (id 3) with ne entries over three queries, B_COUNTS[ne] of them per query: entries are sorted by (expert, query),
    so a query's entries sit side by side -- several times inside one group of 16, and for ne = 17 and 33 as entries 16 and 17 on
    both sides of the group edge."""
    val = _Values(200 + ne, 32)
    g = val.g
    ids = g.integers(0, 200, size=40)
    ids[5:8] = ids[4]  # a run of four postings of one doc
    post = {3: (np.sort(ids).astype(np.int64), val.rows(40)), 5: (np.sort(g.integers(0, 200, size=4)).astype(np.int64), val.rows(4))}
    queries = [({3: [_t(val.vec()) for _ in range(c)]} if c else {}) for c in B_COUNTS[ne]]
    return Case(post, queries, 200, 32, 0, 200, 200, 2000 + ne, f"{ne} entries of one expert over 3 queries")


# ---- C: postings per (expert, range) and a doc's run ---------------------------------------------------------------------------------
C_RUNS = {1: [1], 63: [1, 2] * 21, 64: [64], 65: [1, 64], 129: [62, 65, 2], 200: [60, 130, 2, 8]}


def shape_c(pc):
    """Expert 7 has pc postings inside docs 128 .. 255 (plus five below and three above that range), cut into runs of one doc each of
    the lengths C_RUNS[pc]; position c of the range's slice is the posting's place in that list.  Features 0, 1, 2 of a run are
    designed: feature 0 is largest (2) on the run's FIRST posting, feature 1 on its LAST, feature 2 on the first posting BEHIND the
    last slice boundary (c = 64 or 128) the run straddles (its middle one where it straddles none); elsewhere they lie in
    [-2, 1.75].  Queries 0, 1, 2 pick one of those features each (1.5 e0, e1, 2 e2), so each asks for another winner; query 1 also
    holds a random entry.  One short run of a list of several (the last; for pc = 65 the first) is negative in all three features:
    those cells stay untouched."""
    runs = C_RUNS[pc]
    assert sum(runs) == pc
    val = _Values(300 + pc, 32)
    g = val.g
    docs = np.repeat(128 + np.sort(g.choice(128, size=len(runs), replace=False)), runs)
    rows = val.rows(pc)
    rows[:, :8] = 0
    neg = None if len(runs) == 1 else len(runs) - 1 if runs[-1] < 10 else 0  # (a short run: the long ones carry the winners)
    pos = 0
    for j, L in enumerate(runs):
        if j == neg:
            rows[pos:pos + L, :3] = -g.integers(1, 9, size=(L, 3)) / 4.0
        else:
            f = g.integers(-8, 8, size=(L, 3)) / 4.0
            edges = [b for b in (SLICE, 2 * SLICE) if pos < b <= pos + L - 1]
            far = edges[-1] - pos if edges else L // 2
            f[0, 0], f[L - 1, 1], f[far, 2] = 2.0, 2.0, 2.0
            rows[pos:pos + L, :3] = f
        pos += L
    below, above = np.sort(g.integers(0, 128, size=5)), np.sort(g.integers(256, 400, size=3))
    post = {7: (np.concatenate([below, docs, above]).astype(np.int64), np.concatenate([val.rows(5), rows, val.rows(3)]))}
    e = np.eye(32, dtype=np.float32)
    queries = [{7: [_t(1.5 * e[0])]}, {7: [_t(e[1]), _t(val.vec())]}, {7: [_t(2 * e[2])]}]
    return Case(post, queries, 400, 32, 0, 400, 400, 3000 + pc, f"{pc} postings of one expert in one 128-doc range, runs {runs}")


# ---- D: the doc window ----------------------------------------------------------------------------------------------------------------
D_WINDOWS = ((0, 1), (0, 127), (0, 128), (0, 129), (0, 512), (0, 513), (1, 128), (127, 2), (130, 383), (5, 1000))


def shape_d(doc_begin, cols, wide):
    """Corpus of 1200; experts 1 and 4 both hold doc ids doc_begin - 1, doc_begin, doc_begin + 128 j - 1, + 0, + 1 for every range j
    (one past the window's last), doc_begin + cols - 1 and doc_begin + cols (expert 1 twice each), plus 30 random ones.  All values
    lie in [0.25, 2]: every posting has a positive product with every entry, so a posting wrongly taken or left is seen."""
    ndocs = 1200
    ld = (cols + 7) // 8 * 8 + (24 if wide else 0)
    val = _Values(400 + 7 * doc_begin + cols, 32, lo=1, hi=8)
    g = val.g
    special = {doc_begin - 1, doc_begin, doc_begin + cols - 1, doc_begin + cols}
    special |= {doc_begin + 128 * j + k for j in range(cols // 128 + 2) for k in (-1, 0, 1)}
    special = np.array(sorted(x for x in special if 0 <= x < ndocs))
    post = {}
    for e, rep in ((1, 2), (4, 1)):
        ids = np.sort(np.concatenate([np.repeat(special, rep), g.integers(0, ndocs, size=30)])).astype(np.int64)
        post[e] = (ids, val.rows(len(ids)))
    queries = [{1: [_t(val.vec())], 4: [_t(val.vec()), _t(val.vec())]}, {1: [_t(val.vec()), _t(val.vec())], 4: [_t(val.vec())]}]
    return Case(post, queries, ndocs, 32, doc_begin, cols, ld, 4000 + 3 * doc_begin + cols + wide,
                f"window doc_begin={doc_begin} cols={cols} ld={ld} of a corpus of {ndocs}")


# ---- E: width -------------------------------------------------------------------------------------------------------------------------
E_D = (20, 32, 40, 64, 96, 128)
E_PQ = tuple((dp, dsub) for dp in (32, 64) for dsub in (2, 4, 8))


def shape_e(d):
    """Expert 2: 48 postings, posting i non-zero (and positive) in the 32-feature block i mod (dp / 32) only; expert 6: 12 dense
    random postings.  The entries of expert 2 are constant inside a block and differ from block to block, so a K step that is
    skipped, repeated or taken from another block changes the score."""
    nblk = (d + 31) // 32
    val = _Values(500 + d, d, lo=1, hi=8)
    g = val.g
    ids = np.sort(g.integers(0, 150, size=48)).astype(np.int64)
    rows = val.rows(48)
    blk = np.arange(d) // 32
    for i in range(48):
        rows[i, blk != i % nblk] = 0
    dense = _Values(550 + d, d)
    post = {2: (ids, rows), 6: (np.sort(g.integers(0, 150, size=12)).astype(np.int64), dense.rows(12))}
    up, down = ((1 + blk) / 4.0).astype(np.float32), (2 - blk / 4.0).astype(np.float32)
    queries = [{2: [_t(up)], 6: [_t(dense.vec())]}, {2: [_t(down), _t(dense.vec())]}]
    return Case(post, queries, 150, d, 0, 150, 152, 5000 + d, f"d={d} (dp={nblk * 32}), postings of one 32-feature block each")


_PQ_GIVEN = {}  # case name -> (dsub, codebook fp32 [m, 256, dsub], {expert: codes uint8 [n, m]}) of the cases born as codes


def shape_e_pq(dp, dsub, name=None):
    """A grid-valued codebook [dp / dsub, 256, dsub] and random codes: experts 0, 2, 5 with 70, 20, 10 postings in 150 docs (70 of one
    expert: some 128-doc range holds a run of several).  The rows of the case are the decoded ones."""
    g = np.random.default_rng(700 + dp + dsub)
    m = dp // dsub
    codebook = (g.integers(-8, 9, size=(m, 256, dsub)) / 4.0).astype(np.float32)
    post, codes = {}, {}
    for e, n in ((0, 70), (2, 20), (5, 10)):
        ids = np.sort(g.integers(0, 150, size=n)).astype(np.int64)
        codes[e] = g.integers(0, 256, size=(n, m)).astype(np.uint8)
        post[e] = (ids, codebook[np.arange(m)[None, :], codes[e]].reshape(n, dp))
    vec = lambda: _t(g.integers(-8, 9, size=dp) / 4.0)
    queries = [{0: [vec(), vec()], 5: [vec()]}, {0: [vec()], 2: [vec(), vec()]}, {2: [vec()], 9: [vec()]}]
    if name is not None:
        _PQ_GIVEN[name] = (dsub, codebook, codes)
    return Case(post, queries, 150, dp, 0, 150, 152, 7000 + dp + dsub, f"PQ dp={dp} dsub={dsub}: grid codebook, random codes")


# ---- F: non-finite --------------------------------------------------------------------------------------------------------------------
F_KINDS = ("nan_alone", "nan_beside_positive", "nan_query_entry", "pos_inf", "neg_inf", "inf_times_zero")


def shape_f(kind):
    """Ten docs, expert 0, query 0 = ones (and what the kind adds), query 1 random.  The kind's postings sit on doc 1 or 3."""
    d = 32
    val = _Values(600 + F_KINDS.index(kind), d)
    ones = np.ones(d, dtype=np.float32)
    ids, rows = [0, 2, 2, 5, 7], list(val.rows(5))
    q0 = [ones.copy()]
    at = lambda x: np.concatenate([val.rows(1)[0][:2], [x], val.rows(1)[0][3:]]).astype(np.float32)  # a grid row, x in feature 2
    if kind == "nan_alone":
        extra = [(1, np.full(d, np.nan, dtype=np.float32))]
    elif kind == "nan_beside_positive":
        extra = [(1, np.full(d, np.nan, dtype=np.float32)), (1, 2 * ones)]
    elif kind == "nan_query_entry":
        bad = val.vec()
        bad[4] = np.nan
        q0, extra = [ones.copy(), bad], [(1, 2 * ones)]
    elif kind == "pos_inf":
        extra = [(3, at(np.inf))]
    elif kind == "neg_inf":
        extra = [(3, at(-np.inf))]
    else:
        q0[0][2] = 0.0  # inf x 0 inside the dot product: NaN, the posting counts as absent and the quarter row wins
        extra = [(3, at(np.inf)), (3, 0.25 * ones)]
    for doc, row in extra:
        ids.append(doc)
        rows.append(row)
    order = np.argsort(np.array(ids), kind="stable")
    post = {0: (np.array(ids, dtype=np.int64)[order], np.stack(rows)[order].astype(np.float32))}
    queries = [{0: [_t(u) for u in q0]}, {0: [_t(val.vec())]}]
    return Case(post, queries, 10, d, 0, 10, 16, 6000 + F_KINDS.index(kind), kind.replace("_", " "))


# ---- G: mixed -------------------------------------------------------------------------------------------------------------------------
_CLS = {}  # case name -> (cls_q fp32 [nq, dc], cls_doc fp32 [ndocs, dc])


def shape_g(values="grid", d=64, seed=7, name=None, ndocs=2003, V=150, nq=8, ne=24, dc=24, hot_frac=0.6):
    """The layout of tests/test_ivf_gpu.py's synth: Zipf expert sizes, expert 0 with a posting in more than half of the docs (several
    in many) and a quarter of every query's 24 entries; 2003 docs, 150 experts, 8 queries."""
    val = _Values(seed, d, values)
    g = val.g
    post = {}
    for e in range(V):
        n = max(2, int(ndocs * hot_frac * 1.6 / (e + 1)))
        ids = np.sort(g.integers(0, ndocs, size=n))
        if e == 0:
            ids = np.sort(np.concatenate([ids, g.permutation(ndocs)[: int(ndocs * hot_frac)]]))
        post[e] = (ids.astype(np.int64), val.rows(len(ids)))
    queries = []
    for _ in range(nq):
        q = {}
        for _ in range(ne):
            e = 0 if g.random() < 0.25 else int(g.integers(0, V))
            q.setdefault(e, []).append(_t(val.vec()))
        queries.append(q)
    if name is not None:
        cls = _Values(seed + 1, dc, values)
        _CLS[name] = (np.stack([cls.vec() for _ in range(nq)]), np.stack([cls.vec() for _ in range(ndocs)]))
    return Case(post, queries, ndocs, d, 0, ndocs, 2008, 8000 + d, f"Zipf layout, {ndocs} docs, {V} experts, {nq} x {ne} entries, d={d}")


# ---- the table ------------------------------------------------------------------------------------------------------------------------
TABLE = {}
for _nb in A_NB:
    TABLE[f"A-nb{_nb}"] = functools.partial(shape_a, _nb)
for _ne in B_COUNTS:
    TABLE[f"B-ne{_ne}"] = functools.partial(shape_b, _ne)
for _pc in C_RUNS:
    TABLE[f"C-pc{_pc}"] = functools.partial(shape_c, _pc)
for _b, _c in D_WINDOWS:
    for _w in (0, 1):
        TABLE[f"D-{_b}+{_c}-{'wide' if _w else 'tight'}"] = functools.partial(shape_d, _b, _c, _w)
for _d in E_D:
    TABLE[f"E-d{_d}"] = functools.partial(shape_e, _d)
for _dp, _ds in E_PQ:
    TABLE[f"E-pq{_dp}x{_ds}"] = functools.partial(shape_e_pq, _dp, _ds, name=f"E-pq{_dp}x{_ds}")
for _k in F_KINDS:
    TABLE[f"F-{_k}"] = functools.partial(shape_f, _k)
TABLE["G-zipf"] = functools.partial(shape_g, name="G-zipf")
NAMES = tuple(TABLE)
# the PQ engine: family E's PQ rows as they were born, and A, B, C, F, G re-encoded (sub-vector width by family)
PQ_DSUB = {"A": 2, "B": 4, "C": 8, "F": 2, "G": 4}
PQ_NAMES = tuple(n for n in NAMES if n.startswith("E-pq") or n[0] in PQ_DSUB)


class Loaded(NamedTuple):
    name: str
    case: Case
    S: np.ndarray  # [nq, corpus_len] fp64, the expert part
    m: np.ndarray  # [nq, corpus_len] entries with a posting for the doc


def check_exact(S, allow_inf=False):
    """The condition under which fp32 accumulation in any order is exact: every cell a multiple of 1/16 with 16 (|s| + 2) < 2^24."""
    fin = np.isfinite(S)
    assert not np.isnan(S).any() and (allow_inf or fin.all())
    assert not (S[~fin] < 0).any()
    s = S[fin]
    assert np.array_equal(np.round(s * 16), s * 16) and (16 * (np.abs(s) + 2) < 2 ** 24).all()
    return True


@functools.lru_cache(maxsize=None)
def load(name):
    case = TABLE[name]()
    assert 0 <= case.doc_begin and case.doc_begin + case.cols <= case.corpus_len and case.ld >= case.cols > 0
    assert max(sum(len(v) for v in q.values()) for q in case.queries) <= MAX_ENTRIES and (case.d + 31) // 32 * 32 <= 128
    for ids, rows in case.postings.values():
        assert (np.diff(ids) >= 0).all() and rows.shape == (len(ids), case.d) and rows.dtype == np.float32
        fin = rows[np.isfinite(rows)]
        assert np.array_equal(np.round(fin * 4), fin * 4) and (np.abs(fin) <= 2).all()
    for q in case.queries:
        for vecs in q.values():
            for u in vecs:
                fin = u.numpy()[np.isfinite(u.numpy())]
                assert np.array_equal(np.round(fin * 4), fin * 4) and (np.abs(fin) <= 2).all()
    S, _, m = O.score_matrix(case.postings, case.queries, case.corpus_len, bf16=True, return_abs=True)
    check_exact(S, allow_inf=name.startswith("F-"))
    return Loaded(name, case, S, m)


def cls_of(name):
    load(name)
    return _CLS[name]


def flat(case):
    """(expert int64 [P], doc int64 [P], rows fp32 [P, d]) in the order the case lists them: what IVFIndex takes."""
    es = sorted(case.postings)
    return (np.concatenate([np.full(len(case.postings[e][0]), e, dtype=np.int64) for e in es]),
            np.concatenate([case.postings[e][0] for e in es]).astype(np.int64), np.concatenate([case.postings[e][1] for e in es], 0))


def packed(case):
    """(post_doc int32 [P], rows fp32 [P, dp], exp_off int64 [V + 1]): the device layout of csrc/ivf.h, restated in numpy."""
    ex, docs, rows = flat(case)
    order = np.lexsort((np.arange(len(ex)), docs, ex))  # (expert, doc), listed order inside a doc
    dp = (case.d + 31) // 32 * 32
    out = np.zeros((len(ex), dp), dtype=np.float32)
    out[:, : case.d] = rows[order]
    off = np.concatenate([[0], np.cumsum(np.bincount(ex, minlength=int(ex.max()) + 1))]).astype(np.int64)
    return docs[order].astype(np.int32), out, off


def _bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy()


def pq_form(name):
    """(dsub, codebook fp32 [m, 256, dsub], post_code uint8 [P, m], post_doc int32 [P], exp_off int64 [V + 1]) of a case of PQ_NAMES,
    codes in packed order.  decode(post_code, codebook) equals the case's packed rows bit for bit as bf16 (asserted): family E's PQ
    rows with the codebook and codes they were made from, the others re-encoded -- per subspace the distinct sub-vectors (by bf16
    bit pattern, so a NaN or an inf is a centroid like any other) in order of first appearance, zeros behind them."""
    case = load(name).case
    post_doc, rows, off = packed(case)
    P, dp = rows.shape
    if name in _PQ_GIVEN:
        dsub, codebook, by_expert = _PQ_GIVEN[name]
        ex = flat(case)[0]
        order = np.lexsort((np.arange(len(ex)), flat(case)[1], ex))
        codes = np.concatenate([by_expert[e] for e in sorted(by_expert)], 0)[order]
    else:
        dsub = PQ_DSUB[name[0]]
        m = dp // dsub
        codebook, codes = np.zeros((m, 256, dsub), dtype=np.float32), np.zeros((P, m), dtype=np.uint8)
        bits = _bf16_bits(rows).reshape(P, m, dsub)
        for j in range(m):
            _, first, inv = np.unique(bits[:, j], axis=0, return_index=True, return_inverse=True)
            assert len(first) <= 256, (name, j, len(first))
            rank = np.argsort(np.argsort(first))  # order of first appearance
            codes[:, j] = rank[inv.reshape(-1)]
            codebook[j, rank] = rows.reshape(P, m, dsub)[first, j]
    m = dp // dsub
    dec = codebook[np.arange(m)[None, :], codes].reshape(P, dp)
    assert np.array_equal(_bf16_bits(dec), _bf16_bits(rows))
    return dsub, codebook, codes, post_doc, off


# ---- the window's prefill and what must stand in it afterwards -------------------------------------------------------------------------
# bit patterns sprinkled over the cells that must not change: -0.0, +0.0, NaNs of both signs with payloads, a signalling NaN, +-inf,
# the smallest subnormal, the largest finite value
PREFILL_BITS = (0x80000000, 0x00000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x00000001, 0x7F7FFFFF)


def window(loaded, S=None):
    """(prefill uint32 [nq, ld], expected uint32 [nq, ld], contributed bool [nq, ld]) of a case's window.  A cell the oracle gives a
    contribution (> 0) starts from a grid value in [-2, 2] and must end as prefill + oracle; every other word -- cells without a
    contribution and the ld - cols padding -- starts from an arbitrary bit pattern (PREFILL_BITS on about a third of them) and must
    come back unchanged.  `S`: another oracle matrix for the same case (the PQ engine's, over the decoded rows)."""
    case = loaded.case
    S = loaded.S if S is None else S
    nq = len(case.queries)
    g = np.random.default_rng(case.seed)
    win = np.zeros((nq, case.ld))
    win[:, : case.cols] = S[:, case.doc_begin:case.doc_begin + case.cols]
    contributed = win > 0
    pre = g.integers(0, 2 ** 32, size=(nq, case.ld), dtype=np.uint64).astype(np.uint32)
    pick = g.integers(0, 3 * len(PREFILL_BITS), size=(nq, case.ld))
    for j, b in enumerate(PREFILL_BITS):
        pre[pick == j] = np.uint32(b)
    start = (g.integers(-8, 9, size=(nq, case.ld)) / 4.0).astype(np.float32)
    pre[contributed] = start.view(np.uint32)[contributed]
    want = pre.copy()
    want[contributed] = (start.astype(np.float64) + win)[contributed].astype(np.float32).view(np.uint32)
    return pre, want, contributed
