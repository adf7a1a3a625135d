"""The dense-search conformance table on the CPU (tests/_search_cases.py; the GPU half is tests/test_search_conformance_gpu.py).

  1. The oracle's score part is pinned against a triple Python loop; the loader's exactness assertion holds for every case, and the
     table holds the shapes it names.
  2. CorpusSearch on the stand-in kernels (tests/_oracle_kernels.py) equals the oracle on every case.
  3. `model` restates the filter-then-merge CONTRACT of dprhot_search in numpy -- threshold = the state's k-th entry; a score is taken
     when v > tv, or v == tv and its id is lower or the slot is unfilled; at most `cols` candidates per row; candidates merged in the
     total order -- with a `defect=` switch.  The faithful model must equal the oracle's fold on every case (and leave the candidate
     counts the designed cases write down); every defect of DEFECTS must fail at least one case, and the test prints which.
  4. dprhot_search_plan (host code only: the library loads without a device) reports the expected forms and steps for every case
     under the case's options."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _search_cases as C  # noqa: E402
from _oracle_kernels import OracleKernels  # noqa: E402
from _topk_oracle import fold  # noqa: E402

DEFECTS = {
    "strict_compare": "v > tv only: exact ties with the k-th best are dropped",
    "ties_regardless_of_id": "v >= tv: a tie is taken whatever its id",
    "threshold_slot_0": "the threshold read from slot 0 of the state",
    "id_offset_ignored": "the tie rule compares the shard-local column with the state's id",
    "ragged_8_dropped": "the last 8 columns of a chunk that is no multiple of 16 are not filtered",
    "nan_admitted": "a NaN score is appended",
    "list_cut_at_nsort": "a candidate list longer than TK_NSORT is cut there",
    "stale_row_thresholds": "a persistent workgroup filters its second tile against the row thresholds of its first",
}
_I64MAX = np.iinfo(np.int64).max


def tile_of(wg, nbx, nby):
    """g2_tile_of (csrc/gemm256.h): the (bx, by) of tile number `wg` -- XCD-major, row blocks fastest inside groups of 8."""
    nwg = nbx * nby
    xcd, q, r = wg & 7, nwg >> 3, nwg & 7
    t = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (wg >> 3)
    grp, inside = divmod(t, 8 * nbx)
    rows = min(8, nby - grp * 8)
    return inside // rows, grp * 8 + inside % rows


def _merge(v0, i0, cv, ci, k):
    """One row: filled state entries + candidates in the total order (a NaN candidate, which only a defect admits, sorts first)."""
    keep = i0 >= 0
    v, i = np.concatenate([v0[keep], cv]), np.concatenate([i0[keep], ci])
    key = np.where(np.isnan(v), -np.inf, -v.astype(np.float64))
    o = np.lexsort((i, key))[:k]
    out_v, out_i = np.full(k, -np.inf, np.float32), np.full(k, -1, np.int64)
    out_v[:len(o)], out_i[:len(o)] = v[o], i[o]
    return out_v, out_i


def model(L, order, defect=None):
    """-> (per call: state after it, per call: per step None or [nq] candidate counts)."""
    assert defect is None or defect in DEFECTS
    case = L.case
    k, nq = case.k, case.nq
    st, states, counts = None, [], []
    for call, si in zip(C.plan(case, order), case.orders[order]):
        off, S = case.shards[si][0], L.S[si]
        per_step = []
        for j0, cols, head, form in call:
            piece = S[:, j0:j0 + cols]
            if head:
                st = fold(None, piece, off + j0, k)
                per_step.append(None)
                continue
            slot = 0 if defect == "threshold_slot_0" else k - 1
            tv_rows = st[0][:, slot].copy()
            ti = st[1][:, slot]
            ids = off + j0 + np.arange(cols, dtype=np.int64)
            cmp_ids = np.arange(cols, dtype=np.int64) if defect == "id_offset_ignored" else ids
            tv = np.repeat(tv_rows[:, None], cols, axis=1)
            if defect == "stale_row_thresholds" and form in (C.FORM_BIG, C.FORM_8P):
                nbx, nby = -(-cols // 256), -(-nq // 256)
                for t in range(C.NUM_WG, nbx * nby):
                    (bx, by), (_, by1) = tile_of(t, nbx, nby), tile_of(t - C.NUM_WG, nbx, nby)
                    m = np.arange(by * 256, min(by * 256 + 256, nq))
                    tv[m, bx * 256:bx * 256 + 256] = tv_rows[np.minimum(m - by * 256 + by1 * 256, nq - 1)][:, None]
            with np.errstate(invalid="ignore"):
                tie = piece == tv
                if defect == "strict_compare":
                    tie = np.zeros_like(tie)
                elif defect != "ties_regardless_of_id":
                    tie &= (ti < 0)[:, None] | (cmp_ids[None, :] < ti[:, None])
                take = (piece > tv) | tie
            if defect == "nan_admitted":
                take |= np.isnan(piece)
            if defect == "ragged_8_dropped" and cols % 16:
                take[:, cols - 8:] = False
            cnt = take.sum(axis=1)
            assert cnt.max() <= cols  # the workspace holds `cols` candidates per row
            nv, ni = st[0].copy(), st[1].copy()
            for r in np.nonzero(cnt)[0]:
                j = np.nonzero(take[r])[0]
                if defect == "list_cut_at_nsort":
                    j = j[:C.TK_NSORT[k > 256]]
                nv[r], ni[r] = _merge(st[0][r], st[1][r], piece[r, j], ids[j], k)
            st = (nv, ni)
            per_step.append(cnt)
        states.append(st)
        counts.append(per_step)
    return states, counts


def _same(a, b):
    return np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


def _agrees(L, defect=None):
    case = L.case
    for order in case.orders:
        states, counts = model(L, order, defect)
        if not all(_same(a, b) for a, b in zip(states, L.states[order])):
            return False
        for got, want in zip(counts, case.counts.get(order, [])):
            if not all(w is None or np.array_equal(g, w) for g, w in zip(got, want)):
                return False
    return True


# ---- 1. the oracle and the table -------------------------------------------------------------------------------------------------
def test_oracle_scores_equal_the_triple_loop():
    rng = np.random.default_rng(5)
    Q, Cm = C._grid(rng, 3, 16), C._grid(rng, 7, 16)
    S = C.scores(Q, Cm)
    for n in range(3):
        for j in range(7):
            acc = 0.0
            for a, b in zip(Q[n].tolist(), Cm[j].tolist()):
                acc += a * b
            assert S[n, j] == acc
    st = fold(fold(None, S[:, :4], 10, 3), S[:, 4:], 14, 3)
    for n in range(3):
        best = sorted(range(7), key=lambda j: (-S[n, j], j))[:3]
        assert st[1][n].tolist() == [10 + j for j in best] and st[0][n].tolist() == [S[n, j] for j in best]


def test_the_table_holds_the_shapes_it_names():
    fam = lambda f: [n for n in C.NAMES if n.startswith(f)]
    assert [len(fam(f)) for f in "TBSDN"] == [65, 13, 3, 7, 4] and len(C.NAMES) == 92
    assert C.expected_steps(262152, 262144, True) == [65536, 65536, 131072, 8] and C.expected_steps(262152, 262144, False) == [262144, 8]
    assert C.expected_steps(600, 264, True) == [264, 264, 72] and C.expected_steps(40, 8, True) == [8] * 5
    assert [cols for _, cols, _, _ in C.plan(C.load("S-default-chunk").case, "inc")[0]] == [65536, 65536, 131072, 8]
    forms = {}
    for name in C.NAMES:  # (building a case is cheap; only `load` scores it)
        case = C._BUILDERS[name]()
        forms.setdefault(case.form, []).append(name)
        assert "dec" in case.orders or name in C.LARGE or name.startswith("D-cnt"), name
        if name[0] in "TB" and not name.endswith("258tiles"):
            bn = C.TILES[int(name[1])][1] if name[0] == "T" else 256
            assert case.chunk % bn == 8 and (case.shards[1][0], case.shards[1][1].shape[0]) == (1000 + 2 * case.chunk, case.chunk + 8)
    assert sorted(forms) == list(range(9)) and all(any("dec" in C._BUILDERS[n]().orders for n in v) for v in forms.values())
    for name in fam("B"):
        case = C._BUILDERS[name]()
        tiles = [-(-case.nq // 256) * -(-cols // 256) for call in C.plan(case, "inc") for _, cols, head, _ in call if not head]
        assert (max(tiles) == 258) == name.endswith("258tiles") and max(tiles) in (2, 4, 258)
    # 640 x 21768: the second tile of a workgroup lies in row block 2 (128 rows, whole column tiles), its first in row block 0; 129 x 65800
    # has one row block
    assert [tile_of(t, 86, 3) for t in (0, 1, 256, 257)] == [(0, 0), (11, 0), (10, 2), (21, 2)]
    assert sorted(tile_of(t, 86, 3) for t in range(258)) == sorted((bx, by) for bx in range(86) for by in range(3))
    # the state is partly unfilled when filtering starts; -inf scores are selected over unfilled slots
    L = C.load("S-chunk8-k20")
    assert (fold(None, L.S[0][:, :8], 0, 20)[1][:, -1] == -1).all()
    L = C.load("N-inf")
    v, i = L.states["inc"][-1]
    assert np.isposinf(v).any() and (np.isneginf(v) & (i >= 0)).any() and not np.isnan(v).any()
    v, i = C.load("N-nan-query-row").states["dec"][-1]
    assert (i[1] == -1).all() and np.isneginf(v[1]).all() and (i[0] >= 0).all()
    v, i = C.load("N-nan-few-left").states["inc"][-1]
    assert (i[:, :18] >= 0).all() and (i[:, 18:] == -1).all()
    assert (1 << 33) < C.load("S-three-shards").states["inc"][-1][1].min()
    # a few levels: the k-th score of every row ties with scores that stay outside; the designed counts are what the model must leave
    L = C.load("D-levels")
    assert all(((np.concatenate(L.S, axis=1)[r] == L.states["inc"][-1][0][r, -1]).sum() > 20) for r in range(L.case.nq))
    case = C.load("D-cnt-k256").case
    assert case.counts["inc"][0][1].tolist() == [0, 1, 255, 256, 257] and C.TK_NSORT[False] == 256 and C.TK_NSORT[True] == 2048


@pytest.mark.parametrize("name", C.NAMES)
def test_inputs_are_exact_and_stand_in_search_equals_the_oracle(name):
    from dpr_scale_amd.hotpath import CorpusSearch

    L = C.load(name)  # (asserts the exactness rule)
    case = L.case
    for order, seq in case.orders.items():
        s = CorpusSearch(torch.from_numpy(case.Q), case.k, chunk=case.chunk, kernels=OracleKernels())
        for call, si in enumerate(seq):
            with np.errstate(invalid="ignore"):
                s.add(torch.from_numpy(case.shards[si][1]), case.shards[si][0])
            v, i = s.result()
            assert _same((v.numpy(), i.numpy()), L.states[order][call]), (name, order, call)


# ---- 2. the model of the contract and its defects ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verdicts():
    """name -> {None or defect: the model agrees with the oracle} -- one pass over the table, each case loaded once."""
    out = {}
    for name in C.NAMES:
        L = C.load(name)
        out[name] = {dfc: _agrees(L, dfc) for dfc in (None, *DEFECTS)}
    return out


def test_faithful_model_equals_the_oracle(verdicts):
    bad = [n for n in C.NAMES if not verdicts[n][None]]
    assert not bad, bad


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_defect_is_killed_by_the_table(defect, verdicts):
    killers = [n for n in C.NAMES if not verdicts[n][defect]]
    print(f"[search-defect] {defect} ({DEFECTS[defect]}): killed by {len(killers)} of {len(C.NAMES)} cases: {' '.join(killers)}")
    assert killers, defect
    if defect == "strict_compare":  # the id compare of the filter decides the state in every form's decreasing run
        assert not [n for n in C.NAMES if n[0] in "TB" and not n.endswith("258tiles") and n not in killers]


# ---- 3. the plan query ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_plan_query_reports_the_expected_forms_and_steps(name):
    from dpr_scale_amd import _lib

    case = C._BUILDERS[name]()
    before = {o: _lib.get_option(o) for o in case.options}
    with C.options(case):
        C.check_plan(case)
    assert {o: _lib.get_option(o) for o in case.options} == before


def test_plan_query_refusals_and_capacity():
    import ctypes

    from dpr_scale_amd import _lib

    lib, n = _lib.lib, ctypes.c_int(-7)
    buf = (ctypes.c_int64 * 16)()
    assert lib.dprhot_search_plan(8, 262152, 64, 20, 262144, 1, buf, 4, ctypes.byref(n)) == 0 and n.value == 4
    assert list(buf) == [0, 65536, 1, 3, 65536, 65536, 0, 3, 131072, 131072, 0, 3, 262144, 8, 0, 3]
    buf2 = (ctypes.c_int64 * 16)(*([-1] * 16))
    assert lib.dprhot_search_plan(8, 262152, 64, 20, 262144, 1, buf2, 3, ctypes.byref(n)) == -1 and n.value == 4
    assert b"capacity" in lib.dprhot_last_error() and list(buf2[:12]) == list(buf[:12]) and list(buf2[12:]) == [-1] * 4
    assert lib.dprhot_search_plan(8, 262152, 64, 20, 262144, 0, None, 0, ctypes.byref(n)) == -1 and n.value == 2
    # the default plan: 256 tiles of 256 x 256 take the large-shape kernels, the phase-interleaved one where d % 128 == 0
    assert [s[3] for s in _lib.search_plan(512, 65536, 128, 50, 32768, True)] == [7, 7]
    assert [s[3] for s in _lib.search_plan(512, 65536, 192, 50, 32768, True)] == [6, 6]
    assert _lib.search_plan(512, 32760, 128, 50, 32760, False) == [(0, 32760, False, 7)]
    assert _lib.search_plan(512, 32512, 128, 50, 32512, False)[0][3] == 8  # 254 tiles: below big_min, tile 0 on LDS-DMA by the plan
