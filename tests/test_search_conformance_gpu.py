"""The dense-search conformance table on the MI355X (tests/_search_cases.py; the CPU half is tests/test_search_conformance.py).

For every case, under the case's options: dprhot_search_plan reports the form and the steps the case is named after; dprhot_search,
driven through ctypes alone with values, indices and an exactly sized workspace between guard bands, leaves the oracle's state after
EVERY call, in every order of the shards, twice with the same bits; CorpusSearch on the same shards leaves it too; and dprhot_sim_fwd
under the same pinned form stores the oracle's score matrix.  The inputs are exact (quarter grid, see the case module), so every
comparison is bit for bit: values as int32, ids as int64, no tolerance.  Every input is valid; nothing here provokes a fault."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _search_cases as C  # noqa: E402

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


@pytest.fixture
def loaded(request):
    """The case with its options set in the library; the defaults are restored whatever the test does."""
    L = C.load(request.param)
    ctx = C.options(L.case)
    ctx.__enter__()
    try:
        yield L
    finally:
        ctx.__exit__(None, None, None)


def bare_search(case, Qb, Cb, order):
    """dprhot_search through ctypes alone, one call per shard of `order`: -> the state after every call."""
    from dpr_scale_amd import _lib

    nq, k = case.nq, case.k
    nws = _lib.search_workspace_bytes(nq, case.chunk)
    raws = []
    values = _banded(raws, nq * k * 4).view(torch.float32).view(nq, k)
    indices = _banded(raws, nq * k * 8).view(torch.int64).view(nq, k)
    ws = _banded(raws, nws)
    out = []
    for call, si in enumerate(case.orders[order]):
        _lib.check(_lib.lib.dprhot_search(_p(Qb), nq, _p(Cb[si]), Cb[si].shape[0], case.d, case.shards[si][0], k, case.chunk, _p(values),
                                          _p(indices), int(call == 0), _p(ws), nws, _stream()), "dprhot_search")
        _check_bands(raws)
        out.append((values.cpu().numpy(), indices.cpu().numpy()))
    return out


def _diff(got, want):
    """'' when the states are the same bits, else where they first differ."""
    gv, wv = got[0].view(np.int32), np.ascontiguousarray(want[0]).view(np.int32)
    bad = (gv != wv) | (got[1] != want[1])
    if not bad.any():
        return ""
    r, c = np.argwhere(bad)[0]
    return f"{int(bad.sum())} slots differ, first at row {r} slot {c}: got ({got[0][r, c]}, {got[1][r, c]}), want ({want[0][r, c]}, {want[1][r, c]})"


@pytest.mark.parametrize("loaded", C.NAMES, indirect=True)
def test_search_equals_the_oracle_in_the_form_it_is_named_after(loaded):
    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import CorpusSearch

    L, case = loaded, loaded.case
    C.check_plan(case)
    Qb = torch.from_numpy(case.Q).to(torch.bfloat16).to(DEV)
    Cb = [torch.from_numpy(Cs).to(torch.bfloat16).to(DEV) for _, Cs in case.shards]
    assert torch.equal(Qb.float().cpu().isnan(), torch.from_numpy(case.Q).isnan())
    for order, seq in case.orders.items():
        runs = [bare_search(case, Qb, Cb, order) for _ in range(2)]
        for call, want in enumerate(L.states[order]):
            for run in runs:
                d = _diff(run[call], want)
                assert not d, (case.name, case.note, order, call, d)
        # the public path on the same shards (fp32 in, cast on the device), after every add
        s = CorpusSearch(torch.from_numpy(case.Q).to(DEV), case.k, chunk=case.chunk)
        for call, si in enumerate(seq):
            s.add(torch.from_numpy(case.shards[si][1]).to(DEV), case.shards[si][0])
            v, i = s.result()
            d = _diff((v.cpu().numpy(), i.cpu().numpy()), L.states[order][call])
            assert not d, (case.name, "CorpusSearch", order, call, d)
    # dprhot_sim_fwd in the form of the head (asserted above): the oracle's scores, bit for bit (a NaN is a NaN)
    si = case.orders["inc"][0]
    _, cols, head, form = C.plan(case, "inc")[0][0]
    assert head and form == case.form
    raws = []
    S = _banded(raws, case.nq * cols * 4).view(torch.float32).view(case.nq, cols)
    _lib.check(_lib.lib.dprhot_sim_fwd(_p(Qb), case.nq, _p(Cb[si]), cols, case.d, None, 1.0, _p(S), _stream()), "dprhot_sim_fwd")
    _check_bands(raws)
    got, want = S.cpu().numpy(), np.ascontiguousarray(L.S[si][:, :cols])
    same = (got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (case.name, "sim_fwd", int((~same).sum()), np.argwhere(~same)[0].tolist())
