"""The exact-gradient oracle of tests/_multivec_oracle.py, on the CPU: the explicit (gather + np.add.at) gradients equal autograd's in
float64, every case of the exact GPU tests passes the certificate that makes fp32 summation order irrelevant, and the comparison the
GPU tests use rejects gradients that are wrong by one ulp, by one gathered term, or by one raw entry of a neighbouring slot."""
import numpy as np
import pytest
import torch

import _multivec_oracle as MO

IDS = [MO.case_id(c) for c in MO.EXACT_CASES]


def test_grid_dS_is_on_its_grid():
    g = MO.grid_dS(3, (50, 70))
    assert g.dtype == torch.float32 and g.shape == (50, 70)
    assert torch.equal(g * 8, (g * 8).round()) and g.abs().max() == 2.0 and g.min() == -2.0
    assert torch.equal(g, MO.grid_dS(3, (50, 70))) and not torch.equal(g, MO.grid_dS(4, (50, 70)))


def test_sweep_covers_the_tile_edges():
    S = MO.SWEEP
    assert 15 <= len(S) <= 20
    assert {1, 63, 64, 65} <= {c["LQ"] for c in S} and {1, 63, 64, 65, 129} <= {c["LD"] for c in S}
    assert {32, 40, 256, 288, 768} <= {c["d"] for c in S}
    assert {1, 8, 9, 63, 64, 65, 130} <= {c["Nc"] // c["B"] if c["pairwise"] else c["Nc"] for c in S}
    slots = {c["LQ"] * c["KQ"] * (1 if c["pairwise"] else c["B"]) for c in S}  # row slots one dc workgroup sweeps
    assert {63, 64, 65, 127, 128, 129} <= slots
    assert {(c["pairwise"], c["pool"]) for c in S} == set(MO.MODES)
    for c in S:  # one masked and one all-padding context in every case
        _, cr, mask, *_ = MO.build_case(c)
        assert int(mask.sum()) == 1 and not bool(mask[-1]) and not bool(cr["expert_repr"][-1].any())


@pytest.mark.parametrize("case", MO.EXACT_CASES, ids=IDS)
def test_explicit_grads_equal_autograd(case):
    """Every shape of the GPU tests, both pools, in-batch and (where the contexts divide among the queries) pairwise."""
    for pairwise, pool in MO.MODES:
        if pairwise and case["Nc"] % case["B"]:
            continue
        qr, cr, mask, pairwise, pool, dS = MO.build_case(case, pairwise, pool)
        _, ref = MO.scores_and_grads(qr, cr, mask, pairwise, pool, dS)
        got, abs_sums, gran = MO.explicit_grads(qr, cr, mask, pairwise, pool, dS)
        assert set(got) == set(ref)
        for k in ref:
            assert torch.equal(got[k], ref[k]), (k, pairwise, pool)
            assert bool((abs_sums[k] >= got[k].abs()).all())
            if gran[k] != 1.0:
                assert torch.equal(got[k] / gran[k], (got[k] / gran[k]).round())


@pytest.mark.parametrize("case", MO.EXACT_CASES, ids=IDS)
def test_certificate_holds(case):
    qr, cr, mask, pairwise, pool, dS = MO.build_case(case)
    room = MO.exact_certificate(qr, cr, mask, pairwise, pool, dS)
    assert all(v < 2.0**24 for v in room.values())
    _, ref = MO.scores_and_grads(qr, cr, mask, pairwise, pool, dS)
    assert sum(float(g.abs().sum()) for g in ref.values()) > 0  # the case does carry gradient
    assert bool((ref["dc"][mask] == 0).all())  # masked contexts take no gradient
    if "expert_weights" in cr:  # nor do all-padding ones, whose weights are 0 (without weights their token 0 wins the all-zero tie)
        assert bool((ref["dc"][-1] == 0).all())


def test_granularities_on_the_grid():
    qr, cr, mask, pairwise, pool, dS = MO.build_case(MO.SWEEP[1])
    _, _, gran = MO.explicit_grads(qr, cr, mask, pairwise, pool, dS)
    assert gran["dq"] >= 2.0**-11 and gran["dc"] >= 2.0**-11 and gran["dwq"] >= 2.0**-10 and gran["dwc"] >= 2.0**-10
    assert MO._granularity(np.array([0.75, -2.0, 0.0, 3 * 2.0**-11])) == 2.0**-11


def test_certificate_rejects_inputs_off_the_grid():
    qr, cr, mask, pairwise, pool, dS = MO.build_case(MO.SWEEP[1])
    MO.exact_certificate(qr, cr, mask, pairwise, pool, dS)
    with pytest.raises(AssertionError):
        MO.exact_certificate(qr, cr, mask, pairwise, pool, dS + 2.0**-20)
    qg, cg, mg = MO.make_inputs(5, "citadel", B=2, LQ=9, Nc=4, LD=12, d=64, KQ=2, KD=2, grid=False)
    with pytest.raises(AssertionError):
        MO.exact_certificate(qg, cg, mg, False, "sum", MO.grid_dS(0, (2, 4)))


# ---- sensitivity: the comparison of the GPU tests must reject a subtly wrong kernel ----------------------------------------------
SENS = [MO.SWEEP[1], MO.SWEEP[4], MO.SLOTS[5]]  # CITADEL, sum and max


@pytest.fixture(scope="module", params=SENS, ids=[MO.case_id(c) for c in SENS])
def sens(request):
    qr, cr, mask, pairwise, pool, dS = MO.build_case(request.param)
    _, ref = MO.scores_and_grads(qr, cr, mask, pairwise, pool, dS)
    return qr, cr, MO.gather_terms(qr, cr, mask, pairwise, pool, dS), ref


def test_accepts_the_oracle_itself(sens):
    _, _, _, ref = sens
    for k in MO.GRADS:
        MO.assert_exact(k, ref[k].float(), ref[k])


@pytest.mark.parametrize("k", MO.GRADS)
@pytest.mark.parametrize("which", ["largest", "smallest"])
def test_rejects_one_ulp(sens, k, which):
    _, _, _, ref = sens
    got = ref[k].float().clone().view(-1)
    mag = got.abs()
    e = int(mag.argmax()) if which == "largest" else int(torch.where(mag > 0, mag, torch.inf).argmin())
    got[e] = torch.nextafter(got[e], torch.tensor(float("inf")))
    with pytest.raises(AssertionError, match="1 of"):
        MO.assert_exact(k, got.view(ref[k].shape), ref[k])


def _live(t):
    return np.argwhere((t["gr"] * t["match"] * t["wq"] * t["wc"]) != 0)


@pytest.mark.parametrize("pick", ["first", "last", "smallest"])
def test_rejects_a_dropped_term(sens, pick):
    """One (row slot, y) term left out of the gather: the smallest one included (a small weight behind large neighbours)."""
    qr, cr, t, ref = sens
    live = _live(t)
    if pick == "smallest":
        mags = np.abs(t["gr"] * t["wq"] * t["wc"])[tuple(live.T)]
        at = tuple(live[int(mags.argmin())])
    else:
        at = tuple(live[0 if pick == "first" else -1])
    t2 = dict(t, gr=t["gr"].copy())
    t2["gr"][at] = 0.0
    got, _, _ = MO.accumulate_terms(qr, cr, t2)
    for k in ("dq", "dc"):  # (the term's feature row may be all zero only for a padding token, which carries no weight)
        with pytest.raises(AssertionError, match="differ"):
            MO.assert_exact(k, got[k].float(), ref[k])


def test_rejects_the_neighbouring_slots_raw(sens):
    """dwq of one row slot computed with the raw dot products of row slot + 1 (an off-by-one into the raw table)."""
    qr, cr, t, ref = sens
    live = _live(t)
    for b, rs, _ in live:
        nb = rs + 1 if rs + 1 < t["raw"].shape[1] else rs - 1
        sel = (t["gr"][b, rs] * t["match"][b, rs] * t["wc"][b, rs]) != 0
        if np.any(t["raw"][b, rs][sel] != t["raw"][b, nb][sel]):
            break
    else:
        raise AssertionError("no row slot whose neighbour's raw differs: the case cannot show this fault")
    raw = t["raw"].copy()
    raw[b, rs] = t["raw"][b, nb]
    got, _, _ = MO.accumulate_terms(qr, cr, dict(t, raw=raw))
    assert torch.equal(got["dq"], ref["dq"]) and torch.equal(got["dc"], ref["dc"])  # raw reaches the weight gradients only
    with pytest.raises(AssertionError, match="differ"):
        MO.assert_exact("dwq", got["dwq"].float().reshape(ref["dwq"].shape), ref["dwq"])
    # and by the old bar (1e-3 of the tensor's maximum) the same fault may pass: the reason for the exact comparison
    err = (got["dwq"].reshape(ref["dwq"].shape) - ref["dwq"]).abs().max()
    assert err > 0
