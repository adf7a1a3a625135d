"""The fused late-interaction expert score (csrc/maxsim.h) on the MI355X, bit for bit against the float64 oracle.

Inputs and the upstream gradient live on grids (tests/_multivec_oracle.py) on which every fp32 product and every fp32 partial sum of
the scores and of all four gradients is exact whatever the order of summation; `exact_certificate` proves it per case (and on the CPU
in tests/test_multivec_exact.py).  So nothing here has a tolerance: scores, dq, dc, dwq, dwc and the non-finite pattern are compared
with torch.equal against the oracle cast to fp32."""
import pytest
import torch

import _multivec_oracle as MO
from test_multivec_gpu import DEV, _run

pytestmark = pytest.mark.gpu
_ID = MO.case_id


def _reference(qr, cr, mask, pairwise, pool, dS):
    MO.exact_certificate(qr, cr, mask, pairwise, pool, dS)
    return MO.scores_and_grads(qr, cr, mask, pairwise, pool, dS)


def _check_scores(S, S0, mask, pairwise):
    MO.assert_exact("S", S, S0)  # (-inf where the oracle has it, nowhere else)
    if mask is not None and bool(mask.any()):
        mm = mask.view(S.shape[0], -1) if pairwise else mask.reshape(1, -1).expand(S.shape[0], -1)
        assert bool((S[mm] == float("-inf")).all()) and bool(torch.isfinite(S[~mm]).all())


def _check_grads(grads, g0, cr, mask):
    assert set(grads) == set(g0)
    for k, ref in g0.items():
        MO.assert_exact(k, grads[k], ref)
    zero = [int(m) for m in mask.nonzero().view(-1)]  # masked contexts, and all-padding ones where weights carry the padding
    if "expert_weights" in cr:
        zero.append(cr["expert_repr"].shape[0] - 1)
    for ctx in zero:
        for k in ("dc", "dwc"):
            if k in grads:
                assert torch.equal(grads[k][ctx], torch.zeros_like(grads[k][ctx])), (k, ctx)


def _exact(case):
    qr, cr, mask, pairwise, pool, dS = MO.build_case(case)
    S0, g0 = _reference(qr, cr, mask, pairwise, pool, dS)
    S, grads = _run(qr, cr, mask, pairwise, pool, dS)
    _check_scores(S, S0, mask, pairwise)
    _check_grads(grads, g0, cr, mask)
    return S, grads, g0


@pytest.mark.parametrize("case", MO.SWEEP, ids=_ID)
def test_tile_edges(case):
    _exact(case)


@pytest.mark.parametrize("case", MO.SLOTS, ids=_ID)
def test_slot_counts(case):
    """KQ = 1, 2, 4, 8 are the compiled slot counts; 3, 5 and 7 run the next larger text with its run-time break."""
    _, grads, _ = _exact(case)
    assert grads["dwq"].abs().sum() > 0 and grads["dwc"].abs().sum() > 0


@pytest.mark.parametrize("case", MO.IDS_ONLY, ids=_ID)
def test_ids_without_weights(case):
    """expert_ids and no expert_weights: the match indicator alone scales the score (ms_fwd_kernel<*, true, false>, backward alike)."""
    _, grads, _ = _exact(case)
    assert set(grads) == {"dq", "dc"}


# ---- the kernels object directly ----------------------------------------------------------------------------------------------------
def _direct_inputs(qr, cr, mask, ids=True):
    d = qr["expert_repr"].shape[-1]
    pad = (-d) % 32
    Qb = torch.nn.functional.pad(qr["expert_repr"], (0, pad)).to(DEV, torch.bfloat16).contiguous()
    Cb = torch.nn.functional.pad(cr["expert_repr"], (0, pad)).to(DEV, torch.bfloat16).contiguous()
    qi = ci = None
    if ids:
        qi, ci = (r["expert_ids"].to(DEV, torch.int32).contiguous() for r in (qr, cr))
    qw, cw = (r["expert_weights"].to(DEV).float().contiguous() for r in (qr, cr))
    return Qb, Cb, qi, ci, qw, cw, mask.to(DEV, torch.uint8).contiguous()


def _cpu(t):
    return None if t is None else t.cpu()


@pytest.mark.parametrize("case", MO.WEIGHTS_ONLY, ids=_ID)
def test_weights_without_ids(case):
    """Weights and no ids, which only the C ABI allows (ms_fwd_kernel<1, false, true>, ms_launch_bwd<false, true>): what the oracle
    computes when every slot carries the same expert id."""
    from dpr_scale_amd import hotpath

    kn = hotpath.default_kernels()
    qr, cr, mask, pairwise, pool, dS = MO.build_case(case)
    S0, g0 = _reference(qr, cr, mask, pairwise, pool, dS)
    d, M = case["d"], case["Nc"] // case["B"] if pairwise else 0
    Qb, Cb, _, _, qw, cw, m8 = _direct_inputs(qr, cr, mask, ids=False)
    S, state = kn.maxsim_fwd(Qb, Cb, None, None, qw, cw, 1, 1, hotpath._POOL[pool], M, m8)
    dq, dc, dwq, dwc = kn.maxsim_bwd(dS.to(DEV), Qb, Cb, None, None, qw, cw, 1, 1, hotpath._POOL[pool], M, m8, state, True, True, True)
    torch.cuda.synchronize()
    _check_scores(S.cpu(), S0, mask, pairwise)
    _check_grads({"dq": dq.cpu()[..., :d].contiguous(), "dc": dc.cpu()[..., :d].contiguous(), "dwq": dwq.cpu(), "dwc": dwc.cpu()},
                 g0, cr, mask)
    assert not bool(dq[..., d:].any()) and not bool(dc[..., d:].any())  # the zero padding's gradient


@pytest.fixture(scope="module")
def subset_case():
    from dpr_scale_amd import hotpath

    kn = hotpath.default_kernels()
    qr, cr, mask, pairwise, pool, dS = MO.build_case(MO.SUBSETS)
    _, g0 = _reference(qr, cr, mask, pairwise, pool, dS)
    Qb, Cb, qi, ci, qw, cw, m8 = _direct_inputs(qr, cr, mask)
    KQ, KD = MO.SUBSETS["KQ"], MO.SUBSETS["KD"]
    _, state = kn.maxsim_fwd(Qb, Cb, qi, ci, qw, cw, KQ, KD, 0, 0, m8)

    def bwd(need_dq, need_dc, need_dw):
        out = kn.maxsim_bwd(dS.to(DEV), Qb, Cb, qi, ci, qw, cw, KQ, KD, 0, 0, m8, state, need_dq, need_dc, need_dw)
        torch.cuda.synchronize()
        return dict(zip(MO.GRADS, (_cpu(t) for t in out)))

    return bwd, bwd(True, True, True), g0, MO.SUBSETS["d"]


@pytest.mark.parametrize("needs", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)])
def test_gradient_subsets(subset_case, needs):
    """The launches with dq == nullptr or dc == nullptr (grid y = 1, weight gradients only) and those without weight gradients."""
    bwd, full, g0, d = subset_case
    got = bwd(*map(bool, needs))
    asked = {"dq": needs[0], "dc": needs[1], "dwq": needs[2], "dwc": needs[2]}
    for k in MO.GRADS:
        if not asked[k]:
            assert got[k] is None, k
            continue
        assert torch.equal(got[k], full[k]), k
        MO.assert_exact(k, got[k][..., :d].contiguous() if k in ("dq", "dc") else got[k], g0[k])


@pytest.mark.parametrize("case", MO.TIES, ids=_ID)
def test_max_pool_ties_go_to_the_lowest_row_slot(case):
    """A query token repeated with its ids and weights: its row slots tie exactly under max pooling.  As torch.max does, the whole
    gradient goes to the first of them and none to the copy."""
    qr, cr, mask, pairwise, _, _ = MO.build_case(dict(case, variant=None))
    first = MO.tie_token(qr, cr, mask, pairwise)
    tok = first + 1  # where build_case puts the copy
    _, grads, g0 = _exact(case)
    assert bool(g0["dq"][0, first].any()), "the tied token never wins the pool: the case shows nothing"
    assert torch.equal(grads["dq"][0, tok], torch.zeros(case["d"]))
    if "dwq" in grads:
        assert torch.equal(grads["dwq"][0, tok], torch.zeros(case["KQ"]))
