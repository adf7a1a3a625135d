"""The score-only MaxSim launch (hotpath.expert_score_only / rerank_score, csrc/maxsim.h ms_score_kernel) and the rerank tasks on the
MI355X: the same bits as the training forward's pairwise scores at every wave-split regime, exact against the float64 oracle and the
reference's golden files on grid inputs, NaN as torch.max, deterministic, and inside its buffers."""
import ctypes

import pytest
import torch

import _multivec_oracle as MO
from test_rerank import MULTIVEC_CASES, check_files, load_case, make_rerank_task, run_task

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _to(r):
    return {k: (v.float() if v.is_floating_point() else v).to(DEV) for k, v in r.items()}


def _same_bits(a, b):
    nan = torch.isnan(b)
    assert torch.equal(torch.isnan(a), nan)
    assert torch.equal(a.masked_fill(nan, 0.0), b.masked_fill(nan, 0.0))
    assert torch.equal(a.masked_fill(nan, 0.0).view(torch.int32), b.masked_fill(nan, 0.0).view(torch.int32))  # the sign of a zero too


# (kind, B, LQ, LD, d, KQ, KD, M, pool, grid, masked): every wave-split regime (LQ <= 16: four column groups, <= 32: two, one wave
# per row fragment from 33; the tile loop from 65), LD around the 64-token chunk and the groups' strides, every KQT text.
IDENTITY = [
    ("colbert", 4, 1, 1, 32, 1, 1, 1, "sum", True, False),
    ("citadel", 5, 9, 21, 40, 2, 3, 1, "sum", True, True),
    ("citadel", 3, 16, 63, 32, 8, 5, 3, "max", False, True),
    ("coil", 3, 17, 64, 40, 1, 1, 3, "sum", True, True),
    ("citadel", 3, 32, 181, 32, 1, 8, 1, "max", True, True),
    ("citadel", 3, 33, 181, 32, 2, 3, 1, "max", False, True),
    ("colbert", 2, 49, 65, 128, 1, 1, 3, "max", False, True),
    ("citadel", 2, 64, 511, 32, 2, 3, 1, "sum", False, True),
    ("citadel", 2, 65, 65, 128, 8, 5, 1, "sum", True, False),
    ("coil", 2, 130, 21, 40, 1, 1, 3, "max", False, True),
    ("citadel", 3, 32, 511, 128, 1, 1, 3, "sum", False, True),
    ("citadel", 4, 9, 181, 40, 1, 8, 3, "sum", False, True),
    ("citadel", 2, 130, 63, 32, 2, 3, 1, "max", True, True),
    ("colbert", 5, 32, 181, 128, 1, 1, 1, "sum", False, False),
]


@pytest.mark.parametrize("case", IDENTITY, ids=lambda c: "{}-B{}-LQ{}-LD{}-d{}-K{}x{}-M{}-{}-{}".format(*c[:9], "grid" if c[9] else "gauss"))
def test_same_bits_as_the_training_forward(case):
    from dpr_scale_amd import hotpath

    kind, B, LQ, LD, d, KQ, KD, M, pool, grid, masked = case
    Nc = B * M
    qr, cr, mask = MO.make_inputs(LQ * 7 + LD + KQ, kind, B=B, LQ=LQ, Nc=Nc, LD=LD, d=d, KQ=KQ, KD=KD, n_experts=12, grid=grid,
                                  masked=(1,) if masked else (), all_pad=(Nc - 1,))
    gq, gc, gm = _to(qr), _to(cr), mask.to(DEV) if masked else None
    with torch.no_grad():
        got = hotpath.expert_score_only(gq, gc, gm, pool)
        want = hotpath.expert_sim_score(gq, gc, gm, True, pool)
    assert got.shape == (B, M) and got.grad_fn is None
    _same_bits(got.cpu(), want.cpu())
    if masked:
        assert bool(torch.isinf(got.reshape(-1)[1])) and int(torch.isinf(got).sum()) == 1


ORACLE_KINDS = [("colbert", 1, 1), ("coil", 1, 1), ("citadel", 1, 1), ("citadel", 2, 3), ("citadel", 8, 5)]


@pytest.mark.parametrize("B,LQ,LD,d", [(5, 9, 21, 40), (3, 33, 181, 32), (2, 65, 130, 128), (4, 1, 1, 32)])
def test_exact_against_the_fp64_oracle_on_grid_inputs(B, LQ, LD, d):
    from dpr_scale_amd import hotpath

    for kind, KQ, KD in ORACLE_KINDS:
        qr, cr, _ = MO.make_inputs(B + LQ + LD + KQ, kind, B=B, LQ=LQ, Nc=B, LD=LD, d=d, KQ=KQ, KD=KD, n_experts=12)
        gq, gc = _to(qr), _to(cr)
        for pool in ("sum", "max"):
            S = hotpath.expert_score_only(gq, gc, None, pool).cpu()
            MO.assert_exact(f"{kind} {KQ}x{KD} {pool}", S, MO.expert_sim_score(qr, cr, None, True, pool))


def test_gaussian_inputs_within_accumulation_error():
    from dpr_scale_amd import hotpath

    for kind, KQ, KD, LQ, LD, M in (("citadel", 2, 2, 17, 45, 3), ("colbert", 1, 1, 32, 181, 1), ("citadel", 1, 5, 70, 130, 2)):
        qr, cr, mask = MO.make_inputs(5, kind, B=3, LQ=LQ, Nc=3 * M, LD=LD, d=128, KQ=KQ, KD=KD, grid=False, masked=(1,))
        for pool in ("sum", "max"):
            S = hotpath.expert_score_only(_to(qr), _to(cr), mask.to(DEV), pool).cpu()
            S0 = MO.expert_sim_score(qr, cr, mask, True, pool)
            fin = torch.isfinite(S0)
            assert torch.equal(torch.isfinite(S), fin) and torch.all(S[~fin] == float("-inf"))
            err = (S[fin].double() - S0[fin]).abs().max().item()
            assert err <= 1e-4 * max(S0[fin].abs().max().item(), 1.0), (kind, pool, err)


@pytest.mark.parametrize("name", MULTIVEC_CASES)
def test_golden_scores_bit_for_bit(name):
    from dpr_scale_amd import hotpath

    meta, qr, cr, z = load_case(name)
    S = hotpath.rerank_score(_to(qr), _to(cr), meta["pool"])
    assert S.shape == (meta["B"],)
    MO.assert_exact(name, S.cpu(), torch.from_numpy(z["scores"]).double())


def test_golden_dense_scores_bit_for_bit():
    from dpr_scale_amd import hotpath

    _, _, _, z = load_case("rerank_dense")
    S = hotpath.pairwise_score(torch.from_numpy(z["q"]).to(DEV), torch.from_numpy(z["c"]).to(DEV))[:, 0]
    MO.assert_exact("dense", S.cpu(), torch.from_numpy(z["scores"]).double())


@pytest.mark.parametrize("kind,KQ,KD", [("colbert", 1, 1), ("coil", 1, 1), ("citadel", 2, 3)])
@pytest.mark.parametrize("pool", ["sum", "max"])
def test_nan_tokens_give_nan_scores_as_the_oracle(kind, KQ, KD, pool):
    from dpr_scale_amd import hotpath

    B, M, LQ, LD, d = 3, 2, 6, 70, 32  # (LD > 64: the NaN token sits in the second column group's chunk)
    qr, cr, mask = MO.make_inputs(77, kind, B=B, LQ=LQ, Nc=B * M, LD=LD, d=d, KQ=KQ, KD=KD, masked=(2,))
    qr["expert_repr"][2, :] = float("nan")       # every token of query 2
    cr["expert_repr"][1, 66, 0] = float("nan")   # one token of passage 1 (query 0's second candidate)
    S0 = MO.expert_sim_score(qr, cr, mask, True, pool)
    S = hotpath.expert_score_only(_to(qr), _to(cr), mask.to(DEV), pool).cpu().double()
    assert torch.equal(torch.isnan(S), torch.isnan(S0)) and bool(torch.isnan(S0).any()) and not bool(torch.isnan(S0).all())
    ok = ~torch.isnan(S0)
    assert torch.equal(S[ok], S0[ok]) and S[1, 0] == float("-inf")  # (the masked candidate is -inf, NaN query or not)


def test_two_runs_are_bit_identical():
    from dpr_scale_amd import hotpath

    qr, cr, mask = MO.make_inputs(23, "citadel", B=4, LQ=20, Nc=12, LD=70, d=96, KQ=2, KD=3, grid=False, masked=(3,))
    gq, gc, gm = _to(qr), _to(cr), mask.to(DEV)
    a = hotpath.expert_score_only(gq, gc, gm, "sum")
    b = hotpath.expert_score_only(gq, gc, gm, "sum")
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


@pytest.mark.parametrize("LQ,LD", [(13, 83), (32, 181), (37, 83), (70, 65)])
def test_calls_stay_inside_their_buffers(LQ, LD):
    """S and every input sit between guard bands of a fixed pattern; the launch leaves the bands untouched."""
    from dpr_scale_amd import _lib

    lib = _lib.lib
    B, M, dp, KQ, KD = 3, 2, 64, 2, 3
    Nc = B * M
    G = 4096
    qr, cr, mask = MO.make_inputs(9, "citadel", B=B, LQ=LQ, Nc=Nc, LD=LD, d=dp, KQ=KQ, KD=KD, masked=(5,))
    bufs = []

    def guarded(nbytes):
        t = torch.full((nbytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
        bufs.append((t, nbytes))
        return t[G:G + nbytes]

    def put(src):
        src = src.contiguous()
        dst = guarded(src.numel() * src.element_size())
        dst.copy_(src.view(-1).view(torch.uint8).to(DEV))
        return dst

    Qb, Cb = put(qr["expert_repr"].to(torch.bfloat16)), put(cr["expert_repr"].to(torch.bfloat16))
    qi, ci = put(qr["expert_ids"].to(torch.int32)), put(cr["expert_ids"].to(torch.int32))
    qw, cw = put(qr["expert_weights"].float()), put(cr["expert_weights"].float())
    m8 = put(mask.to(torch.uint8))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for pool in (0, 1):
        S = guarded(B * M * 4)
        _lib.check(lib.dprhot_maxsim_score(p(Qb), p(Cb), B, LQ, Nc, LD, dp, p(qi), p(ci), p(qw), p(cw), KQ, KD, pool, M, p(m8), p(S), st))
        outs.append(S)
    torch.cuda.synchronize()
    for t, n in bufs:
        h = t.cpu()
        assert bool((h[:G] == 0xA5).all()) and bool((h[G + n:] == 0xA5).all()), f"guard band of a {n}-byte buffer overwritten"
    for pool, S in zip(("sum", "max"), outs):  # and every element of S was written, with the right value
        MO.assert_exact(pool, S.cpu().view(torch.float32).view(B, M), MO.expert_sim_score(qr, cr, mask, True, pool))


def test_multivec_task_end_to_end_on_gpu(tmp_path):
    from dpr_scale_amd.task.rerank import RerankMultiVecRetrieverTask

    for i, name in enumerate(("rerank_citadel23_sum_cls", "rerank_colbert_max")):
        meta, qr, cr, z = load_case(name)
        task = make_rerank_task(RerankMultiVecRetrieverTask, str(tmp_path / str(i)), None, query_pool=meta["pool"]).to(DEV)
        outs, files = run_task(task, qr, cr, meta, DEV)
        check_files(task, outs, files, meta, z)


def test_dense_task_end_to_end_on_gpu(tmp_path):
    from dpr_scale_amd.task.rerank import RerankDenseRetrieverTask

    meta, _, _, z = load_case("rerank_dense")
    task = make_rerank_task(RerankDenseRetrieverTask, str(tmp_path / "out"), None).to(DEV)
    outs, files = run_task(task, torch.from_numpy(z["q"]), torch.from_numpy(z["c"]), meta, DEV)
    check_files(task, outs, files, meta, z)
