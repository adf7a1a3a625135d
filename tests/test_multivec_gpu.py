"""The fused late-interaction expert score (hotpath.expert_sim_score, csrc/maxsim.h) on the MI355X against the float64 restatement of
dpr_scale/task/citadel_task.py:155-238 in tests/_multivec_oracle.py.  On the oracle's grid inputs every score and every maximum is
exact in fp32, so scores and argmax must agree exactly (ties to the lowest index); gradients within 1e-3 of max |grad|."""
import ctypes

import numpy as np
import pytest
import torch

import _multivec_oracle as MO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SHAPES = {"colbert": dict(KQ=1, KD=1), "coil": dict(KQ=1, KD=1), "citadel": dict(KQ=2, KD=3)}


def _to(r, dev, grad=True):
    out = {}
    for k, t in r.items():
        t = t.to(dev)
        if k == "expert_repr" or (k == "expert_weights" and t.is_floating_point()):
            t = t.clone().requires_grad_(grad)
        out[k] = t
    return out


def _run(qr, cr, mask, pairwise, pool, dS, kernels=None):
    from dpr_scale_amd import hotpath

    gq, gc = _to(qr, DEV), _to(cr, DEV)
    S = hotpath.expert_sim_score(gq, gc, None if mask is None else mask.to(DEV), pairwise, pool, kernels)
    fin = torch.isfinite(S)
    (S.masked_fill(~fin, 0.0) * dS.to(DEV).masked_fill(~fin, 0.0)).sum().backward()
    grads = {"dq": gq["expert_repr"].grad, "dc": gc["expert_repr"].grad}
    if gq.get("expert_weights") is not None and gq["expert_weights"].requires_grad:
        grads["dwq"], grads["dwc"] = gq["expert_weights"].grad, gc["expert_weights"].grad
    torch.cuda.synchronize()
    return S.detach().cpu(), {k: v.cpu() for k, v in grads.items()}


def _check(qr, cr, mask, pairwise, pool, seed=0, exact=True):
    B, Nc = qr["expert_repr"].shape[0], cr["expert_repr"].shape[0]
    Y = Nc // B if pairwise else Nc
    dS = torch.from_numpy(np.random.default_rng(seed).standard_normal((B, Y)).astype(np.float32))
    S, grads = _run(qr, cr, mask, pairwise, pool, dS)
    S0, g0 = MO.scores_and_grads(qr, cr, mask, pairwise, pool, dS)
    fin = torch.isfinite(S0)
    assert torch.equal(torch.isfinite(S), fin) and torch.all(S[~fin] == float("-inf"))
    if exact:
        assert torch.equal(S[fin].double(), S0[fin]), (S[fin] - S0[fin]).abs().max()
    else:
        assert (S[fin].double() - S0[fin]).abs().max() <= 1e-4 * max(S0[fin].abs().max().item(), 1.0)
    for k, ref in g0.items():
        got = grads[k].double()
        scale = max(ref.abs().max().item(), 1e-30)
        assert (got - ref).abs().max().item() <= 1e-3 * scale, (k, (got - ref).abs().max().item(), scale)
    return S, grads


@pytest.mark.parametrize("kind", MO.KINDS)
@pytest.mark.parametrize("pairwise", [False, True])
@pytest.mark.parametrize("pool", ["sum", "max"])
def test_matches_fp64_oracle(kind, pairwise, pool):
    qr, cr, mask = MO.make_inputs(11, kind, B=4, LQ=9, Nc=12, LD=21, d=40, masked=(2, 7), **SHAPES[kind])
    _check(qr, cr, mask, pairwise, pool)


@pytest.mark.parametrize("LQ,LD,d", [(1, 1, 32), (31, 179, 128), (7, 511, 40), (511, 31, 768), (32, 256, 128)])
def test_ragged_lengths_and_widths(LQ, LD, d):
    B, Nc = (2, 5) if max(LQ, LD) > 200 else (3, 13)
    for kind, KQ, KD in (("colbert", 1, 1), ("citadel", 2, 5), ("citadel", 8, 3)):
        qr, cr, mask = MO.make_inputs(LQ * 7 + LD + KQ, kind, B=B, LQ=LQ, Nc=Nc, LD=LD, d=d, masked=(1,), all_pad=(Nc - 1,), KQ=KQ,
                                      KD=KD, n_experts=12)
        # sums of up to 511 x 8 weighted maxima outgrow fp32's 24 bits on the grid: the issue's 1e-4 bar, not exactness
        _check(qr, cr, mask, False, "sum", exact=kind == "colbert")
    qr, cr, mask = MO.make_inputs(LQ + LD, "citadel", B=B, LQ=LQ, Nc=B * 2, LD=LD, d=d, masked=(1,), KQ=4, KD=2, n_experts=12)
    _check(qr, cr, mask, True, "max")


def test_gaussian_inputs_within_accumulation_error():
    qr, cr, mask = MO.make_inputs(5, "citadel", B=3, LQ=17, Nc=9, LD=45, d=128, KQ=2, KD=2, grid=False)
    _check(qr, cr, mask, False, "sum", exact=False)
    _check(qr, cr, mask, True, "max", exact=False)


def test_citadel_eight_slots_and_weight_grads():
    qr, cr, mask = MO.make_inputs(3, "citadel", B=2, LQ=6, Nc=6, LD=10, d=64, KQ=8, KD=8, n_experts=12, masked=(4,))
    _, grads = _check(qr, cr, mask, False, "sum")
    assert grads["dwq"].abs().sum() > 0 and grads["dwc"].abs().sum() > 0


def _tables(state, Nq, LQ, KQ, Ny):
    tab = Ny * Nq * LQ * KQ * 4
    off = (tab + 255) // 256 * 256
    return state[:tab].view(torch.float32).view(Ny, Nq * LQ * KQ), state[off:off + tab].view(torch.int32).view(Ny, Nq * LQ * KQ)


@pytest.mark.parametrize("kind", MO.KINDS)
def test_ties_go_to_the_lowest_index(kind):
    from dpr_scale_amd import hotpath

    B, LQ, Nc, LD, d = 3, 5, 4, 40, 32
    qr, cr, _ = MO.make_inputs(17, kind, B=B, LQ=LQ, Nc=Nc, LD=LD, d=d, pad_frac=0.6, **SHAPES[kind])
    c = cr["expert_repr"]
    c[:, 3] = c[:, 1]  # repeated tokens: exact ties between real tokens as well as between padding zeros / unmatched slots
    kn = hotpath.default_kernels()
    KQ, KD = SHAPES[kind]["KQ"], SHAPES[kind]["KD"]
    pad = (-d) % 32
    Qb = torch.nn.functional.pad(qr["expert_repr"], (0, pad)).to(DEV, torch.bfloat16).contiguous()
    Cb = torch.nn.functional.pad(c, (0, pad)).to(DEV, torch.bfloat16).contiguous()
    ids = [None, None]
    w = [None, None]
    if kind != "colbert":
        ids = [qr["expert_ids"].to(DEV, torch.int32).contiguous(), cr["expert_ids"].to(DEV, torch.int32).contiguous()]
        w = [qr["expert_weights"].to(DEV).float().contiguous(), cr["expert_weights"].to(DEV).float().contiguous()]
    S, state = kn.maxsim_fwd(Qb, Cb, ids[0], ids[1], w[0], w[1], KQ, KD, 0, 0, None)
    val, arg = _tables(state.cpu(), B, LQ, KQ, Nc)
    _, ref_arg, _ = MO.expert_sim_score(qr, cr, None, False, "sum", return_argmax=True)  # [B, LQ*KQ, Nc]
    ref_arg = ref_arg.permute(2, 0, 1).reshape(Nc, -1)
    assert torch.equal(arg.long(), ref_arg)


def test_two_runs_are_bit_identical():
    qr, cr, mask = MO.make_inputs(23, "citadel", B=4, LQ=20, Nc=16, LD=70, d=96, KQ=2, KD=3, grid=False, masked=(3,))
    dS = torch.randn(4, 16, generator=torch.Generator().manual_seed(1))
    a = _run(qr, cr, mask, False, "sum", dS)
    b = _run(qr, cr, mask, False, "sum", dS)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_calls_stay_inside_their_buffers():
    """Every output and the workspace sit between guard bands of a fixed pattern; forward and backward leave the bands untouched."""
    from dpr_scale_amd import _lib

    lib = _lib.lib
    B, LQ, Nc, LD, dp, KQ, KD = 3, 37, 12, 83, 64, 2, 3
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
    for pool, M in ((0, 0), (1, 0), (1, Nc // B), (0, Nc // B)):  # in-batch and pairwise (B * M = Nc contexts)
        Ny = M if M else Nc
        ws_n = _lib.maxsim_workspace_bytes(B, LQ, KQ, Ny, True)
        ws, S = guarded(ws_n), guarded(B * Ny * 4)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.dprhot_maxsim_fwd(p(Qb), p(Cb), B, LQ, Nc, LD, dp, p(qi), p(ci), p(qw), p(cw), KQ, KD, pool, M, p(m8), p(S),
                                         p(ws), ws_n, st))
        dS = put(torch.randn(B, Ny))
        dq, dc = guarded(B * LQ * dp * 4), guarded(Nc * LD * dp * 4)
        dwq, dwc = guarded(B * LQ * KQ * 4), guarded(Nc * LD * KD * 4)
        _lib.check(lib.dprhot_maxsim_bwd(p(dS), p(Qb), p(Cb), B, LQ, Nc, LD, dp, p(qi), p(ci), p(qw), p(cw), KQ, KD, pool, M, p(m8),
                                         p(ws), ws_n, p(dq), p(dc), p(dwq), p(dwc), st))
    torch.cuda.synchronize()
    for t, n in bufs:
        h = t.cpu()
        assert bool((h[:G] == 0xA5).all()) and bool((h[G + n:] == 0xA5).all()), f"guard band of a {n}-byte buffer overwritten"


def test_at_scale_against_sampled_oracle_rows():
    """128 queries x 32 tokens against 1024 contexts x 256 tokens, d = 128: forward and dQ checked on sampled query rows (a full fp64
    oracle is too large); the kernel never holds the [Nq, LQ, Nc, LD] tensor (peak memory well below its 4.3 GB)."""
    B, LQ, Nc, LD, d = 128, 32, 1024, 256, 128
    qr, cr, _ = MO.make_inputs(2024, "colbert", B=B, LQ=LQ, Nc=Nc, LD=LD, d=d)
    from dpr_scale_amd import hotpath

    torch.cuda.reset_peak_memory_stats()
    gq, gc = _to(qr, DEV), _to(cr, DEV)
    base = torch.cuda.memory_allocated()
    S = hotpath.expert_sim_score(gq, gc, None, False, "sum")
    dS = torch.randn(B, Nc, generator=torch.Generator().manual_seed(3)).to(DEV)
    (S * dS).sum().backward()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 512 * 2**20
    rows = [0, 37, 127]
    sub_q = {"expert_repr": qr["expert_repr"][rows]}
    lq = MO.leaf(sub_q)
    lc = MO.leaf(cr)
    S0 = MO.expert_sim_score(lq, lc, None, False, "sum")
    assert torch.equal(S.detach().cpu()[rows].double(), S0.detach())
    (S0 * dS.cpu()[rows].double()).sum().backward()
    ref = lq["expert_repr"].grad
    got = gq["expert_repr"].grad.cpu()[rows].double()
    assert (got - ref).abs().max() <= 1e-3 * ref.abs().max()
    # dC on sampled contexts: a context's gradient depends only on its own column of S
    ctxs = [0, 511, 1023]
    lq2, lc2 = MO.leaf(qr), MO.leaf({"expert_repr": cr["expert_repr"][ctxs]})
    S1 = MO.expert_sim_score(lq2, lc2, None, False, "sum")
    assert torch.equal(S.detach().cpu()[:, ctxs].double(), S1.detach())
    (S1 * dS.cpu()[:, ctxs].double()).sum().backward()
    ref_c = lc2["expert_repr"].grad
    got_c = gc["expert_repr"].grad.cpu()[ctxs].double()
    assert (got_c - ref_c).abs().max() <= 1e-3 * ref_c.abs().max()


def test_dropin_task_step_on_gpu():
    from test_multivec import _attach, make_task, toy_batch

    batch, qr, cr = toy_batch(7, "citadel", DEV)
    task = _attach(make_task(in_batch=True, query_pool="sum"), qr, cr, DEV)
    loss = task.training_step(batch, 0)
    loss.backward()
    assert torch.isfinite(loss)
    ref_loss = torch.nn.functional.cross_entropy(MO.expert_sim_score(qr, cr, batch["ctx_mask"].cpu()).float(),
                                                 batch["pos_ctx_indices"].cpu())
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * max(1.0, abs(ref_loss.item()))
    assert "train_expert_loss" in task.logged


@pytest.mark.parametrize("kind", MO.KINDS)
@pytest.mark.parametrize("pool", ["sum", "max"])
def test_nan_tokens_give_nan_scores_as_the_reference(kind, pool):
    """A NaN token (how a diverging run shows up) propagates as torch.max propagates it: NaN scores wherever the reference has them,
    valid argmax indices in the tables, and a backward that runs (on valid indices only)."""
    from dpr_scale_amd import hotpath

    B, LQ, Nc, LD, d = 3, 6, 5, 9, 32
    qr, cr, mask = MO.make_inputs(77, kind, B=B, LQ=LQ, Nc=Nc, LD=LD, d=d, masked=(2,), **SHAPES[kind])
    qr["expert_repr"][1, :] = float("nan")   # every token of query 1
    cr["expert_repr"][3, 4, 0] = float("nan")  # one token of context 3
    S0 = MO.expert_sim_score(qr, cr, mask, False, pool)
    gq, gc = _to(qr, DEV), _to(cr, DEV)
    S = hotpath.expert_sim_score(gq, gc, mask.to(DEV), False, pool)
    Sc = S.detach().cpu().double()
    assert torch.equal(torch.isnan(Sc), torch.isnan(S0)) and bool(torch.isnan(S0).any())
    fin = torch.isfinite(S0)
    assert torch.equal(Sc[fin], S0[fin]) and torch.equal(Sc[torch.isinf(S0)], S0[torch.isinf(S0)])
    S.nansum().backward()
    torch.cuda.synchronize()
    assert gq["expert_repr"].grad is not None and gc["expert_repr"].grad is not None
    kn = hotpath.default_kernels()
    Qb = qr["expert_repr"].to(DEV, torch.bfloat16).contiguous()
    Cb = cr["expert_repr"].to(DEV, torch.bfloat16).contiguous()
    KQ, KD = SHAPES[kind]["KQ"], SHAPES[kind]["KD"]
    ids = [None, None] if kind == "colbert" else [qr["expert_ids"].to(DEV, torch.int32).contiguous(),
                                                    cr["expert_ids"].to(DEV, torch.int32).contiguous()]
    w = [None, None] if kind == "colbert" else [qr["expert_weights"].to(DEV).float().contiguous(),
                                                  cr["expert_weights"].to(DEV).float().contiguous()]
    _, state = kn.maxsim_fwd(Qb, Cb, ids[0], ids[1], w[0], w[1], KQ, KD, 0, 0, None)
    _, arg = _tables(state.cpu(), B, LQ, KQ, Nc)
    assert int(arg.min()) >= 0 and int(arg.max()) < LD * KD
    _, ref_arg, _ = MO.expert_sim_score(qr, cr, None, False, "sum", return_argmax=True)
    assert torch.equal(arg.long(), ref_arg.permute(2, 0, 1).reshape(Nc, -1))
