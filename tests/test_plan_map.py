"""The default dispatcher walked across every gate of tests/test_bounds_cpu.py's plan table, with NO set_option call: each shape just
inside and just outside a gate runs through the library's entry points of the training step and every output is held to the per-element
fp64 bounds of tests/_bounds.py.  The kernels each row launches are recorded; the last test asserts they cover every kernel family of
the training step.  Prints one `[bound-ratio]` line per case (worst score per output, ambiguous G elements)."""
import math

import pytest
import torch

import _bounds as BD
from test_bounds_cpu import PLAN_TABLE

pytestmark = pytest.mark.gpu

MAX_SCORES = 1 << 27  # fp64 references of at most this many scores per case (device memory)
SHAPES = sorted({s for r in PLAN_TABLE for s in (r[1], r[3]) if s[0] * s[1] <= MAX_SCORES})
KINDS = ["flat", "peaky", "dup", "lonely"]
LAUNCHED = {}  # shape -> kernel names seen

# kernel families of the training step (substrings of the launched kernels' names)
# (the fused small step; the few-rows step's sim, dScores and backward units with and without the dScores launch; the wide-vector sim;
# the register-staged sim, streaming softmax and backward pair; the one-pass forwards on the 256 x 256 and 128 x 128 tiles and their
# row kernel; the backward pairs on the 128 x 128 LDS-DMA tile and the phase-interleaved 256 x 256 tile.  The 256 x 256 LDS-DMA pair,
# gemm256_bwd_kernel, is not one of them: the shapes of this table all qualify for the phase-interleaved kernel -- it runs only where a
# shape fails a term of `ok8` in inbatch_bwd_body: B or Nc no multiple of 64, kchunk % 128 != 0, or operands past 2^31 bytes.)
FAMILIES = ["step_small_kernel", "sk_sim_kernel", "sk_simp_kernel", "sk_g_kernel", "sk_bwd_kernel", "sk_bwdf_kernel", "wide_sim_kernel",
            "gemm_bf16_kernel", "gfinal_kernel", "gfinal_short_kernel", "gemm_pair_kernel", "gemm8p_kernel", "g8_lse_p2g_kernel",
            "gemm128d_kernel", "gemm128d_pair_kernel", "gemm8p_bwd_kernel"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def kn():
    from dpr_scale_amd.hotpath import default_kernels

    return default_kernels()


def _problem(B, Nc, d, kind, seed, dev):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    scale, T = (1.0, 0.05) if kind == "peaky" else (d ** -0.25, 0.5)
    q = (torch.randn(B, d, generator=gen) * scale).to(torch.bfloat16).float()
    c = (torch.randn(Nc, d, generator=gen) * scale).to(torch.bfloat16).float()
    if kind == "dup":  # exact score ties
        src = torch.randint(0, Nc, (max(Nc // 16, 1),), generator=gen)
        dst = torch.randint(0, Nc, (max(Nc // 16, 1),), generator=gen)
        c[dst] = c[src]
    y = torch.randint(0, Nc, (B,), generator=gen)
    mask = torch.rand(Nc, generator=gen) < 0.05
    mask[y[: B // 2]] = False  # the other half's gold columns may be masked (loss +inf there)
    if kind == "lonely":  # one row with everything but its gold masked (a column mask: every row sees that one column only)
        mask[:] = True
        mask[y[0]] = False
    return q.to(dev), c.to(dev), y.to(dev), mask.to(torch.uint8).to(dev), T


def _record(shape, fn):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    LAUNCHED.setdefault(shape, set()).update(n for n in names if "Memcpy" not in n and "Memset" not in n)
    return out


def _report(tag, sc, n_amb):
    print(f"[bound-ratio] {tag}: worst {max(sc.values()):.3g} " + " ".join(f"{k} {v:.3g}" for k, v in sc.items()) + f"; ambiguous G {n_amb}")
    bad = {k: v for k, v in sc.items() if not v <= 1.0}
    assert not bad, (tag, sc)


@pytest.mark.parametrize("B,Nc,d", SHAPES)
def test_default_plan_within_elementwise_bounds(B, Nc, d, kn, dev):
    from dpr_scale_amd import _lib, hotpath

    i = SHAPES.index((B, Nc, d))
    kind = KINDS[i % len(KINDS)]
    q, c, y, m8, T = _problem(B, Nc, d, kind, 1000 + i, dev)
    inv_T = 1.0 / T
    gs = inv_T / B
    one_pass = _lib.fwd_one_pass(B, Nc, d) > 0
    ref = BD.forward(q, c, y, m8, inv_T, gs, f16=one_pass)
    Qb = q.to(torch.bfloat16)
    Cb = c.to(torch.bfloat16)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    tag = f"{B}x{Nc}x{d} {kind}"

    # forward, then backward from the exposed G
    def fb():
        rl, lse, ls, G, _ = kn.inbatch_fwd(Qb, Cb, y, 0, m8, inv_T, gs)
        dq, dc = kn.inbatch_bwd(G, Qb, Cb, 1.0, one)
        return rl, lse, ls, G, dq, dc

    rl, lse, ls, G, dq, dc = _record((B, Nc, d), fb)
    sc, n_amb = BD.check_step(ref, row_loss=rl, row_lse=lse, loss_sum=ls.item(), G=G, dQ=dq, dC=dc, q=q, c=c, slabs_q=64, slabs_c=64)
    _report(f"{tag} fwd+bwd", sc, n_amb)

    # one-call step, G wanted
    Qs = torch.empty_like(Qb)
    Cs = torch.empty_like(Cb)
    rl, lse, ls, G, dq, dc = _record((B, Nc, d), lambda: kn.inbatch_step_f32(q, c, Qs, Cs, y, 0, m8, inv_T, gs, want_G=True))
    sc, n_amb = BD.check_step(ref, row_loss=rl, row_lse=lse, loss_sum=ls.item(), G=G, dQ=dq, dC=dc, q=q, c=c, slabs_q=64, slabs_c=64)
    _report(f"{tag} step G", sc, n_amb)
    hidden = "bf16_g_f16num" if one_pass else "bf16_g"
    if not _lib.step_wants_g(B, Nc, d):  # the few-rows step without its dScores launch
        hidden = "sk_tile_bf16"
        rl, lse, ls, G0, dq, dc = _record((B, Nc, d), lambda: kn.inbatch_step_f32(q, c, Qs, Cs, y, 0, m8, inv_T, gs, want_G=False))
        assert G0 is None
        sc, n_amb = BD.check_step(ref, row_loss=rl, row_lse=lse, loss_sum=ls.item(), dQ=dq, dC=dc, q=q, c=c, model=hidden, slabs_q=64,
                                  slabs_c=64)
        _report(f"{tag} step G=NULL ({hidden})", sc, n_amb)

    # the operator's step: loss multiplied by loss_scale, gradients by the device scalar
    d_scale = torch.full((1,), 2.0, dtype=torch.float32, device=dev)
    rl, lse, lo, G, dq, dc = _record((B, Nc, d), lambda: kn.train_step_f32(q, c, Qs, Cs, y, 0, m8, inv_T, gs, 1.0 / B, d_scale))
    sc, n_amb = BD.check_step(ref, row_loss=rl, row_lse=lse, loss_sum=lo[0].item(), loss_scale=1.0 / B, G=G, dQ=dq, dC=dc, q=q, c=c, h=2.0,
                              slabs_q=64, slabs_c=64)
    _report(f"{tag} train_step", sc, n_amb)

    # the autograd operator with a loss scale (G stays inside: the plan's rounding model)
    tq = q.clone().requires_grad_(True)
    tc = c.clone().requires_grad_(True)

    def op():
        loss = hotpath.inbatch_contrastive_loss(tq, tc, y, m8, T)
        loss.backward(torch.full((), 8.0, device=dev))
        return loss

    loss = _record((B, Nc, d), op)
    sc, n_amb = BD.check_step(ref, loss_sum=loss.item(), loss_scale=1.0 / B, dQ=tq.grad, dC=tc.grad, q=q, c=c, h=8.0, model=hidden,
                              slabs_q=64, slabs_c=64)
    _report(f"{tag} operator ({hidden})", sc, n_amb)


def test_hidden_size_not_a_multiple_of_8_through_the_operator(dev):
    """d % 8 != 0: the operator zero-pads the hidden axis; the bounds of the unpadded problem hold."""
    from dpr_scale_amd import hotpath

    B, Nc, d = 256, 2048, 764
    q, c, y, m8, T = _problem(B, Nc, d, "flat", 77, dev)
    tq = q.clone().requires_grad_(True)
    tc = c.clone().requires_grad_(True)
    loss = hotpath.inbatch_contrastive_loss(tq, tc, y, m8, T)
    loss.backward()
    from dpr_scale_amd import _lib

    model = "bf16_g_f16num" if _lib.fwd_one_pass(B, Nc, d + 4) > 0 else "bf16_g"
    ref = BD.forward(q, c, y, m8, 1.0 / T, 1.0 / (T * B), f16=model == "bf16_g_f16num")
    sc, n_amb = BD.check_step(ref, loss_sum=loss.item(), loss_scale=1.0 / B, dQ=tq.grad, dC=tc.grad, q=q, c=c, model=model, slabs_q=64,
                              slabs_c=64)
    _report(f"{B}x{Nc}x{d} operator, d % 8 = 4 ({model})", sc, n_amb)


@pytest.mark.parametrize("W,B,K,d", [(2, 256, 8, 768), (4, 128, 16, 768)])
def test_packed_step_within_elementwise_bounds(W, B, K, d, kn, dev):
    """The packed multi-rank layout (mask bytes in trailing rows of the gathered buffer), every rank of the world emulated on one GPU."""
    n_ctx = B * K
    rows_c = kn.packed_rows(n_ctx, d)
    Nc = W * rows_c
    gen = torch.Generator(device="cpu").manual_seed(W * 100 + B)
    qs = [(torch.randn(B, d, generator=gen) * d ** -0.25).to(torch.bfloat16).float().to(dev) for _ in range(W)]
    cs = [(torch.randn(n_ctx, d, generator=gen) * d ** -0.25).to(torch.bfloat16).float().to(dev) for _ in range(W)]
    ms = [(torch.rand(n_ctx, generator=gen) < 0.05) for _ in range(W)]
    y = torch.arange(B) * K
    for m in ms:
        m[y[: B // 2]] = False
    sends = []
    for r in range(W):
        send = torch.empty((rows_c, d), dtype=torch.bfloat16, device=dev)
        kn.pack_ctx(cs[r], ms[r].to(torch.uint8).to(dev), send)
        sends.append(send)
    Cb = torch.cat(sends, 0).contiguous()
    c_ref = torch.zeros(Nc, d, device=dev)
    mask_ref = torch.ones(Nc, dtype=torch.uint8, device=dev)
    for r in range(W):
        c_ref[r * rows_c:r * rows_c + n_ctx] = cs[r]
        mask_ref[r * rows_c:r * rows_c + n_ctx] = ms[r].to(torch.uint8).to(dev)
    yd = y.to(dev)
    T = 0.5
    gs = 1.0 / (T * W * B)
    Qb = torch.empty((B, d), dtype=torch.bfloat16, device=dev)
    one_pass = kn._lib.fwd_one_pass(B, Nc, d) > 0
    for r in range(W):
        ref = BD.forward(qs[r], c_ref, yd, mask_ref, 1.0 / T, gs, y_offset=r * rows_c, f16=one_pass)
        rl, lse, ls, G, dq, dcp = _record((W, B, K, d), lambda: kn.inbatch_step_packed_f32(qs[r], Cb, Qb, W, r, n_ctx, yd, 1.0 / T, gs, want_G=True))
        dcp = dcp.clone()
        for k in range(W):  # the loss numerator rides in the first mask row of every chunk
            stamp, total = dcp[k * rows_c + n_ctx, 0].item(), ls.item()
            assert stamp == total if not math.isfinite(total) else abs(stamp - total) <= 1e-6 * abs(total)
            dcp[k * rows_c + n_ctx, 0] = 0.0
        sc, n_amb = BD.check_step(ref, row_loss=rl, row_lse=lse, loss_sum=ls.item(), G=G, dQ=dq, dC=dcp, q=qs[r], c=c_ref, slabs_q=64,
                                  slabs_c=64)
        _report(f"packed W{W} {B}x{K}x{d} rank {r}", sc, n_amb)


def test_launched_kernels_cover_every_family_of_the_training_step(kn, dev):
    names = set().union(*LAUNCHED.values()) if LAUNCHED else set()
    if not LAUNCHED:
        pytest.skip("no plan-map row ran in this session")
    if not names:
        pytest.skip("the profiler recorded no device activity on this box")
    print("[plan-map kernels] " + " | ".join(sorted(names)))
    missing = [f for f in FAMILIES if not any(f in n for n in names)]
    assert not missing, (missing, sorted(names))
