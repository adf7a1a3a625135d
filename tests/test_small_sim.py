"""The barrier-free similarity launch of the batch-32 step (csrc/sim_small.h, option small_sim) against the GEMM engine it replaces
(small_sim = 0), in one process: the results must be the SAME BITS, not merely close -- the new kernel rounds, places and sums every
operand exactly as gemm_tile's tile 5 does.  Compared: everything dprhot_sim_stats_f32 leaves behind (the whole workspace -- partial-
logit slabs and the cleared header words included -- Qb, Cb, and the summed logits dprhot_softmax_finish forms from the slabs) and
everything the one-call steps return.  Every form the option can select (wave-private LDS patch / registers, one / two waves per
workgroup) is held to the same equality.  Shapes outside the kernel's guard (32 x 1032: the single-slab plan) run the engine under
both settings and are listed so that the guard cannot start taking them unnoticed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")


def test_new_kernel_has_no_scratch():
    """Every instantiation of sim_small_kernel: no scratch, no spilled VGPR (its loads are meant to stay in flight in registers)."""
    assert os.path.isfile(REPORT), "no resource report next to the library: build with the Makefile (__graft_entry__.build)"
    cur, rows = None, {}
    for ln in open(REPORT, errors="replace"):
        m = re.search(r" Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", ln)
        if m and cur:
            rows[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    mine = {k: v for k, v in rows.items() if "16sim_small_kernel" in k}
    assert len(mine) == 4, f"expected the four instantiations of sim_small_kernel in the report, found {sorted(mine)}"
    for name, r in mine.items():
        assert r == {"ScratchSize": 0, "VGPRs Spill": 0}, f"{name}: {r}"


# B, Nc, d, T, masked fraction
SHAPES = [
    pytest.param(32, 256, 768, 1.0, 0.0, id="cfg2"),
    pytest.param(32, 64, 768, 1.0, 0.0, id="32x64x768"),
    pytest.param(32, 528, 768, 1.0, 0.05, id="32x528x768"),
    pytest.param(32, 1032, 768, 1.0, 0.05, id="32x1032x768"),
    pytest.param(32, 256, 1024, 1.0, 0.0, id="32x256x1024"),
    pytest.param(27, 248, 768, 0.05, 0.2, id="ragged-27x248-masked-T0.05"),
]
FORMS = [1, 2, 3, 4]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture()
def small_sim():
    """Sets the option for the duration of a test and restores the default."""
    from dpr_scale_amd import _lib

    default = _lib.get_option("small_sim")
    yield lambda v: _lib.set_option("small_sim", v)
    _lib.set_option("small_sim", default)


def _inputs(B, Nc, d, mask_frac, dev, seed):
    import torch

    gen = torch.Generator(device="cpu").manual_seed(seed)
    # (NOT bf16-representable: the rounding of both operands is part of what is compared)
    q = (torch.randn(B, d, generator=gen) * d ** -0.25).to(dev)
    c = (torch.randn(Nc, d, generator=gen) * d ** -0.25).to(dev)
    y = torch.randperm(Nc, generator=gen)[:B].to(torch.int64)
    m = torch.rand(Nc, generator=gen) < mask_frac
    m[y] = False
    return q, c, y.to(dev), (m.to(torch.uint8).to(dev) if mask_frac > 0 else None)


def _bits(t):
    import torch

    if t is None:
        return None
    t = t.contiguous()
    return t.view(torch.uint8).cpu().numpy().copy() if t.dtype == torch.uint8 else t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().copy()


def _same(a, b, what):
    import numpy as np

    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), f"{what}[{k}]"
        if x is not None:
            assert np.array_equal(x, y), f"{what}[{k}]: {int((x != y).sum())} of {x.size} words differ"


def _sim_stats(B, Nc, d, T, q, c, y, mask, dev):
    """dprhot_sim_stats_f32 into a workspace, Qb and Cb that start from a fixed byte pattern, then dprhot_softmax_finish with S_in:
    (whole workspace after the sim launch, Qb, Cb, summed logits, row_loss, row_lse, loss_sum, G)."""
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import _ptr

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = _lib.workspace_bytes(B, Nc, d)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    Qb = torch.full((B, d), 7.0, dtype=torch.bfloat16, device=dev)
    Cb = torch.full((Nc, d), 7.0, dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.lib.dprhot_sim_stats_f32(_ptr(q), _ptr(c), _ptr(Qb), _ptr(Cb), B, Nc, d, _ptr(y), 0, _ptr(mask), 1.0 / T, None,
                                             _ptr(ws), nbytes, st), "dprhot_sim_stats_f32")
    torch.cuda.synchronize()
    ws_after = _bits(ws)
    S = torch.full((B, Nc), 3.0, dtype=torch.float32, device=dev)
    row_loss = torch.zeros(B, dtype=torch.float32, device=dev)
    row_lse = torch.zeros(B, dtype=torch.float32, device=dev)
    loss_sum = torch.zeros(1, dtype=torch.float32, device=dev)
    G = torch.zeros((B, Nc), dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.lib.dprhot_softmax_finish(_ptr(S), B, Nc, d, _ptr(y), 0, 1.0 / (T * B), _ptr(row_loss), _ptr(row_lse), _ptr(loss_sum),
                                              _ptr(G), _ptr(ws), nbytes, st), "dprhot_softmax_finish")
    torch.cuda.synchronize()
    return [ws_after, _bits(Qb), _bits(Cb), _bits(S), _bits(row_loss), _bits(row_lse), _bits(loss_sum), _bits(G)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc,d,T,mask_frac", SHAPES)
def test_sim_stats_same_bits_as_engine(B, Nc, d, T, mask_frac, dev, small_sim):
    import numpy as np

    q, c, y, mask = _inputs(B, Nc, d, mask_frac, dev, seed=B * 1000 + Nc)
    small_sim(0)
    ref = _sim_stats(B, Nc, d, T, q, c, y, mask, dev)
    assert np.array_equal(ref[0][:16], np.zeros(16, np.uint8)), "the sim launch clears the two header words"
    assert np.isfinite(ref[3].view(np.float32)).any() and not np.array_equal(ref[1], np.full_like(ref[1], ref[1].flat[0]))
    for form in FORMS:
        small_sim(form)
        _same(_sim_stats(B, Nc, d, T, q, c, y, mask, dev), ref, f"small_sim={form} sim_stats")


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc,d,T,mask_frac", SHAPES)
def test_whole_step_same_bits_as_engine(B, Nc, d, T, mask_frac, dev, small_sim):
    import torch

    from dpr_scale_amd.hotpath import HipKernels

    kn = HipKernels()
    q, c, y, mask = _inputs(B, Nc, d, mask_frac, dev, seed=B * 1000 + Nc + 1)

    def step():
        Qb = torch.full((B, d), 7.0, dtype=torch.bfloat16, device=dev)
        Cb = torch.full((Nc, d), 7.0, dtype=torch.bfloat16, device=dev)
        out = kn.inbatch_step_f32(q, c, Qb, Cb, y, 0, mask, 1.0 / T, 1.0 / (T * B), want_G=True)
        torch.cuda.synchronize()
        return [_bits(o) for o in out] + [_bits(Qb), _bits(Cb)]  # row_loss, row_lse, loss_sum, G, dQ, dC, Qb, Cb

    small_sim(0)
    ref = step()
    for form in FORMS:
        small_sim(form)
        _same(step(), ref, f"small_sim={form} step")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [768, 1024])
def test_packed_two_rank_step_same_bits_as_engine(d, dev, small_sim):
    """dprhot_inbatch_step_packed_f32: bf16 gathered contexts (read as fragments straight from memory), the column mask taken from the
    packed buffer, the loss stamp in dC."""
    import torch

    from dpr_scale_amd.hotpath import HipKernels

    kn = HipKernels()
    W, B, K, T = 2, 32, 8, 0.5
    n_ctx = B * K
    gen = torch.Generator(device="cpu").manual_seed(77 + d)
    rows_c = kn.packed_rows(n_ctx, d)
    sends, qs = [], []
    for r in range(W):
        qs.append((torch.randn(B, d, generator=gen) * d ** -0.25).to(dev))
        c = (torch.randn(n_ctx, d, generator=gen) * d ** -0.25).to(dev)
        m = torch.rand(n_ctx, generator=gen) < 0.1
        m[torch.arange(B) * K] = False
        send = torch.empty((rows_c, d), dtype=torch.bfloat16, device=dev)
        kn.pack_ctx(c, m.to(torch.uint8).to(dev), send)
        sends.append(send)
    Cb = torch.cat(sends, 0).contiguous()
    y = (torch.arange(B) * K).to(torch.int64).to(dev)

    def step(r):
        Qb = torch.full((B, d), 7.0, dtype=torch.bfloat16, device=dev)
        out = kn.inbatch_step_packed_f32(qs[r], Cb, Qb, W, r, n_ctx, y, 1.0 / T, 1.0 / (T * W * B), want_G=True)
        torch.cuda.synchronize()
        return [_bits(o) for o in out] + [_bits(Qb)]

    small_sim(0)
    ref = [step(r) for r in range(W)]
    for form in FORMS:
        small_sim(form)
        for r in range(W):
            _same(step(r), ref[r], f"small_sim={form} packed step, rank {r}")
