"""The sim launch of the batch-32 step on its exact three-dimensional grid (csrc/sim_small.h: row tile, column tile and K chunk from the
block index, the mask byte loaded behind the operands) against the GEMM engine (small_sim = 0), in one process: what
dprhot_sim_stats_f32 leaves behind -- the whole workspace with its partial-logit slabs and cleared header words, Qb, Cb -- and what the
one-call step returns must be the SAME WORDS, for every form the option selects (1-4: LDS patch / registers, one / two waves per
workgroup), with and without a column mask.  Shapes: two row tiles and one, one ragged column tile, a column count that is no multiple
of 16 tiles per slab plan, four K chunks; and the packed one-rank step (bf16 contexts, padded columns, the mask in the packed buffer)."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

# B, Nc, d
SHAPES = {
    "cfg2": (32, 256, 768),
    "16x256x768-one-row-tile": (16, 256, 768),
    "9x8x768-one-column-tile-ragged-rows": (9, 8, 768),
    "32x528x768": (32, 528, 768),
    "32x256x1024-four-chunks": (32, 256, 1024),
}
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


def _inputs(B, Nc, d, masked, dev, seed):
    import torch

    gen = torch.Generator(device="cpu").manual_seed(seed)
    # (NOT bf16-representable: the rounding of both operands is part of what is compared)
    q = (torch.randn(B, d, generator=gen) * d ** -0.25).to(dev)
    c = (torch.randn(Nc, d, generator=gen) * d ** -0.25).to(dev)
    # (a label per row: fewer columns than rows -- 9 x 8 -- draws them with repetition)
    y = (torch.randperm(Nc, generator=gen)[:B] if Nc >= B else torch.randint(0, Nc, (B,), generator=gen)).to(torch.int64)
    m = torch.rand(Nc, generator=gen) < 0.25
    m[y] = False
    if Nc > B:
        m[[j for j in range(Nc) if j not in set(y.tolist())][0]] = True  # (at least one masked column)
    return q, c, y.to(dev), (m.to(torch.uint8).to(dev) if masked else None)


def _bits(t):
    import torch

    t = t.contiguous()
    return t.view(torch.uint8).cpu().numpy().copy() if t.dtype == torch.uint8 else t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().copy()


def _same(a, b, what):
    import numpy as np

    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"{what}[{k}]: {int((x != y).sum())} of {x.size} words differ"


def _sim_stats(B, Nc, d, q, c, y, mask, dev):
    """dprhot_sim_stats_f32 into a workspace, Qb and Cb that start from a fixed byte pattern: (workspace, Qb, Cb)."""
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import _ptr

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = _lib.workspace_bytes(B, Nc, d)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    Qb = torch.full((B, d), 7.0, dtype=torch.bfloat16, device=dev)
    Cb = torch.full((Nc, d), 7.0, dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.lib.dprhot_sim_stats_f32(_ptr(q), _ptr(c), _ptr(Qb), _ptr(Cb), B, Nc, d, _ptr(y), 0, _ptr(mask), 1.0, None,
                                             _ptr(ws), nbytes, st), "dprhot_sim_stats_f32")
    torch.cuda.synchronize()
    return [_bits(ws), _bits(Qb), _bits(Cb)]


def _whole_step(B, Nc, d, q, c, y, mask, dev):
    import torch

    from dpr_scale_amd.hotpath import HipKernels

    kn = HipKernels()
    Qb = torch.full((B, d), 7.0, dtype=torch.bfloat16, device=dev)
    Cb = torch.full((Nc, d), 7.0, dtype=torch.bfloat16, device=dev)
    out = kn.inbatch_step_f32(q, c, Qb, Cb, y, 0, mask, 1.0, 1.0 / B, want_G=True)
    torch.cuda.synchronize()
    return [_bits(o) for o in out] + [_bits(Qb), _bits(Cb)]  # row_loss, row_lse, loss_sum, G, dQ, dC, Qb, Cb


@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "column-mask"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_same_words_as_engine(name, masked, dev, small_sim):
    import numpy as np

    B, Nc, d = SHAPES[name]
    q, c, y, mask = _inputs(B, Nc, d, masked, dev, seed=B * 1000 + Nc + 3)
    small_sim(0)
    ref = _sim_stats(B, Nc, d, q, c, y, mask, dev)
    ref_step = _whole_step(B, Nc, d, q, c, y, mask, dev)
    assert np.array_equal(ref[0][:16], np.zeros(16, np.uint8)), "the sim launch clears the two header words"
    assert not np.array_equal(ref[1], np.full_like(ref[1], ref[1].flat[0])) and not np.array_equal(ref[2], np.full_like(ref[2], ref[2].flat[0]))
    if masked and Nc > B:
        assert (ref_step[3] == 0).any(), "a masked column has dScores +0"
    for form in FORMS:
        small_sim(form)
        _same(_sim_stats(B, Nc, d, q, c, y, mask, dev), ref, f"small_sim={form} {name} sim_stats")
        _same(_whole_step(B, Nc, d, q, c, y, mask, dev), ref_step, f"small_sim={form} {name} step")


@pytest.mark.parametrize("d", [768, 1024])
def test_packed_one_rank_step_same_words_as_engine(d, dev, small_sim):
    """dprhot_inbatch_step_packed_f32 at W = 1: the bf16-context instantiation, columns padded to the packed row count and masked there,
    the column mask read from the packed buffer."""
    import torch

    from dpr_scale_amd.hotpath import HipKernels

    kn = HipKernels()
    W, B, K, T = 1, 32, 8, 0.5
    n_ctx = B * K
    gen = torch.Generator(device="cpu").manual_seed(177 + d)
    rows_c = kn.packed_rows(n_ctx, d)
    assert rows_c > n_ctx
    q = (torch.randn(B, d, generator=gen) * d ** -0.25).to(dev)
    c = (torch.randn(n_ctx, d, generator=gen) * d ** -0.25).to(dev)
    m = torch.rand(n_ctx, generator=gen) < 0.1
    m[torch.arange(B) * K] = False
    Cb = torch.empty((rows_c, d), dtype=torch.bfloat16, device=dev)
    kn.pack_ctx(c, m.to(torch.uint8).to(dev), Cb)
    y = (torch.arange(B) * K).to(torch.int64).to(dev)

    def step():
        Qb = torch.full((B, d), 7.0, dtype=torch.bfloat16, device=dev)
        out = kn.inbatch_step_packed_f32(q, Cb, Qb, W, 0, n_ctx, y, 1.0 / T, 1.0 / (T * W * B), want_G=True)
        torch.cuda.synchronize()
        return [_bits(o) for o in out] + [_bits(Qb)]

    small_sim(0)
    ref = step()
    for form in FORMS:
        small_sim(form)
        _same(step(), ref, f"small_sim={form} packed one-rank step")
