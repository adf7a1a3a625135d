"""The sim launch of the batch-32 step with its bf16 copies on waves of their own (option small_sim_copy, csrc/sim_small.h:
sim_small_split_kernel) against the GEMM engine (small_sim = 0), in one process, for both values of the option: what dprhot_sim_stats_f32
leaves behind -- the whole workspace with its partial-logit slabs and cleared header words, Qb, Cb -- and every output of the one-call
step must be the SAME WORDS, with and without a column mask.  Shapes: the flagship, one row tile, one ragged tile each way (copy waves
meet clamped rows, and one layer of the grid has fewer waves than there are operand tiles), 33 column tiles, four K chunks; and the
packed one-rank step (bf16 contexts: Q copies only).  Qb and Cb are the first rows of larger buffers filled with a pattern, and the rows
behind them must keep it: a copy wave that stores a clamped row is seen."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

# B, Nc, d
SHAPES = {
    "cfg2": (32, 256, 768),
    "16x256x768-one-row-tile": (16, 256, 768),
    "9x8x768-one-ragged-tile-each-way": (9, 8, 768),
    "32x528x768-33-column-tiles": (32, 528, 768),
    "32x256x1024-four-chunks": (32, 256, 1024),
}
GUARD = 24  # rows behind Qb / Cb: more than one 16-row tile
PATTERN = 7.0


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture()
def options():
    """Sets small_sim / small_sim_copy for the duration of a test and restores the defaults."""
    from dpr_scale_amd import _lib

    defaults = {k: _lib.get_option(k) for k in ("small_sim", "small_sim_copy")}
    yield lambda sim, copy: (_lib.set_option("small_sim", sim), _lib.set_option("small_sim_copy", copy))
    for k, v in defaults.items():
        _lib.set_option(k, v)


def _inputs(B, Nc, d, masked, dev, seed):
    import torch

    gen = torch.Generator(device="cpu").manual_seed(seed)
    # (NOT bf16-representable: the rounding of both operands is part of what is compared)
    q = (torch.randn(B, d, generator=gen) * d ** -0.25).to(dev)
    c = (torch.randn(Nc, d, generator=gen) * d ** -0.25).to(dev)
    assert not torch.equal(q.bfloat16().float(), q) and not torch.equal(c.bfloat16().float(), c)
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


def _guarded(rows, d, dev):
    """(the whole buffer, the view of its first `rows` rows that a call is given)"""
    import torch

    whole = torch.full((rows + GUARD, d), PATTERN, dtype=torch.bfloat16, device=dev)
    return whole, whole[:rows]


def _guard_kept(whole, rows, what):
    import torch

    assert bool((whole[rows:] == PATTERN).all()), f"{what}: rows behind the operand were written"


def _sim_stats(B, Nc, d, q, c, y, mask, dev, what):
    """dprhot_sim_stats_f32 into a workspace, Qb and Cb that start from a fixed byte pattern: (workspace, Qb, Cb)."""
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import _ptr

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = _lib.workspace_bytes(B, Nc, d)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    Qw, Qb = _guarded(B, d, dev)
    Cw, Cb = _guarded(Nc, d, dev)
    _lib.check(_lib.lib.dprhot_sim_stats_f32(_ptr(q), _ptr(c), _ptr(Qb), _ptr(Cb), B, Nc, d, _ptr(y), 0, _ptr(mask), 1.0, None,
                                             _ptr(ws), nbytes, st), "dprhot_sim_stats_f32")
    torch.cuda.synchronize()
    _guard_kept(Qw, B, what + " Qb")
    _guard_kept(Cw, Nc, what + " Cb")
    return [_bits(ws), _bits(Qb), _bits(Cb)]


def _whole_step(B, Nc, d, q, c, y, mask, dev, what):
    import torch

    from dpr_scale_amd.hotpath import HipKernels

    kn = HipKernels()
    Qw, Qb = _guarded(B, d, dev)
    Cw, Cb = _guarded(Nc, d, dev)
    out = kn.inbatch_step_f32(q, c, Qb, Cb, y, 0, mask, 1.0, 1.0 / B, want_G=True)
    torch.cuda.synchronize()
    _guard_kept(Qw, B, what + " Qb")
    _guard_kept(Cw, Nc, what + " Cb")
    return [_bits(o) for o in out] + [_bits(Qb), _bits(Cb)]  # row_loss, row_lse, loss_sum, G, dQ, dC, Qb, Cb


@pytest.mark.parametrize("copy", [0, 1], ids=["small_sim_copy=0", "small_sim_copy=1"])
@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "column-mask"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_same_words_as_engine(name, masked, copy, dev, options):
    import numpy as np

    B, Nc, d = SHAPES[name]
    q, c, y, mask = _inputs(B, Nc, d, masked, dev, seed=B * 1000 + Nc + 5)
    options(0, copy)
    ref = _sim_stats(B, Nc, d, q, c, y, mask, dev, "engine sim_stats")
    ref_step = _whole_step(B, Nc, d, q, c, y, mask, dev, "engine step")
    assert np.array_equal(ref[0][:16], np.zeros(16, np.uint8)), "the sim launch clears the two header words"
    assert not np.array_equal(ref[1], np.full_like(ref[1], ref[1].flat[0])) and not np.array_equal(ref[2], np.full_like(ref[2], ref[2].flat[0]))
    options(1, copy)
    what = f"small_sim_copy={copy} {name}"
    _same(_sim_stats(B, Nc, d, q, c, y, mask, dev, what + " sim_stats"), ref, what + " sim_stats")
    _same(_whole_step(B, Nc, d, q, c, y, mask, dev, what + " step"), ref_step, what + " step")


@pytest.mark.parametrize("copy", [0, 1], ids=["small_sim_copy=0", "small_sim_copy=1"])
@pytest.mark.parametrize("d", [768, 1024])
def test_packed_one_rank_step_same_words_as_engine(d, copy, dev, options):
    """dprhot_inbatch_step_packed_f32 at W = 1: the bf16-context instantiation -- only the Q tiles have copy waves."""
    import torch

    from dpr_scale_amd.hotpath import HipKernels

    kn = HipKernels()
    W, B, K, T = 1, 32, 8, 0.5
    n_ctx = B * K
    gen = torch.Generator(device="cpu").manual_seed(179 + d)
    rows_c = kn.packed_rows(n_ctx, d)
    assert rows_c > n_ctx
    q = (torch.randn(B, d, generator=gen) * d ** -0.25).to(dev)
    assert not torch.equal(q.bfloat16().float(), q)
    c = (torch.randn(n_ctx, d, generator=gen) * d ** -0.25).to(dev)
    m = torch.rand(n_ctx, generator=gen) < 0.1
    m[torch.arange(B) * K] = False
    Cb = torch.empty((rows_c, d), dtype=torch.bfloat16, device=dev)
    kn.pack_ctx(c, m.to(torch.uint8).to(dev), Cb)
    Cb_before = _bits(Cb)
    y = (torch.arange(B) * K).to(torch.int64).to(dev)

    def step(what):
        Qw, Qb = _guarded(B, d, dev)
        out = kn.inbatch_step_packed_f32(q, Cb, Qb, W, 0, n_ctx, y, 1.0 / T, 1.0 / (T * W * B), want_G=True)
        torch.cuda.synchronize()
        _guard_kept(Qw, B, what + " Qb")
        return [_bits(o) for o in out] + [_bits(Qb), _bits(Cb)]

    options(0, copy)
    ref = step("engine")
    options(1, copy)
    got = step(f"small_sim_copy={copy} packed")
    _same(got, ref, f"small_sim_copy={copy} packed one-rank step")
    assert (got[-1] == Cb_before).all(), "the packed contexts are read, not written"
