"""The batch-32 step with the bf16 copies of its sim launch leaving as 16-byte write-through stores (csrc/sim_small.h: sms_copy_wave
with WT = 1, what option small_sim_copy = 1 launches) and as the 8-byte plain stores they had before (small_sim_copy = 2), against the bit
reference -- the GEMM engine's sim launch (small_sim = 0) and the unsplit step_small_kernel (small_step_roles = 0) -- in one process:
every output of the one-call step (row_loss, row_lse, loss_sum, G, dQ, dC, Qb, Cb) and the whole workspace dprhot_sim_stats_f32
leaves behind must be the SAME WORDS, with and without a column mask.  The write-through form pairs the copy waves' 8-byte pieces
across neighbouring lanes: the words and where they land may not change.  Shapes: the flagship, one ragged tile each way with fewer
context rows than a wave's 16 (clamped rows in both halves of a lane pair), 33 column tiles with a ragged last 32-block, four K
chunks; and the packed one-rank step (bf16 contexts: Q copies only, the loss stamped into dC[:, 0]).  Qb, Cb, dQ and dC are the first
rows of larger buffers filled with a pattern, and the rows behind them must keep it: a 16-byte store to a clamped row is seen."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

# B, Nc, d
SHAPES = {
    "cfg2": (32, 256, 768),
    "9x8x768-one-ragged-tile-each-way": (9, 8, 768),
    "32x528x768-three-chunks-ragged-32-block": (32, 528, 768),
    "32x256x1024-four-chunks": (32, 256, 1024),
}
GUARD = 24  # rows behind every guarded buffer: more than one 16-row tile
PATTERN = 7.0
OPTIONS = ("small_sim", "small_step_roles", "small_sim_copy")
FORMS = {"write-through": 1, "plain": 2}  # values of small_sim_copy: 16-byte sc1 stores (the default) | 8-byte plain stores
_REF = {}  # (shape name, masked) or "packed" -> the reference's words, computed once and never changed


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture()
def options():
    """Sets small_sim / small_step_roles / small_sim_copy for the duration of a test and restores the defaults."""
    from dpr_scale_amd import _lib

    defaults = {k: _lib.get_option(k) for k in OPTIONS}

    def set_all(sim, roles, copy):
        for k, v in zip(OPTIONS, (sim, roles, copy)):
            _lib.set_option(k, v)

    yield defaults, set_all
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


def _same(a, b, names, what):
    import numpy as np

    assert len(a) == len(b) == len(names)
    for k, x, y in zip(names, a, b):
        assert np.array_equal(x, y), f"{what} {k}: {int((x != y).sum())} of {x.size} words differ"


class _Guarded:
    """Buffers whose first rows a call is given; the rows behind them must still hold the pattern afterwards."""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def __call__(self, rows, d, dtype, name):
        import torch

        whole = torch.full((rows + GUARD, d), PATTERN, dtype=dtype, device=self.dev)
        self.all.append((name, whole, rows))
        return whole[:rows]

    def check(self, what):
        for name, whole, rows in self.all:
            assert bool((whole[rows:] == PATTERN).all()), f"{what} {name}: rows behind the buffer were written"


def _sim_stats(B, Nc, d, q, c, y, mask, dev, what):
    """dprhot_sim_stats_f32 into a workspace, Qb and Cb that start from a fixed byte pattern: (workspace, Qb, Cb)."""
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import _ptr

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = _lib.workspace_bytes(B, Nc, d)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    g = _Guarded(dev)
    Qb, Cb = g(B, d, torch.bfloat16, "Qb"), g(Nc, d, torch.bfloat16, "Cb")
    _lib.check(_lib.lib.dprhot_sim_stats_f32(_ptr(q), _ptr(c), _ptr(Qb), _ptr(Cb), B, Nc, d, _ptr(y), 0, _ptr(mask), 1.0, None,
                                             _ptr(ws), nbytes, st), "dprhot_sim_stats_f32")
    torch.cuda.synchronize()
    g.check(what)
    return [_bits(ws), _bits(Qb), _bits(Cb)]


STEP_NAMES = ("row_loss", "row_lse", "loss_sum", "G", "dQ", "dC", "Qb", "Cb")


def _whole_step(B, Nc, d, q, c, y, mask, dev, what):
    """dprhot_inbatch_step_f32 (the call of HipKernels.inbatch_step_f32) with guarded Qb, Cb, dQ and dC."""
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import _ptr

    f32 = torch.float32
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = _lib.workspace_bytes(B, Nc, d)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    g = _Guarded(dev)
    Qb, Cb = g(B, d, torch.bfloat16, "Qb"), g(Nc, d, torch.bfloat16, "Cb")
    dQ, dC = g(B, d, f32, "dQ"), g(Nc, d, f32, "dC")
    row_loss, row_lse, loss_sum = (torch.full((n,), PATTERN, dtype=f32, device=dev) for n in (B, B, 1))
    G = torch.full((B, Nc), PATTERN, dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.lib.dprhot_inbatch_step_f32(
        q.data_ptr(), _ptr(c), Qb.data_ptr(), Cb.data_ptr(), B, Nc, d, _ptr(y), 0, _ptr(mask), 1.0, 1.0 / B, 1.0, None, None, row_loss.data_ptr(),
        row_lse.data_ptr(), loss_sum.data_ptr(), _ptr(G), dQ.data_ptr(), dC.data_ptr(), ws.data_ptr(), nbytes, st), "dprhot_inbatch_step_f32")
    torch.cuda.synchronize()
    g.check(what)
    return [_bits(o) for o in (row_loss, row_lse, loss_sum, G, dQ, dC, Qb, Cb)]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "column-mask"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_same_words_as_reference(name, masked, form, dev, options):
    import numpy as np

    from dpr_scale_amd import _lib

    defaults, set_all = options
    B, Nc, d = SHAPES[name]
    q, c, y, mask = _inputs(B, Nc, d, masked, dev, seed=B * 1000 + Nc + 11)
    if (name, masked) not in _REF:
        set_all(0, 0, defaults["small_sim_copy"])
        sim = _sim_stats(B, Nc, d, q, c, y, mask, dev, "reference sim_stats")
        step = _whole_step(B, Nc, d, q, c, y, mask, dev, "reference step")
        assert np.array_equal(sim[0][:16], np.zeros(16, np.uint8)), "the sim launch clears the two header words"
        for k in (1, 2):  # Qb, Cb were written
            assert not np.array_equal(sim[k], np.full_like(sim[k], sim[k].flat[0]))
        for x in sim + step:
            x.setflags(write=False)
        _REF[(name, masked)] = (sim, step)
    ref_sim, ref_step = _REF[(name, masked)]
    assert defaults["small_sim"] == 1 and defaults["small_sim_copy"] == FORMS["write-through"]  # the library runs what is tested here
    set_all(defaults["small_sim"], defaults["small_step_roles"], FORMS[form])
    assert _lib.get_option("small_sim_copy") == FORMS[form]
    what = f"{form} copies {name}"
    _same(_sim_stats(B, Nc, d, q, c, y, mask, dev, what + " sim_stats"), ref_sim, ("workspace", "Qb", "Cb"), what + " sim_stats")
    _same(_whole_step(B, Nc, d, q, c, y, mask, dev, what + " step"), ref_step, STEP_NAMES, what + " step")


@pytest.mark.parametrize("form", list(FORMS))
def test_packed_one_rank_step_same_words_as_reference(form, dev, options):
    """dprhot_inbatch_step_packed_f32 at W = 1, 32 x 256 x 768: the bf16-context instantiation (only the Q tiles have copy waves) and
    the stamping launch (the lead dC workgroup puts the loss into column 0 of row n_ctx)."""
    import numpy as np
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import HipKernels

    defaults, set_all = options
    kn = HipKernels()
    W, B, K, T, d = 1, 32, 8, 0.5, 768
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
    f32 = torch.float32
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def step(what):
        nbytes = _lib.workspace_bytes(B, rows_c, d)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        g = _Guarded(dev)
        Qb, dQ, dC = g(B, d, torch.bfloat16, "Qb"), g(B, d, f32, "dQ"), g(rows_c, d, f32, "dC")
        row_loss, row_lse, loss_sum = (torch.full((n,), PATTERN, dtype=f32, device=dev) for n in (B, B, 1))
        G = torch.full((B, rows_c), PATTERN, dtype=torch.bfloat16, device=dev)
        _lib.check(_lib.lib.dprhot_inbatch_step_packed_f32(
            q.data_ptr(), Cb.data_ptr(), Qb.data_ptr(), B, W, 0, n_ctx, d, y.data_ptr(), 1.0 / T, 1.0 / (T * W * B), 1.0, None, row_loss.data_ptr(),
            row_lse.data_ptr(), loss_sum.data_ptr(), G.data_ptr(), dQ.data_ptr(), dC.data_ptr(), ws.data_ptr(), nbytes, st),
            "dprhot_inbatch_step_packed_f32")
        torch.cuda.synchronize()
        g.check(what)
        return [_bits(o) for o in (row_loss, row_lse, loss_sum, G, dQ, dC, Qb, Cb)]

    if "packed" not in _REF:
        set_all(0, 0, defaults["small_sim_copy"])
        ref = step("reference packed")
        stamped = ref[5].reshape(rows_c, d)[n_ctx, 0]
        assert stamped == ref[2][0] and stamped != 0, "the reference stamps its loss into dC[n_ctx][0]"
        for x in ref:
            x.setflags(write=False)
        _REF["packed"] = ref
    set_all(defaults["small_sim"], defaults["small_step_roles"], FORMS[form])
    got = step(f"{form} copies packed")
    _same(got, _REF["packed"], STEP_NAMES, f"{form} copies packed one-rank step")
    assert np.array_equal(got[-1], Cb_before), "the packed contexts are read, not written"
