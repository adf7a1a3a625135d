"""The lean row softmax of the role-split batch-32 step (csrc/step_small.h: ss_row_softmax / ss_load_slabs under step_small_kernel_roles
and step_small_kernel_out, option small_step_roles = 1, 2, 3) against the untouched step_small_kernel (small_step_roles = 0), in one
process.  The lean text drops selects, compares, address arithmetic and LDS lane exchanges and keeps every arithmetic instruction, so
every output of dprhot_inbatch_step_f32 -- dQ, dC, G, S_out, row_loss, row_lse, loss_sum -- must be the SAME WORDS as the reference
kernel's, for every form.  The shapes are the smallest at which each changed line can go wrong: the compile-time FULL path
(B == 32 and Nc == 256 * CPT) at one, two, three and four slabs and at CPT = 2, and the run-time path one row, one half and one
chunk short of it.  The slab count of a shape is read off the launched kernel's name (its second template argument)."""
import ctypes
import re

import pytest

NAMES = ["loss_sum", "row_loss", "row_lse", "G", "S_out", "dQ", "dC"]
FORMS = [3, 2, 1]
PATTERN = 3.0  # what every output buffer holds before the step

# B, Nc, d, masked fraction, slabs the plan map gives (NS), CPT
SHAPES = [
    pytest.param(32, 256, 768, 0.0, 3, 1, id="32x256x768-full-3-slabs-flagship"),
    pytest.param(32, 256, 256, 0.0, 1, 1, id="32x256x256-full-1-slab"),
    pytest.param(32, 256, 512, 0.0, 2, 1, id="32x256x512-full-2-slabs"),
    pytest.param(32, 256, 1024, 0.0, 4, 1, id="32x256x1024-full-4-slabs"),
    pytest.param(32, 512, 768, 0.0, 3, 2, id="32x512x768-full-cpt2"),
    pytest.param(31, 256, 768, 0.0, 3, 1, id="31x256x768-one-row-short"),
    pytest.param(17, 256, 768, 0.0, 3, 1, id="17x256x768-second-half-one-row"),
    pytest.param(32, 248, 768, 0.0, 3, 1, id="32x248x768-last-chunk-absent"),
    pytest.param(32, 264, 768, 0.0, 3, 2, id="32x264x768-cpt2-one-chunk"),
    pytest.param(32, 256, 768, 0.1, 3, 1, id="32x256x768-full-column-mask"),
    pytest.param(27, 248, 768, 0.1, 3, 1, id="27x248x768-column-mask"),
]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture()
def roles():
    """Sets the option for the duration of a test and restores the default."""
    from dpr_scale_amd import _lib

    default = _lib.get_option("small_step_roles")
    yield lambda v: _lib.set_option("small_step_roles", v)
    _lib.set_option("small_step_roles", default)


def _inputs(B, Nc, d, mask_frac, dev, seed):
    import torch

    gen = torch.Generator(device="cpu").manual_seed(seed)
    # (NOT bf16-representable: the rounding of both operands is part of what is compared)
    q = (torch.randn(B, d, generator=gen) * d ** -0.25).to(dev)
    c = (torch.randn(Nc, d, generator=gen) * d ** -0.25).to(dev)
    y = torch.randperm(Nc, generator=gen)[:B].to(torch.int64)
    m = torch.rand(Nc, generator=gen) < mask_frac
    m[y] = False
    return q, c, y, (m.to(torch.uint8) if mask_frac > 0 else None)


def _bits(t):
    import torch

    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().copy()


def _same(a, b, what, nan_aware=False):
    """Word for word.  nan_aware (the dead-row case only): NaN in the same places, every other word the same."""
    import numpy as np

    assert len(a) == len(b) == len(NAMES)
    for k, (x, y) in zip(NAMES, zip(a, b)):
        if nan_aware:
            if x.dtype == np.int16:  # bf16: exponent all ones, mantissa non-zero
                nx, ny = (x & 0x7F80 == 0x7F80) & (x & 0x007F != 0), (y & 0x7F80 == 0x7F80) & (y & 0x007F != 0)
            else:
                nx, ny = np.isnan(x.view(np.float32)), np.isnan(y.view(np.float32))
            assert np.array_equal(nx, ny), f"{what} {k}: NaN in {int(nx.sum())} places against {int(ny.sum())}"
            x, y = np.where(nx, 0, x), np.where(ny, 0, y)
        assert np.array_equal(x, y), f"{what} {k}: {int((x != y).sum())} of {x.size} words differ"


def _step(B, Nc, d, q, c, y, mask, dev, y_offset=0, T=1.0):
    """dprhot_inbatch_step_f32 with every optional output asked for, into buffers that start from a fixed pattern."""
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import _ptr

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f32, bf16 = torch.float32, torch.bfloat16
    y = y.to(dev)
    mask = mask.to(dev) if mask is not None else None
    nbytes = _lib.workspace_bytes(B, Nc, d)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    Qb = torch.full((B, d), 7.0, dtype=bf16, device=dev)
    Cb = torch.full((Nc, d), 7.0, dtype=bf16, device=dev)
    S = torch.full((B, Nc), PATTERN, dtype=f32, device=dev)
    rl, lse = torch.full((B,), PATTERN, dtype=f32, device=dev), torch.full((B,), PATTERN, dtype=f32, device=dev)
    ls = torch.full((1,), PATTERN, dtype=f32, device=dev)
    G = torch.full((B, Nc), PATTERN, dtype=bf16, device=dev)
    dQ, dC = torch.full((B, d), PATTERN, dtype=f32, device=dev), torch.full((Nc, d), PATTERN, dtype=f32, device=dev)
    _lib.check(_lib.lib.dprhot_inbatch_step_f32(_ptr(q), _ptr(c), _ptr(Qb), _ptr(Cb), B, Nc, d, _ptr(y), y_offset, _ptr(mask), 1.0 / T,
                                                1.0 / (T * B), 1.0, None, _ptr(S), _ptr(rl), _ptr(lse), _ptr(ls), _ptr(G), _ptr(dQ), _ptr(dC),
                                                _ptr(ws), nbytes, st),
               "dprhot_inbatch_step_f32")
    torch.cuda.synchronize()
    return [_bits(t) for t in (ls, rl, lse, G, S, dQ, dC)]


def _kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    return {n for n in names if "Memcpy" not in n and "Memset" not in n}


def _against_reference(B, Nc, d, q, c, y, mask, dev, roles, what, y_offset=0, nan_aware=False, check_ref=None):
    """One reference run (small_step_roles = 0), then every role-split form on the same inputs."""
    import numpy as np

    roles(0)
    ref = _step(B, Nc, d, q, c, y, mask, dev, y_offset)
    pat = np.float32(PATTERN).view(np.int32)
    for k in ("dQ", "dC"):
        assert not (ref[NAMES.index(k)] == pat).any(), f"the reference left elements of {k} unwritten"
    if check_ref is not None:
        check_ref(ref)
    for form in FORMS:
        roles(form)
        _same(_step(B, Nc, d, q, c, y, mask, dev, y_offset), ref, f"{what}, small_step_roles={form}", nan_aware)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc,d,mask_frac,ns,cpt", SHAPES)
def test_same_words_as_untouched_kernel(B, Nc, d, mask_frac, ns, cpt, dev, roles):
    import numpy as np

    q, c, y, mask = _inputs(B, Nc, d, mask_frac, dev, seed=B * 1000 + Nc + d)

    def finite(ref):
        dq, dc = ref[5].view(np.float32), ref[6].view(np.float32)
        assert np.isfinite(dq).all() and np.isfinite(dc).all() and np.abs(dq).max() > 0 and np.abs(dc).max() > 0

    _against_reference(B, Nc, d, q, c, y, mask, dev, roles, f"{B}x{Nc}x{d}", check_ref=finite)
    # the instantiation the shape is listed for: CPT and the slab count NS, as the plan map gives them, and the 32-column dQ tile
    roles(3)
    for _ in range(3):  # (a profiler session now and then returns without a single device event: ask again)
        k = _kernels(lambda: _step(B, Nc, d, q, c, y, mask, dev))
        if k:
            break
    got = [re.search(r"step_small_kernel_out<(\d+),\s*(\d+),\s*(\d+)>", n) for n in k]
    got = [tuple(int(x) for x in m.groups()) for m in got if m]
    assert got == [(cpt, ns, 32)], (sorted(k), got)


def _gold_case(Nc, gold, mask_cols, seed, dev):
    """Random inputs at 32 x Nc x 768 with the gold columns of the given rows set by hand."""
    import torch

    B, d = 32, 768
    q, c, y, _ = _inputs(B, Nc, d, 0.0, dev, seed)
    for r, col in gold.items():
        y[r] = col
    mask = None
    if mask_cols:
        mask = torch.zeros(Nc, dtype=torch.uint8)
        mask[list(mask_cols)] = 1
    return B, Nc, d, q, c, y, mask


@pytest.mark.gpu
@pytest.mark.parametrize("Nc", [256, 512])
def test_gold_column_at_the_edges_of_a_chunk_and_shared_in_a_wave(Nc, dev, roles):
    """Gold columns 0, 7, 8 and Nc - 1 (first and last element of a chunk, first element of the next lane, last lane), rows 4 and 5
    -- the two rows of wave 2 -- on ONE gold column, and, at Nc = 512 (two chunks per thread), rows 6 and 7 of wave 3 with gold
    columns in different chunks: 5 in the chunk of columns 0-255 and 300 in the chunk of columns 256-511, and rows 8 and 9 in the
    same lane's two chunks (columns 16 and 272: lane 2, elements 0)."""
    import numpy as np

    gold = {0: 0, 1: 7, 2: 8, 3: Nc - 1, 4: 100, 5: 100}
    if Nc == 512:
        gold.update({6: 5, 7: 300, 8: 16, 9: 272})
    B, Nc, d, q, c, y, mask = _gold_case(Nc, gold, (), 4100 + Nc, dev)

    def gold_is_negative(ref):  # G = (p - onehot) / B: the gold column is the one negative entry of its row
        import torch

        G = torch.from_numpy(ref[3]).view(torch.bfloat16).float().numpy()
        assert np.array_equal(np.argmin(G, axis=1), y.numpy()) and ((G < 0).sum(axis=1) == 1).all()

    _against_reference(B, Nc, d, q, c, y, mask, dev, roles, f"gold columns {gold} at Nc={Nc}", check_ref=gold_is_negative)


@pytest.mark.gpu
def test_masked_gold_column(dev, roles):
    """Row 6's gold column is masked: its gold logit is -inf, its loss +inf, its dScores entry (0 - 1) / B."""
    import numpy as np

    B, Nc, d, q, c, y, mask = _gold_case(256, {6: 50}, (50, 51, 200), 77, dev)

    def inf_loss(ref):
        rl = ref[1].view(np.float32)
        assert np.isposinf(rl[6]) and np.isfinite(np.delete(rl, 6)).all() and np.isposinf(ref[0].view(np.float32)[0])

    _against_reference(B, Nc, d, q, c, y, mask, dev, roles, "masked gold column", check_ref=inf_loss)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc", [(32, 256), (31, 264)])
def test_y_offset(B, Nc, dev, roles):
    d, off = 768, 37
    q, c, y, mask = _inputs(B, Nc, d, 0.0, dev, seed=B + Nc + 5)
    plain = _against_reference(B, Nc, d, q, c, y, mask, dev, roles, "y_offset = 0")
    shifted = _against_reference(B, Nc, d, q, c, y - off, mask, dev, roles, f"y_offset = {off}", y_offset=off)
    _same(shifted, plain, "y - off with y_offset = off against y")


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc", [(32, 256), (17, 248)])
def test_fully_masked_row_same_nan_pattern(B, Nc, dev, roles):
    """A dead row: row 5 of q is -inf against contexts that are all positive, so every slab holds -inf along that row -- max = -inf,
    sum = 0, dScores inf * 0 = NaN, logsumexp -inf + log(0).  NaN in the same places for both kernels, every other word the same."""
    import numpy as np
    import torch

    d = 768
    q, c, y, mask = _inputs(B, Nc, d, 0.1, dev, seed=97 + B)
    c = c.abs() + 1e-3
    q = q.clone()
    q[5] = float("-inf")

    def dead_row(ref):
        G = torch.from_numpy(ref[3]).view(torch.bfloat16).float().numpy()
        live = [r for r in range(B) if r != 5]
        assert np.isnan(G[5]).all() and np.isfinite(G[live]).all(), "the reference has the NaN row this test is about"
        assert np.isneginf(ref[2].view(np.float32)[5]), "logsumexp of the dead row is -inf"

    # (dC = G^T Q takes the dead row's NaN into EVERY element, however the row is made dead -- NaN x Q[5][k] is NaN for any Q -- so dC
    # is compared as all-NaN in both kernels; dQ's other rows, G, S_out, the row losses and logsumexps are compared word for word)
    _against_reference(B, Nc, d, q, c, y, mask, dev, roles, "one dead row", nan_aware=True, check_ref=dead_row)


@pytest.mark.gpu
def test_nan_logit_in_an_otherwise_masked_row_is_the_one_documented_difference(dev, roles):
    """The one input on which the lean softmax is NOT form 0 bit for bit ("the lean row softmax"): a row whose logits are
    -inf except for a NaN.  Row 5 of q is -inf, the contexts are positive except context 7, which is all zeros: logit [5][7] is
    -inf x 0 = NaN.  The row maximum ignores the NaN and is -inf in both kernels.  Form 0 then selects 0 for every exponential: sum 0,
    logsumexp -inf.  The lean text selects the subtrahend: exp(NaN - 0) = NaN reaches the sum, logsumexp NaN.  Everything else is NaN
    in the same places (the row's G and row loss, dQ's row 5, dC, loss_sum) and the same words elsewhere."""
    import numpy as np

    B, Nc, d = 32, 256, 768
    q, c, y, mask = _inputs(B, Nc, d, 0.0, dev, seed=131)
    c = c.abs() + 1e-3
    c[7] = 0.0
    q = q.clone()
    q[5] = float("-inf")
    assert int(y[5]) != 7
    roles(0)
    ref = _step(B, Nc, d, q, c, y, mask, dev)
    i = NAMES.index("row_lse")
    assert np.isnan(ref[NAMES.index("S_out")].view(np.float32).reshape(B, Nc)[5, 7]), "the NaN logit this test is about"
    assert np.isneginf(ref[i].view(np.float32)[5])
    for form in FORMS:
        roles(form)
        out = _step(B, Nc, d, q, c, y, mask, dev)
        lse = out[i].view(np.float32)
        assert np.isnan(lse[5]), f"small_step_roles={form}: logsumexp of the row is {lse[5]}"
        out[i] = out[i].copy()
        out[i][5] = ref[i][5]  # the documented difference, checked above; every other logsumexp must be the reference's word
        _same(out, ref, f"NaN logit in a masked row, small_step_roles={form}", nan_aware=True)


@pytest.mark.gpu
def test_packed_step_stamping_launch(dev, roles):
    """The packed step's stamping launch at 32 x 264 x 768 (W = 1: 256 contexts + the mask rows): form 2 with the loss in
    dC[n_ctx][0], whichever of forms 2 and 3 is asked for, against small_step_roles = 0."""
    import numpy as np
    import torch

    from dpr_scale_amd.hotpath import HipKernels

    kn = HipKernels()
    W, B, K, T, d = 1, 32, 8, 0.5, 768
    n_ctx = B * K
    gen = torch.Generator(device="cpu").manual_seed(177 + d)
    rows_c = kn.packed_rows(n_ctx, d)
    assert rows_c == 264
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
        return [_bits(o) for o in out]

    names = ["row_loss", "row_lse", "loss_sum", "G", "dQ", "dC"]
    roles(0)
    ref = step()
    stamp = ref[5].view(np.float32).reshape(rows_c, d)[n_ctx, 0]
    assert stamp == ref[2].view(np.float32)[0] and np.isfinite(stamp) and stamp != 0.0, "the loss stamp sits in dC[n_ctx][0]"
    for form in (2, 3):
        roles(form)
        out = step()
        for k, x, r in zip(names, out, ref):
            assert np.array_equal(x, r), f"packed step, small_step_roles={form} {k}: {int((x != r).sum())} of {x.size} words differ"
        for _ in range(3):
            k = _kernels(step)
            if k:
                break
        assert any(re.search(r"step_small_kernel_roles<2,\s*3,\s*32>", n) for n in k), sorted(k)
