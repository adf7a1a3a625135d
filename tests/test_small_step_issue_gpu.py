"""The priced row softmax of the role-split batch-32 step (csrc/step_small.h: ss_row_softmax on two-element vectors, the one-statement
row maximum ss_row32_max, the gold column through the addend of an fma) against the
untouched step_small_kernel (small_step_roles = 0), in one process: every output of dprhot_inbatch_step_f32 -- loss, row loss,
logsumexp, G, logits, dQ, dC -- as raw words, for forms 1, 2 and 3.  NaN-aware only where a row is dead.
The shapes are the smallest that reach each text (FULL: B == 32 and Nc == 256 * CPT, at three and four slabs and at CPT 2; the run-time
text one row, one chunk and most chunks short of it, at CPT 3 with a partial second half, and without a second half), the inputs are
chosen for what the rewrite can break: the gold column at every element of a chunk, in the first and the last chunk and in lanes 0, 15,
16 and 31 of a row; labels that are negative before y_offset; a masked column next to a gold one; a row whose maximum is its gold logit;
a fully masked row and the NaN-logit row of tests/test_small_step_lean.py; inv_T = 50 (most exponentials underflow); the device-side
scale given and NULL; the optional outputs asked for and NULL."""
import ctypes
import re

import pytest

NAMES = ["loss_sum", "row_loss", "row_lse", "G", "S_out", "dQ", "dC"]
FORMS = [3, 2, 1]
PATTERN = 3.0  # what every output buffer holds before the step
Y_OFFSET = 37
DEAD_ROW, NAN_ROW, NAN_COL, MAX_ROW = 3, 5, 7, 2

SHAPES = [
    pytest.param(32, 256, 768, id="32x256x768-full-cpt1-3-slabs"),
    pytest.param(32, 256, 1024, id="32x256x1024-full-4-slabs"),
    pytest.param(32, 512, 768, id="32x512x768-full-cpt2"),
    pytest.param(31, 256, 768, id="31x256x768-run-time"),
    pytest.param(32, 264, 768, id="32x264x768-run-time"),
    pytest.param(32, 64, 768, id="32x64x768-run-time"),
    pytest.param(17, 520, 768, id="17x520x768-run-time-cpt3-partial-second-half"),
    pytest.param(16, 256, 768, id="16x256x768-run-time-no-second-half"),
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


def _gold_columns(B, Nc):
    """Row r's gold column.  A row is 32 lanes, lane t holds the 8-column chunks t, t + 32, ...: every element 0-7 of the first chunk
    (lane 0) and of the last chunk, then one element each in lanes 15, 16 and 31 (where the row has that many chunks) and in the
    chunks behind the first 32; rows beyond the list start over.  16 x 256: lanes 16, 15, the last chunk and elements 2-7 of the first;
    17 x 520: lanes 31 + 32, 16 + 32, 15 + 32, 31, 16, 15, the last chunk, elements 5-7 of the first."""
    cand = list(range(8)) + [Nc - 8 + e for e in range(8)]
    for lane, e in ((15, 3), (16, 4), (31, 5), (15 + 32, 6), (16 + 32, 1), (31 + 32, 2)):
        col = lane * 8 + e
        if col < Nc - 8:
            cand.append(col)
    if B < len(cand):  # fewer rows than candidates: the END of the list, backwards, so that the lanes are there at 16 and 17 rows too
        cand = cand[-B:][::-1]
    gold = [cand[r % len(cand)] for r in range(B)]
    assert gold[NAN_ROW] != NAN_COL and min(gold) < Y_OFFSET
    return gold


def _inputs(B, Nc, d, dev, dead):
    """Positive contexts (so that a query row of -inf is a dead row), random queries, the gold columns of _gold_columns handed over as
    y - Y_OFFSET, one column masked right behind a gold one, row MAX_ROW aligned with its gold context.  dead: row DEAD_ROW fully
    masked (every logit -inf: its first component is -inf, and every context's is positive) and row NAN_ROW -inf except for a NaN at
    column NAN_COL (every component is -inf, and context NAN_COL is zero behind its first)."""
    import torch

    gen = torch.Generator(device="cpu").manual_seed(7 * B + Nc + d + int(dead))
    # logits: the part that varies along a row has a standard deviation of about 0.6 (1.2 with dead: there the step runs at inv_T = 50,
    # and exp(x - max) leaves the normal range 87 below the maximum, about 1.5 deviations of 60 with the maximum of 256 at 2.7)
    q = torch.randn(B, d, generator=gen) * d ** -0.25 * (2.0 if dead else 1.0)
    c = (torch.randn(Nc, d, generator=gen) * d ** -0.25).abs() + 1e-3
    gold = _gold_columns(B, Nc)
    y = torch.tensor(gold, dtype=torch.int64) - Y_OFFSET
    assert (y < 0).any()
    q[MAX_ROW] = 0.3 * c[gold[MAX_ROW]]  # (a margin of about 3 over the row: the gold probability stays well below 1)
    masked = next(col + 1 for col in gold if col + 1 < Nc and col + 1 not in gold and col + 1 != NAN_COL)
    mask = torch.zeros(Nc, dtype=torch.uint8)
    mask[masked] = 1
    if dead:
        c[NAN_COL] = 0.0
        c[NAN_COL, 0] = 1.0
        q[DEAD_ROW, 0] = float("-inf")  # -inf x a positive number in every column, context NAN_COL included
        q[NAN_ROW] = float("-inf")      # ... and -inf x 0 = NaN at context NAN_COL
        mask[NAN_COL] = 0
    return q.to(dev), c.to(dev), y.to(dev), mask.to(dev), gold, masked


def _bits(t):
    import torch

    if t is None:
        return None
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().copy()


def _wants_g(B, Nc, d):
    from dpr_scale_amd import _lib

    w = ctypes.c_int(1)
    _lib.check(_lib.lib.dprhot_step_wants_g(B, Nc, d, ctypes.byref(w)), "dprhot_step_wants_g")
    return w.value != 0


def _step(B, Nc, d, q, c, y, mask, dev, inv_T, scale, optional):
    """dprhot_inbatch_step_f32 into buffers that start from a fixed pattern.  scale: the device-side scale or None (NULL).  optional:
    whether the outputs the API lets a caller leave out are asked for (G is left out only where dprhot_step_wants_g allows it)."""
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import _ptr

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f32, bf16 = torch.float32, torch.bfloat16
    nbytes = _lib.workspace_bytes(B, Nc, d)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    Qb = torch.full((B, d), 7.0, dtype=bf16, device=dev)
    Cb = torch.full((Nc, d), 7.0, dtype=bf16, device=dev)
    S = torch.full((B, Nc), PATTERN, dtype=f32, device=dev) if optional else None
    rl = torch.full((B,), PATTERN, dtype=f32, device=dev) if optional else None
    lse = torch.full((B,), PATTERN, dtype=f32, device=dev) if optional else None
    G = torch.full((B, Nc), PATTERN, dtype=bf16, device=dev) if optional or _wants_g(B, Nc, d) else None
    ls = torch.full((1,), PATTERN, dtype=f32, device=dev)
    dQ, dC = torch.full((B, d), PATTERN, dtype=f32, device=dev), torch.full((Nc, d), PATTERN, dtype=f32, device=dev)

    def ptr(t):
        return _ptr(t) if t is not None else None

    _lib.check(_lib.lib.dprhot_inbatch_step_f32(_ptr(q), _ptr(c), _ptr(Qb), _ptr(Cb), B, Nc, d, _ptr(y), Y_OFFSET, _ptr(mask), inv_T,
                                                inv_T / B, 0.5, ptr(scale), ptr(S), ptr(rl), ptr(lse), _ptr(ls), ptr(G), _ptr(dQ),
                                                _ptr(dC), _ptr(ws), nbytes, st),
               "dprhot_inbatch_step_f32")
    torch.cuda.synchronize()
    return [_bits(t) for t in (ls, rl, lse, G, S, dQ, dC)]


def _is_nan(x):
    import numpy as np

    if x.dtype == np.int16:  # bf16: exponent all ones, mantissa non-zero
        return (x & 0x7F80 == 0x7F80) & (x & 0x007F != 0)
    return np.isnan(x.view(np.float32))


def _same(out, ref, what, nan_aware=False):
    """Word for word.  nan_aware (inputs with a dead row only): NaN in the same places, every other word the same."""
    import numpy as np

    for k, x, r in zip(NAMES, out, ref):
        assert (x is None) == (r is None), f"{what} {k}"
        if x is None:
            continue
        if nan_aware:
            nx, nr = _is_nan(x), _is_nan(r)
            assert np.array_equal(nx, nr), f"{what} {k}: NaN in {int(nx.sum())} places against {int(nr.sum())}"
            x, r = np.where(nx, 0, x), np.where(nr, 0, r)
        assert np.array_equal(x, r), f"{what} {k}: {int((x != r).sum())} of {x.size} words differ"


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc,d", SHAPES)
def test_live_rows_same_words_as_untouched_kernel(B, Nc, d, dev, roles):
    """Every row live: strict equality of every word, with the scale given and every output asked for, and with the scale NULL and
    the optional outputs left out."""
    import numpy as np
    import torch

    q, c, y, mask, gold, masked = _inputs(B, Nc, d, dev, dead=False)
    scale = torch.full((1,), 0.75, dtype=torch.float32, device=dev)
    for sc, optional in ((scale, True), (None, False)):
        roles(0)
        ref = _step(B, Nc, d, q, c, y, mask, dev, 1.0, sc, optional)
        if optional:  # the reference has what this test is about
            S = ref[NAMES.index("S_out")].view(np.float32).reshape(B, Nc)
            G = torch.from_numpy(ref[NAMES.index("G")]).view(torch.bfloat16).float().numpy().reshape(B, Nc)
            assert np.isneginf(S[:, masked]).all() and np.isfinite(np.delete(S, masked, axis=1)).all()
            assert np.array_equal(np.argmin(G, axis=1), np.array(gold)) and ((G < 0).sum(axis=1) == 1).all()
            assert int(np.argmax(S[MAX_ROW])) == gold[MAX_ROW]
            assert np.isfinite(ref[0].view(np.float32)).all()
        for k in ("dQ", "dC"):
            x = ref[NAMES.index(k)]
            assert not (x == np.float32(PATTERN).view(np.int32)).any() and not _is_nan(x).any(), f"the reference's {k}"
        for form in FORMS:
            roles(form)
            _same(_step(B, Nc, d, q, c, y, mask, dev, 1.0, sc, optional), ref, f"{B}x{Nc}x{d} optional={optional}, small_step_roles={form}")


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc,d", SHAPES)
def test_dead_row_nan_row_and_underflow(B, Nc, d, dev, roles):
    """inv_T = 50 with a fully masked row and the NaN-logit row.  The row maximum ignores the NaN and is -inf in every form; form 0
    then selects 0 for every exponential (logsumexp -inf) where the lean text selects the subtrahend (exp(NaN - 0) = NaN, logsumexp
    NaN): the one documented difference (tests/test_small_step_lean.py), set aside here after it has been checked.  Everything else:
    NaN in the same places, every other word the same."""
    import numpy as np

    import torch

    q, c, y, mask, gold, masked = _inputs(B, Nc, d, dev, dead=True)
    i = NAMES.index("row_lse")
    live = [r for r in range(B) if r not in (DEAD_ROW, NAN_ROW)]
    for sc in (None, torch.full((1,), 0.75, dtype=torch.float32, device=dev)):
        roles(0)
        ref = _step(B, Nc, d, q, c, y, mask, dev, 50.0, sc, True)
        S = ref[NAMES.index("S_out")].view(np.float32).reshape(B, Nc)
        assert np.isneginf(S[DEAD_ROW]).all() and np.isnan(S[NAN_ROW, NAN_COL]) and np.isneginf(np.delete(S[NAN_ROW], NAN_COL)).all()
        assert np.isneginf(ref[i].view(np.float32)[[DEAD_ROW, NAN_ROW]]).all()
        G = ref[NAMES.index("G")].reshape(B, Nc)
        assert _is_nan(G[DEAD_ROW]).all() and not _is_nan(G[live]).any()
        assert (G[live] & 0x7F80 == 0).mean() > 0.5, "at inv_T = 50 most probabilities underflow to a denormal or to zero"
        for form in FORMS:
            roles(form)
            out = _step(B, Nc, d, q, c, y, mask, dev, 50.0, sc, True)
            lse = out[i].view(np.float32)
            assert np.isnan(lse[NAN_ROW]) and np.isneginf(lse[DEAD_ROW]), f"small_step_roles={form}: logsumexp {lse[NAN_ROW]}, {lse[DEAD_ROW]}"
            out[i] = out[i].copy()
            out[i][NAN_ROW] = ref[i][NAN_ROW]
            _same(out, ref, f"{B}x{Nc}x{d} dead rows, scale {'given' if sc is not None else 'NULL'}, small_step_roles={form}", nan_aware=True)


def _kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    return {n for n in names if "Memcpy" not in n and "Memset" not in n}


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
    gen = torch.Generator(device="cpu").manual_seed(311 + d)
    rows_c = kn.packed_rows(n_ctx, d)
    assert rows_c == 264
    q = (torch.randn(B, d, generator=gen) * d ** -0.25).to(dev)
    c = (torch.randn(n_ctx, d, generator=gen) * d ** -0.25).to(dev)
    y = torch.tensor([(r * K + r) % n_ctx for r in range(B)], dtype=torch.int64)  # every element position of a chunk
    m = torch.rand(n_ctx, generator=gen) < 0.1
    m[y] = False
    Cb = torch.empty((rows_c, d), dtype=torch.bfloat16, device=dev)
    kn.pack_ctx(c, m.to(torch.uint8).to(dev), Cb)
    y = y.to(dev)

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
    for _ in range(3):  # form 3 is still set (a profiler session now and then returns without a single device event: ask again)
        k = _kernels(step)
        if k:
            break
    assert any(re.search(r"step_small_kernel_roles<2,\s*3,\s*32>", n) for n in k), sorted(k)
