"""Form 3 of the batch-32 step's softmax + backward launch (csrc/step_small.h: step_small_kernel_out, option small_step_roles = 3, the
default): the role split of form 2 with the loss, logsumexp, dScores and logits written by ONE output workgroup that has no product to
do, instead of by the dC workgroup of tile 0.  Every value keeps its instruction sequence -- the output workgroup runs the shared
softmax, and adds the row losses in a double, rows in ascending order, as the lead did -- so every output of dprhot_inbatch_step_f32
must be the SAME BITS as under small_step_roles = 0 (step_small_kernel), whatever is asked for.  A stamping launch (the packed step)
and the shapes outside the guard keep the kernels they had."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
NEW = "step_small_kernel_out"
# the launcher's dispatch: CPT in {1, 2, 3} (rows of up to 256 / 512 / 768 columns) x NS in {1, 2, 3, 4} (slabs) x QTW in {16, 32}
N_INST = 3 * 4 * 2


def test_output_kernel_has_no_scratch():
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
    mine = {k: v for k, v in rows.items() if NEW in k}
    assert len(mine) == N_INST, f"expected the {N_INST} instantiations of {NEW} in the report, found {sorted(mine)}"
    assert not any("step_small_kernel_roles" in k for k in mine), "the new kernel's name must not count as a step_small_kernel_roles"
    for name, r in mine.items():
        assert r == {"ScratchSize": 0, "VGPRs Spill": 0}, f"{name}: {r}"


# B, Nc, d, T, masked fraction
SHAPES = [
    pytest.param(32, 256, 768, 1.0, 0.0, id="cfg2"),
    pytest.param(32, 64, 768, 1.0, 0.0, id="32x64x768-cpt1-short-rows"),
    pytest.param(32, 528, 768, 1.0, 0.05, id="32x528x768-cpt3-masked"),
    pytest.param(32, 256, 1024, 1.0, 0.0, id="32x256x1024-4-slabs"),
    pytest.param(27, 248, 768, 0.05, 0.2, id="ragged-27x248-masked-T0.05"),
    pytest.param(9, 8, 768, 1.0, 0.0, id="9x8x768-second-half-empty"),
]
OUTSIDE = [
    pytest.param(32, 1032, 768, 0, id="32x1032x768-as-planned"),
    pytest.param(32, 1032, 768, 1, id="32x1032x768-single-slab"),
    pytest.param(64, 256, 768, 0, id="64x256x768-two-row-blocks"),
]
NAMES = ["loss_sum", "row_loss", "row_lse", "G", "S_out", "dQ", "dC"]
PATTERN = 3.0  # what every output buffer holds before the step


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
    return q, c, y.to(dev), (m.to(torch.uint8).to(dev) if mask_frac > 0 else None)


def _bits(t):
    import torch

    if t is None:
        return None
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().copy()


def _same(a, b, names, what):
    import numpy as np

    assert len(a) == len(b) == len(names)
    for k, (x, y) in zip(names, zip(a, b)):
        if x is None and y is None:
            continue
        assert np.array_equal(x, y), f"{what} {k}: {int((x != y).sum())} of {x.size} words differ"


def _step(B, Nc, d, T, q, c, y, mask, dev, optional=True):
    """dprhot_inbatch_step_f32 into buffers that start from a fixed pattern; optional = False: S_out, row_loss and row_lse are NULL."""
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
    ls = torch.full((1,), PATTERN, dtype=f32, device=dev)
    G = torch.full((B, Nc), PATTERN, dtype=bf16, device=dev)
    dQ, dC = torch.full((B, d), PATTERN, dtype=f32, device=dev), torch.full((Nc, d), PATTERN, dtype=f32, device=dev)
    _lib.check(_lib.lib.dprhot_inbatch_step_f32(_ptr(q), _ptr(c), _ptr(Qb), _ptr(Cb), B, Nc, d, _ptr(y), 0, _ptr(mask), 1.0 / T, 1.0 / (T * B),
                                                1.0, None, _ptr(S), _ptr(rl), _ptr(lse), _ptr(ls), _ptr(G), _ptr(dQ), _ptr(dC), _ptr(ws), nbytes, st),
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


def _no_pattern_left(out):
    import numpy as np

    pat = np.float32(PATTERN).view(np.int32)
    for k in ("dQ", "dC"):
        left = int((out[NAMES.index(k)] == pat).sum())
        assert left == 0, f"{left} elements of {k} still hold the buffer's initial pattern: a tile nobody wrote"


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc,d,T,mask_frac", SHAPES)
def test_same_bits_as_unsplit_kernel(B, Nc, d, T, mask_frac, dev, roles):
    import numpy as np

    q, c, y, mask = _inputs(B, Nc, d, mask_frac, dev, seed=B * 1000 + Nc + 11)
    roles(0)
    ref = _step(B, Nc, d, T, q, c, y, mask, dev)
    dq, dc = ref[5].view(np.float32), ref[6].view(np.float32)
    assert np.isfinite(dq).all() and np.isfinite(dc).all() and np.abs(dq).max() > 0 and np.abs(dc).max() > 0
    _no_pattern_left(ref)
    roles(3)
    out = _step(B, Nc, d, T, q, c, y, mask, dev)
    _no_pattern_left(out)
    _same(out, ref, NAMES, "small_step_roles=3")


@pytest.mark.gpu
def test_optional_outputs_absent(dev, roles):
    """S_out, row_loss and row_lse NULL: the output workgroup still writes loss_sum and G, and nothing through a NULL pointer."""
    B, Nc, d = 32, 64, 768
    q, c, y, mask = _inputs(B, Nc, d, 0.0, dev, seed=41)
    roles(0)
    ref = _step(B, Nc, d, 1.0, q, c, y, mask, dev, optional=False)
    full = _step(B, Nc, d, 1.0, q, c, y, mask, dev)
    roles(3)
    out = _step(B, Nc, d, 1.0, q, c, y, mask, dev, optional=False)
    assert out[1] is None and out[2] is None and out[4] is None
    _no_pattern_left(out)
    _same(out, ref, NAMES, "small_step_roles=3, optional outputs NULL")
    for k in ("loss_sum", "G", "dQ", "dC"):  # and asking for fewer outputs changes none of the others
        i = NAMES.index(k)
        _same([out[i]], [full[i]], [k], "small_step_roles=3, optional outputs NULL against all asked for")
    k3 = _kernels(lambda: _step(B, Nc, d, 1.0, q, c, y, mask, dev, optional=False))
    assert any(NEW in n for n in k3), sorted(k3)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["one-row", "every-column"])
def test_fully_masked_row_same_nan_pattern(how, dev, roles):
    """A row whose every logit is -inf: max = -inf, sum = 0, and the kernel yields inf * 0 = NaN for its dScores, as the reference
    does.  one-row: the column mask cannot single out a row, so row 5 of q is -inf against contexts that are all positive -- every
    product of that row is -inf in every slab.  every-column: the mask takes all columns, so every row is such a row."""
    import numpy as np
    import torch

    B, Nc, d = 27, 248, 768
    q, c, y, mask = _inputs(B, Nc, d, 0.2, dev, seed=97)
    if how == "one-row":
        c = c.abs() + 1e-3
        q = q.clone()
        q[5] = float("-inf")
    else:
        mask = torch.ones(Nc, dtype=torch.uint8, device=dev)
    roles(0)
    ref = _step(B, Nc, d, 1.0, q, c, y, mask, dev)
    G = torch.from_numpy(ref[3]).view(torch.bfloat16).float().numpy()
    dead = [5] if how == "one-row" else list(range(B))
    live = [r for r in range(B) if r not in dead]
    assert np.isnan(G[dead]).all() and np.isfinite(G[live]).all(), "the reference has the NaN rows this test is about"
    assert np.isnan(ref[0].view(np.float32)).all() or np.isinf(ref[0].view(np.float32)).all()
    roles(3)
    out = _step(B, Nc, d, 1.0, q, c, y, mask, dev)
    _no_pattern_left(out)
    _same(out, ref, NAMES, f"small_step_roles=3, {how} masked")


@pytest.mark.gpu
def test_default_takes_the_output_kernel_at_cfg2(dev):
    from dpr_scale_amd import _lib

    assert _lib.get_option("small_step_roles") == 3
    B, Nc, d = 32, 256, 768
    q, c, y, mask = _inputs(B, Nc, d, 0.0, dev, seed=5)
    _step(B, Nc, d, 1.0, q, c, y, mask, dev)  # (first launch outside the profiler)
    k = _kernels(lambda: _step(B, Nc, d, 1.0, q, c, y, mask, dev))
    assert any(NEW in n for n in k), sorted(k)
    assert not any("step_small_kernel_roles" in n for n in k), sorted(k)


@pytest.mark.gpu
def test_packed_step_keeps_the_lead(dev):
    """The stamping launch (dprhot_inbatch_step_packed_f32, W = 1): the loss goes into dC[n_ctx][0], whose owner needs the finished
    sum, so the launcher stays on step_small_kernel_roles at the default option."""
    import numpy as np
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import HipKernels

    assert _lib.get_option("small_step_roles") == 3
    kn = HipKernels()
    W, B, K, T, d = 1, 32, 8, 0.5, 768
    n_ctx = B * K
    gen = torch.Generator(device="cpu").manual_seed(177 + d)
    rows_c = kn.packed_rows(n_ctx, d)
    q = (torch.randn(B, d, generator=gen) * d ** -0.25).to(dev)
    c = (torch.randn(n_ctx, d, generator=gen) * d ** -0.25).to(dev)
    m = torch.rand(n_ctx, generator=gen) < 0.1
    m[torch.arange(B) * K] = False
    Cb = torch.empty((rows_c, d), dtype=torch.bfloat16, device=dev)
    kn.pack_ctx(c, m.to(torch.uint8).to(dev), Cb)
    y = (torch.arange(B) * K).to(torch.int64).to(dev)
    res = {}

    def step():
        Qb = torch.full((B, d), 7.0, dtype=torch.bfloat16, device=dev)
        res["out"] = kn.inbatch_step_packed_f32(q, Cb, Qb, W, 0, n_ctx, y, 1.0 / T, 1.0 / (T * W * B), want_G=True)
        torch.cuda.synchronize()

    step()
    k = _kernels(step)
    assert any("step_small_kernel_roles" in n for n in k) and not any(NEW in n for n in k), sorted(k)
    row_loss, row_lse, loss_sum, G, dQ, dC = res["out"]
    stamp = _bits(dC).reshape(rows_c, d)[n_ctx, 0]
    assert stamp == _bits(loss_sum)[0], "the loss stamp in dC[n_ctx][0] is loss_sum"
    val = np.int32(stamp).view(np.float32)
    assert np.isfinite(val) and val != 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc,d,no_skinny", OUTSIDE)
def test_outside_the_guard_same_kernel_and_bits(B, Nc, d, no_skinny, dev, roles):
    """Shapes of step_small_kernel that the role-split forms do not take.  The plan map gives 32 x 1032 x 768 to the few-rows plan
    (skinny.h takes B = 32 above 1024 columns), so that shape is run twice: as the library plans it, and with option no_skinny = 1,
    where it is step_small_kernel's single-slab plan -- the kernel this guard is about."""
    from dpr_scale_amd import _lib

    q, c, y, mask = _inputs(B, Nc, d, 0.05, dev, seed=B + Nc)
    _lib.set_option("no_skinny", no_skinny)
    try:
        roles(0)
        ref = _step(B, Nc, d, 1.0, q, c, y, mask, dev)
        _no_pattern_left(ref)
        k0 = _kernels(lambda: _step(B, Nc, d, 1.0, q, c, y, mask, dev))
        roles(3)
        _same(_step(B, Nc, d, 1.0, q, c, y, mask, dev), ref, NAMES, "small_step_roles=3 (outside the guard)")
        k = _kernels(lambda: _step(B, Nc, d, 1.0, q, c, y, mask, dev))
    finally:
        _lib.set_option("no_skinny", 0)
    assert k == k0, (sorted(k), sorted(k0))
    assert not any("step_small_kernel_roles" in n or NEW in n for n in k), sorted(k)
    if not (B == 32 and Nc == 1032 and no_skinny == 0):
        assert any("step_small_kernel" in n for n in k), sorted(k)


@pytest.mark.gpu
def test_fifty_steps_same_words(dev, roles):
    B, Nc, d = 32, 256, 768
    q, c, y, mask = _inputs(B, Nc, d, 0.0, dev, seed=23)
    roles(3)
    first = _step(B, Nc, d, 1.0, q, c, y, mask, dev)
    for it in range(1, 50):
        _same(_step(B, Nc, d, 1.0, q, c, y, mask, dev), first, NAMES, f"small_step_roles=3, step {it} against step 0")
