"""The role-split form of the batch-32 step's softmax + backward launch (csrc/step_small.h: step_small_kernel_roles, option
small_step_roles) against the kernel it replaces (small_step_roles = 0), in one process: every output of dprhot_inbatch_step_f32 --
loss_sum, row_loss, row_lse, G, S_out, dQ, dC -- must be the SAME BITS, for every form the option can select.  The new kernel keeps
the softmax's lane partition and instruction sequence, the 8 K slices of dQ and their order of addition, and one MFMA from a zero
accumulator per 16-context block of dC; only which workgroup does what has changed.  Shapes outside the guard (32 x 1032: the
single-slab plan; 64 x 256: two row blocks) run step_small_kernel under both settings and are listed so that the guard cannot start
taking them unnoticed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
FORMS = [1, 2]


def test_new_kernel_has_no_scratch():
    """Every instantiation of step_small_kernel_roles (3 row lengths x 4 slab counts x 2 dQ tile widths): no scratch, no spill."""
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
    mine = {k: v for k, v in rows.items() if "step_small_kernel_roles" in k}
    assert len(mine) == 24, f"expected the 24 instantiations of step_small_kernel_roles in the report, found {sorted(mine)}"
    for name, r in mine.items():
        assert r == {"ScratchSize": 0, "VGPRs Spill": 0}, f"{name}: {r}"


# B, Nc, d, T, masked fraction
SHAPES = [
    pytest.param(32, 256, 768, 1.0, 0.0, id="cfg2"),
    pytest.param(32, 64, 768, 1.0, 0.0, id="32x64x768"),
    pytest.param(32, 528, 768, 1.0, 0.05, id="32x528x768-masked"),
    pytest.param(32, 256, 1024, 1.0, 0.0, id="32x256x1024"),
    pytest.param(27, 248, 768, 0.05, 0.2, id="ragged-27x248-masked-T0.05"),
    pytest.param(9, 8, 768, 1.0, 0.0, id="9x8x768-second-half-empty"),
]
OUTSIDE = [
    pytest.param(32, 1032, 768, id="32x1032x768-single-slab"),
    pytest.param(64, 256, 768, id="64x256x768-two-row-blocks"),
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
    return q, c, y.to(dev), (m.to(torch.uint8).to(dev) if mask_frac > 0 else None)


def _bits(t):
    import torch

    if t is None:
        return None
    t = t.contiguous()
    return t.view(torch.uint8).cpu().numpy().copy() if t.dtype == torch.uint8 else t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().copy()


def _same(a, b, names, what):
    import numpy as np

    assert len(a) == len(b) == len(names)
    for k, (x, y) in zip(names, zip(a, b)):
        assert np.array_equal(x, y), f"{what} {k}: {int((x != y).sum())} of {x.size} words differ"


NAMES = ["loss_sum", "row_loss", "row_lse", "G", "S_out", "dQ", "dC"]


def _step(B, Nc, d, T, q, c, y, mask, dev):
    """dprhot_inbatch_step_f32 with every optional output asked for, into buffers that start from a fixed pattern."""
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import _ptr

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f32, bf16 = torch.float32, torch.bfloat16
    nbytes = _lib.workspace_bytes(B, Nc, d)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    Qb = torch.full((B, d), 7.0, dtype=bf16, device=dev)
    Cb = torch.full((Nc, d), 7.0, dtype=bf16, device=dev)
    S = torch.full((B, Nc), 3.0, dtype=f32, device=dev)
    rl, lse, ls = torch.full((B,), 3.0, dtype=f32, device=dev), torch.full((B,), 3.0, dtype=f32, device=dev), torch.full((1,), 3.0, dtype=f32, device=dev)
    G = torch.full((B, Nc), 3.0, dtype=bf16, device=dev)
    dQ, dC = torch.full((B, d), 3.0, dtype=f32, device=dev), torch.full((Nc, d), 3.0, dtype=f32, device=dev)
    _lib.check(_lib.lib.dprhot_inbatch_step_f32(_ptr(q), _ptr(c), _ptr(Qb), _ptr(Cb), B, Nc, d, _ptr(y), 0, _ptr(mask), 1.0 / T, 1.0 / (T * B),
                                                1.0, None, _ptr(S), _ptr(rl), _ptr(lse), _ptr(ls), _ptr(G), _ptr(dQ), _ptr(dC), _ptr(ws), nbytes, st),
               "dprhot_inbatch_step_f32")
    torch.cuda.synchronize()
    return [_bits(t) for t in (ls, rl, lse, G, S, dQ, dC)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc,d,T,mask_frac", SHAPES)
def test_step_same_bits_as_unsplit_kernel(B, Nc, d, T, mask_frac, dev, roles):
    import numpy as np

    q, c, y, mask = _inputs(B, Nc, d, mask_frac, dev, seed=B * 1000 + Nc + 7)
    roles(0)
    ref = _step(B, Nc, d, T, q, c, y, mask, dev)
    dq, dc = ref[5].view(np.float32), ref[6].view(np.float32)
    assert np.isfinite(dq).all() and np.isfinite(dc).all() and np.abs(dq).max() > 0 and np.abs(dc).max() > 0
    assert not (dq == 3.0).any() and not (dc == 3.0).any(), "the reference wrote every element of dQ and dC"
    for form in FORMS:
        roles(form)
        _same(_step(B, Nc, d, T, q, c, y, mask, dev), ref, NAMES, f"small_step_roles={form}")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [768, 1024])
def test_packed_step_same_bits_with_loss_stamp(d, dev, roles):
    """dprhot_inbatch_step_packed_f32 with W = 1 at a shape of the small step: the lead workgroup stamps the finished loss into
    dC[n_ctx][0] (the packed step: StepCtx::packed.stamp_src set), behind the one barrier only that workgroup keeps."""
    import numpy as np
    import torch

    from dpr_scale_amd.hotpath import HipKernels

    kn = HipKernels()
    W, B, K, T = 1, 32, 8, 0.5
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

    def step():
        Qb = torch.full((B, d), 7.0, dtype=torch.bfloat16, device=dev)
        out = kn.inbatch_step_packed_f32(q, Cb, Qb, W, 0, n_ctx, y, 1.0 / T, 1.0 / (T * W * B), want_G=True)
        torch.cuda.synchronize()
        return [_bits(o) for o in out] + [_bits(Qb)]

    names = ["row_loss", "row_lse", "loss_sum", "G", "dQ", "dC", "Qb"]
    roles(0)
    ref = step()
    stamp = ref[5].view(np.float32).reshape(rows_c, d)[n_ctx, 0]
    assert stamp == ref[2].view(np.float32)[0] and np.isfinite(stamp) and stamp != 0.0, "the loss stamp sits in dC[n_ctx][0]"
    for form in FORMS:
        roles(form)
        _same(step(), ref, names, f"small_step_roles={form} packed step")
        k = _kernels(step)
        assert any("step_small_kernel_roles" in n for n in k), f"the packed step at {B} x {rows_c} x {d} did not take the role-split kernel: {sorted(k)}"


def _kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    return {n for n in names if "Memcpy" not in n and "Memset" not in n}


@pytest.mark.gpu
def test_guard_takes_cfg2(dev, roles):
    """The positive of the two tests below: at 32 x 256 x 768 the option does change the kernel."""
    B, Nc, d = 32, 256, 768
    q, c, y, mask = _inputs(B, Nc, d, 0.0, dev, seed=5)
    seen = {}
    for form in [0] + FORMS:
        roles(form)
        _step(B, Nc, d, 1.0, q, c, y, mask, dev)  # (first launch outside the profiler)
        seen[form] = _kernels(lambda: _step(B, Nc, d, 1.0, q, c, y, mask, dev))
    assert all(seen.values()), "the profiler recorded no device activity"
    assert not any("step_small_kernel_roles" in n for n in seen[0]) and any("step_small_kernel" in n for n in seen[0]), seen[0]
    for form in FORMS:
        assert any("step_small_kernel_roles" in n for n in seen[form]), (form, seen[form])
    assert seen[1] != seen[2], "the two forms are different instantiations"


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nc,d", OUTSIDE)
def test_outside_the_guard_same_kernel_and_bits(B, Nc, d, dev, roles):
    q, c, y, mask = _inputs(B, Nc, d, 0.05, dev, seed=B + Nc)
    roles(0)
    ref = _step(B, Nc, d, 1.0, q, c, y, mask, dev)
    k0 = _kernels(lambda: _step(B, Nc, d, 1.0, q, c, y, mask, dev))
    for form in FORMS:
        roles(form)
        _same(_step(B, Nc, d, 1.0, q, c, y, mask, dev), ref, NAMES, f"small_step_roles={form} (outside the guard)")
        k = _kernels(lambda: _step(B, Nc, d, 1.0, q, c, y, mask, dev))
        assert k == k0, (form, sorted(k), sorted(k0))
        assert not any("step_small_kernel_roles" in n for n in k), sorted(k)
