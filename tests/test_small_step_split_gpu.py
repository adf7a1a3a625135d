"""Form 3 of the batch-32 step's second launch with its output role split (csrc/step_small.h: a loss block and two row-store blocks in
front of the dC and dQ blocks) and the device-side scale read behind the operand loads: every output of dprhot_inbatch_step_f32 under
small_step_roles = 3 must be the SAME WORDS as under small_step_roles = 0 (step_small_kernel, untouched), whichever outputs are asked
for and however the scale arrives.  Every buffer starts from a pattern, and none of it may be left in dQ or dC (a tile nobody owns).

G == NULL: dprhot_inbatch_step_f32 refuses it at these shapes (dprhot_step_wants_g = 1: the plan materialises the dScores), so the
kernel's G == NULL path cannot be reached through the C ABI; that case asserts the refusal, the same under both forms, with nothing
written."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

NAMES = ["loss_sum", "row_loss", "row_lse", "G", "S_out", "dQ", "dC"]
PATTERN = 3.0  # what every output buffer holds before the step

# B, Nc, d, T, masked fraction
SHAPES = {
    "cfg2": (32, 256, 768, 1.0, 0.0),
    "32x64x768": (32, 64, 768, 1.0, 0.0),
    "32x528x768-masked": (32, 528, 768, 1.0, 0.05),
    "32x256x1024": (32, 256, 1024, 1.0, 0.0),
    "ragged-27x248-masked-T0.05": (27, 248, 768, 0.05, 0.2),
    "9x8x768-second-half-empty": (9, 8, 768, 1.0, 0.0),
    "17x40x768-one-row-in-second-half": (17, 40, 768, 1.0, 0.0),
}
# which optional outputs are NULL ("row" = row_loss and row_lse), then (d_scale, h_scale)
ABSENT = {
    "no-S_out": ({"S_out"}, None, 1.0),
    "no-row-stats": ({"row"}, None, 1.0),
    "only-G": ({"S_out", "row"}, None, 1.0),
    "d_scale-null": (set(), None, 1.0),
    "d_scale-0.37-h_scale-1.5": (set(), 0.37, 1.5),
}


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
    # (a label per row: fewer columns than rows -- 9 x 8 -- draws them with repetition)
    y = (torch.randperm(Nc, generator=gen)[:B] if Nc >= B else torch.randint(0, Nc, (B,), generator=gen)).to(torch.int64)
    m = torch.rand(Nc, generator=gen) < mask_frac
    m[y] = False
    return q, c, y.to(dev), (m.to(torch.uint8).to(dev) if mask_frac > 0 else None)


def _bits(t):
    import torch

    if t is None:
        return None
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().copy()


def _same(a, b, what):
    import numpy as np

    assert len(a) == len(b) == len(NAMES)
    for k, x, y in zip(NAMES, a, b):
        assert (x is None) == (y is None), f"{what} {k}"
        if x is not None:
            assert np.array_equal(x, y), f"{what} {k}: {int((x != y).sum())} of {x.size} words differ"


def _step(shape, inp, dev, absent=frozenset(), d_scale=None, h_scale=1.0, expect_rc0=True):
    """dprhot_inbatch_step_f32 into buffers that start from PATTERN: the words of NAMES (None for a NULL output), or the return code
    when the call is expected to be refused."""
    import torch

    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import _ptr

    B, Nc, d, T, _ = shape
    q, c, y, mask = inp
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f32, bf16 = torch.float32, torch.bfloat16
    nbytes = _lib.workspace_bytes(B, Nc, d)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    Qb = torch.full((B, d), 7.0, dtype=bf16, device=dev)
    Cb = torch.full((Nc, d), 7.0, dtype=bf16, device=dev)
    S = None if "S_out" in absent else torch.full((B, Nc), PATTERN, dtype=f32, device=dev)
    rl = None if "row" in absent else torch.full((B,), PATTERN, dtype=f32, device=dev)
    lse = None if "row" in absent else torch.full((B,), PATTERN, dtype=f32, device=dev)
    ls = torch.full((1,), PATTERN, dtype=f32, device=dev)
    G = None if "G" in absent else torch.full((B, Nc), PATTERN, dtype=bf16, device=dev)
    dQ, dC = torch.full((B, d), PATTERN, dtype=f32, device=dev), torch.full((Nc, d), PATTERN, dtype=f32, device=dev)
    ds = None if d_scale is None else torch.full((1,), d_scale, dtype=f32, device=dev)
    rc = _lib.lib.dprhot_inbatch_step_f32(_ptr(q), _ptr(c), _ptr(Qb), _ptr(Cb), B, Nc, d, _ptr(y), 0, _ptr(mask), 1.0 / T, 1.0 / (T * B),
                                          ctypes.c_float(h_scale), _ptr(ds), _ptr(S), _ptr(rl), _ptr(lse), _ptr(ls), _ptr(G), _ptr(dQ), _ptr(dC),
                                          _ptr(ws), nbytes, st)
    torch.cuda.synchronize()
    out = [_bits(t) for t in (ls, rl, lse, G, S, dQ, dC)]
    if not expect_rc0:
        return rc, out
    _lib.check(rc, "dprhot_inbatch_step_f32")
    return out


def _no_pattern_left(out):
    import numpy as np

    pat = np.float32(PATTERN).view(np.int32)
    for k in ("dQ", "dC"):
        left = int((out[NAMES.index(k)] == pat).sum())
        assert left == 0, f"{left} elements of {k} still hold the buffer's initial pattern: a tile nobody wrote"


_CACHE = {}


def _case(name, dev, roles):
    """Inputs and the words of the unsplit kernel (small_step_roles = 0) for a shape: made once, shared, never written to."""
    if name not in _CACHE:
        shape = SHAPES[name]
        B, Nc, d, _, mask_frac = shape
        inp = _inputs(B, Nc, d, mask_frac, dev, seed=B * 1000 + Nc + 29)
        roles(0)
        ref = _step(shape, inp, dev)
        for a in ref:
            a.setflags(write=False)
        _CACHE[name] = (shape, inp, ref)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_same_words_as_unsplit_kernel(name, dev, roles):
    import numpy as np

    shape, inp, ref = _case(name, dev, roles)
    dq, dc = ref[5].view(np.float32), ref[6].view(np.float32)
    assert np.isfinite(dq).all() and np.isfinite(dc).all() and np.abs(dq).max() > 0 and np.abs(dc).max() > 0
    _no_pattern_left(ref)
    roles(3)
    out = _step(shape, inp, dev)
    _no_pattern_left(out)
    _same(out, ref, f"small_step_roles=3 {name}")


@pytest.mark.parametrize("how", list(ABSENT))
@pytest.mark.parametrize("name", ["cfg2", "17x40x768-one-row-in-second-half"])
def test_optional_outputs_and_scale(name, how, dev, roles):
    import numpy as np

    absent, d_scale, h_scale = ABSENT[how]
    shape, inp, full = _case(name, dev, roles)
    roles(0)
    ref = _step(shape, inp, dev, absent, d_scale, h_scale)
    roles(3)
    out = _step(shape, inp, dev, absent, d_scale, h_scale)
    _no_pattern_left(out)
    _same(out, ref, f"small_step_roles=3 {name} {how}")
    if d_scale is None:  # asking for fewer outputs changes none of the others
        for k, x, y in zip(NAMES, out, full):
            if x is not None:
                assert np.array_equal(x, y), f"{name} {how}: {k} differs from the step that asks for everything"
    else:  # and the scale is applied: it is no power of two, so dQ differs from the unscaled step's
        assert not np.array_equal(out[5], full[5])


@pytest.mark.parametrize("also", ["G-alone", "G-S_out-row-stats"])
@pytest.mark.parametrize("name", ["cfg2", "17x40x768-one-row-in-second-half"])
def test_null_g_is_refused_alike(name, also, dev, roles):
    import numpy as np

    from dpr_scale_amd import _lib

    shape, inp, _ = _case(name, dev, roles)
    assert _lib.step_wants_g(*shape[:3]), "this shape's plan materialises the dScores"
    absent = {"G"} if also == "G-alone" else {"G", "S_out", "row"}
    res = {}
    for form in (0, 3):
        roles(form)
        res[form] = _step(shape, inp, dev, absent, expect_rc0=False)
        rc, out = res[form]
        assert rc != 0, f"small_step_roles={form}: G == NULL accepted"
        pat32, = np.float32(PATTERN).view(np.int32).reshape(1)
        for k, x in zip(NAMES, out):
            if x is not None:
                assert (x == pat32).all(), f"small_step_roles={form}: {k} written by a refused call"
    assert res[0][0] == res[3][0]


def test_fifty_steps_same_words(dev, roles):
    shape, inp, ref = _case("cfg2", dev, roles)
    roles(3)
    for it in range(50):
        _same(_step(shape, inp, dev), ref, f"small_step_roles=3, step {it}")
