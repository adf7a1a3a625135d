"""hotpath.router_head (csrc/router_head.h) on the GPU against the fp64 oracle of tests/_router_head_oracle.py and against what the
reference's own encoders returned (tests/golden/router_head_*.npz).  The logits are multiples of 1/64 in [-4, 4): ties are frequent (the
tie rules are exercised), 1 + x is exact in fp32 and distinct values' logs lie far apart (ids and argmax compare exactly).

Bars (from the issue that introduced the head): ids / argmax / router_mask exact; router_repr and expert_weights within
2^-23 + 2^-22 |ref| (one rounding of 1 + x plus a few ulp of the logarithm); softmax_sum within 1e-5 ref; gradients within 1e-5 of
max |ref grad| per element for fp32 logits, plus one rounding of the output dtype (2^-8 / 2^-11 relative; for fp16 also 2^-25 absolute,
its subnormal half-spacing) for bf16 / fp16."""
import math

import numpy as np
import pytest
import torch

import _router_head_oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# fp16 has subnormals from 2^-14 down (spacing 2^-24): one rounding there is up to 2^-25 ABSOLUTE, which no relative figure covers -- the
# softmax term of a 30522-wide row lies almost entirely in that range.  bf16 has fp32's exponent range and needs no such term.
SUBNORMAL = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}


def _np(t):
    return t.detach().double().cpu().numpy()


def _check_forward(ret, arg, ref, k, want_softmax, dtype=torch.float32):
    out_ulp = ULP[dtype]
    for key in ("router_repr",) + (("expert_weights",) if k else ()):
        got, want = _np(ret[key]), ref[key]
        err = np.abs(got - want)
        print(f"{key}: max |err| {err.max():.3e}, max |ref| {np.abs(want).max():.3e}")
        assert (err <= 2.0 ** -23 + (2.0 ** -22 + out_ulp) * np.abs(want)).all(), key
    assert np.array_equal(arg.cpu().numpy(), ref["argmax"])
    if k:
        assert ret["expert_ids"].dtype == torch.int64 and np.array_equal(ret["expert_ids"].cpu().numpy(), ref["expert_ids"])
        if dtype == torch.float32:
            assert np.array_equal(_np(ret["router_mask"]), ref["router_mask"])
            # (a torch mean over B in fp32: an exact integer sum, one rounding of the division)
            assert abs(_np(ret["avg_cond_num_experts"]) - ref["avg_cond_num_experts"]) <= 2.0 ** -23 * ref["avg_cond_num_experts"]
            assert np.array_equal(_np(ret["avg_marg_num_experts"]), ref["avg_marg_num_experts"])
    else:
        assert "expert_ids" not in ret and "router_mask" not in ret
    if want_softmax:
        got, want = _np(ret["router_softmax_repr"]), ref["router_softmax_repr"]
        print(f"softmax_sum: max rel err {(np.abs(got - want) / want).max():.3e}")
        assert (np.abs(got - want) <= (1e-5 + out_ulp) * want).all()
    else:
        assert "router_softmax_repr" not in ret


def _head_with_argmax(logits, mask, k, skip, want_softmax=True):
    """router_head plus the argmax table the autograd function keeps for its backward (read through the kernels object)."""
    from dpr_scale_amd.hotpath import default_kernels, router_head

    ret = router_head(logits, mask, topk=k, skip_first=skip, want_softmax=want_softmax)
    m8 = (mask != 0).to(torch.uint8).contiguous()
    arg = default_kernels().router_head_fwd(logits.detach(), m8, k, skip, want_softmax)[1]
    return ret, arg


# (B, T, V, k, skip): every value of V {8, 509, 1024, 30522}, T {1, 2, 31, 33, 180}, B {1, 5}, k {0, 1, 3, 8}, skip {0, 1}; V = 8 with
# k = 8; 1024 and 1025.. sit on both sides of the one-value-per-thread row form, 30522 takes the 32-value form
SWEEP = [(1, 1, 8, 8, 0), (5, 2, 8, 8, 1), (5, 33, 509, 3, 1), (5, 31, 1024, 1, 0), (1, 2, 1024, 0, 1), (5, 180, 509, 8, 1),
         (1, 33, 1030, 3, 1), (1, 31, 30522, 8, 1), (5, 2, 30522, 1, 0), (1, 180, 4099, 1, 1)]


@pytest.mark.parametrize("B,T,V,k,skip", SWEEP)
def test_forward_matches_the_fp64_oracle(B, T, V, k, skip):
    rng = np.random.default_rng(B * 1000003 + T * 1009 + V + k)
    x, m = O.grid_logits(rng, B, T + skip, V), O.masks(rng, B, T + skip)
    ref = O.forward(x, m, k=k, skip=skip)
    ret, arg = _head_with_argmax(torch.from_numpy(x).to(DEV), torch.from_numpy(m).to(DEV), k, skip)
    _check_forward(ret, arg, ref, k, True)
    assert ret["router_repr"].dtype == torch.float32


def _grads(rng, B, T, V, k):
    """Incoming gradients on a grid (multiples of 1/8 in [-2, 2]): exact in bf16 and fp16, so the cast autograd applies to the
    gradient of a half-width output changes nothing and the oracle sees the values the kernel sees."""
    return tuple((rng.integers(-16, 17, size=s) / 8.0).astype(np.float32) for s in ((B, V), (B, T, k), (B, V)))


def _run_backward(x, m, k, skip, g, want_softmax=True):
    """dlogits of sum(out * g) for the given subset of incoming gradients (None = absent)."""
    from dpr_scale_amd.hotpath import router_head

    tl = x.clone().requires_grad_(True)
    ret = router_head(tl, m, topk=k, skip_first=skip, want_softmax=want_softmax)
    terms = []
    for key, w in zip(("router_repr", "expert_weights", "router_softmax_repr"), g):
        if w is not None:
            terms.append((ret[key].float() * torch.from_numpy(w).to(DEV)).sum())
    sum(terms).backward()
    return tl.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,T,V,k,skip", [(3, 5, 509, 3, 1), (3, 3, 1500, 1, 0), (2, 2, 30522, 8, 1)])
def test_gradients_match_the_fp64_oracle(B, T, V, k, skip, dtype):
    rng = np.random.default_rng(V + k + B)
    m = O.masks(rng, B, T + skip)
    x = torch.from_numpy(O.grid_logits(rng, B, T + skip, V)).to(DEV).to(dtype)  # the grid is exact in bf16 and fp16
    xw = x.float().cpu().numpy()
    tm = torch.from_numpy(m).to(DEV)
    ref_fwd = O.forward(xw, m, k=k, skip=skip)
    g = _grads(rng, B, T, V, k)
    got = {}
    for name, sel in (("router", (0,)), ("weights", (1,)), ("soft", (2,)), ("all", (0, 1, 2))):
        gs = [w if i in sel else None for i, w in enumerate(g)]
        d = _run_backward(x, tm, k, skip, gs)
        assert d.dtype == dtype and d.shape == x.shape
        ref = O.backward(xw, m, ref_fwd, *gs, skip=skip)
        err = np.abs(_np(d) - ref)
        print(f"{dtype} {name}: max |err| {err.max():.3e}, max |ref| {np.abs(ref).max():.3e}")
        assert (err <= 1e-5 * np.abs(ref).max() + ULP[dtype] * np.abs(ref) + SUBNORMAL[dtype]).all(), name
        assert not d[:, :skip].any()
        got[name] = d
    dead = torch.from_numpy(m == 0).to(DEV)
    dead[:, :skip] = False
    assert dead.any() and torch.equal(got["all"][dead], got["soft"][dead])  # masked tokens: exactly the softmax term
    both = _run_backward(x, tm, k, skip, [g[0], g[1], None])
    assert torch.equal(both, _run_backward(x, tm, k, skip, [g[0], g[1], None], want_softmax=False))


@pytest.mark.parametrize("name", ["router_head_citadel_k1", "router_head_citadel_k3", "router_head_splade"])
def test_reference_fixture(name):
    from dpr_scale_amd.hotpath import router_head

    meta, z = load_golden(name)
    k, skip = meta["k"], meta["skip"]
    tl = torch.from_numpy(z["logits"]).to(DEV).requires_grad_(True)
    tm = torch.from_numpy(z["attention_mask"]).to(DEV)
    ret = router_head(tl, tm, topk=k, skip_first=skip, want_softmax=k > 0)
    keys = ["router_repr"] + (["expert_weights", "router_softmax_repr"] if k else [])
    for key in keys:
        want, got = z["ret_" + key].astype(np.float64), _np(ret[key])
        bar = 1e-5 * want if key == "router_softmax_repr" else 2.0 ** -23 + 2.0 ** -22 * np.abs(want)
        assert (np.abs(got - want) <= bar).all(), key
    if k:
        live = z["ret_expert_weights"] > 0
        assert np.array_equal(ret["expert_ids"].cpu().numpy()[live], z["ret_expert_ids"][live])
        assert np.array_equal(_np(ret["router_mask"]), z["ret_router_mask"])
        for key in ("avg_cond_num_experts", "avg_marg_num_experts"):
            assert ret[key].shape == (1, 1) and abs(_np(ret[key]) - z["ret_" + key]) <= 2.0 ** -23 * z["ret_" + key]
    sum((ret[key] * torch.from_numpy(z["g_" + key]).to(DEV)).sum() for key in keys).backward()
    ref = z["dlogits"].astype(np.float64)
    assert (np.abs(_np(tl.grad) - ref) <= 1e-5 * np.abs(ref).max()).all()


def test_encoders_return_the_fixture_keys_shapes_and_dtypes():
    from dpr_scale_amd.models.citadel_model import CITADELEncoder
    from dpr_scale_amd.models.splade_model import SPLADEEncoder

    meta, z = load_golden("router_head_citadel_k3")
    B, T1, V, H = meta["B"], meta["T1"], meta["V"], meta["H"]
    arch = dict(vocab_size=V, hidden_size=H, num_hidden_layers=1, num_attention_heads=2, intermediate_size=32, max_position_embeddings=32)
    torch.manual_seed(0)
    tokens = {"input_ids": torch.randint(0, V, (B, T1)).to(DEV), "attention_mask": torch.from_numpy(z["attention_mask"]).to(DEV)}
    enc = CITADELEncoder(arch, dropout=0.0).to(DEV)
    ret = enc(tokens, topk=meta["k"], add_cls=True)
    want = {key[4:]: v for key, v in z.items() if key.startswith("ret_")}
    assert sorted(ret) == sorted(want)
    for key, v in want.items():
        assert tuple(ret[key].shape) == v.shape, key
        assert ret[key].dtype == torch.from_numpy(v).dtype, key
    ret["router_repr"].sum().backward()
    assert any(p.grad is not None for p in enc.transformer.parameters())
    assert tuple(CITADELEncoder(arch, tok_projection_dim=4, cls_projection_dim=6).to(DEV)(tokens, topk=1, add_cls=True)["expert_repr"].shape) == (B, T1 - 1, 4)
    _, zs = load_golden("router_head_splade")
    rep = SPLADEEncoder(arch, dropout=0.0).to(DEV)(tokens)
    assert tuple(rep.shape) == zs["ret_router_repr"].shape and rep.dtype == torch.float32 and rep.requires_grad
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CITADELEncoder(arch)({k_: v.cpu() for k_, v in tokens.items()})


GUARD = 4096
PATTERN = 0xA5


class _Guards:
    """The method of tests/test_guard_bands.py: every HIP tensor torch.empty hands out is the interior of a byte buffer of PATTERN."""

    def __init__(self):
        self.orig = torch.empty
        self.regions = []

    def empty(self, *size, dtype=None, device=None, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        dev = torch.device(device) if device is not None else None
        size = tuple(int(x) for x in size)
        if dev is None or dev.type != "cuda" or kw:
            return self.orig(size, dtype=dtype, device=device, **kw)
        dt = dtype if dtype is not None else torch.get_default_dtype()
        n = int(math.prod(size)) * self.orig((), dtype=dt).element_size()
        if n == 0:
            return self.orig(size, dtype=dtype, device=device)
        raw = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=dev)
        self.regions.append((raw, n))
        return raw[GUARD:GUARD + n].view(dt).view(size)

    def check(self, what):
        torch.cuda.synchronize()
        for raw, n in self.regions:
            assert bool((raw[:GUARD] == PATTERN).all()), f"{what}: bytes BEFORE a {n}-byte buffer were overwritten"
            assert bool((raw[GUARD + n:] == PATTERN).all()), f"{what}: bytes BEHIND a {n}-byte buffer were overwritten"
        count, self.regions = len(self.regions), []
        return count


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("B,T1,V,k", [(3, 6, 509, 3), (2, 4, 30522, 8), (2, 5, 1027, 1)])
def test_strided_logits_and_guard_bands(B, T1, V, k, dtype, monkeypatch):
    """A [:, 1:, :] view and a column slice of a wider buffer (odd offset: rows aligned to the element only) give the bits of the
    contiguous call; every output and the exactly-sized workspace stay inside their guard bands."""
    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import HipKernels

    rng = np.random.default_rng(V)
    full = torch.from_numpy(O.grid_logits(rng, B, T1 + 1, V + 11)).to(DEV).to(dtype)
    tm = torch.from_numpy(O.masks(rng, B, T1)).to(DEV)
    m8 = (tm != 0).to(torch.uint8)
    views = {"contiguous": full[:, 1:, 3:3 + V].contiguous(), "token view": full[:, 1:, 3:3 + V].contiguous(),
             "column slice": full[:, 1:, 3:3 + V]}
    tmp = torch.zeros((B, T1 + 1, V), dtype=dtype, device=DEV)
    tmp[:, 1:] = views["contiguous"]
    views["token view"] = tmp[:, 1:, :]
    assert not views["column slice"].is_contiguous() and not views["token view"].is_contiguous()
    g = _Guards()
    kn = HipKernels()
    gr, gw, gs = (torch.from_numpy(a).to(DEV) for a in _grads(rng, B, T1 - 1, V, k))
    monkeypatch.setattr(torch, "empty", g.empty)
    outs = {}
    for name, x in views.items():
        fwd = kn.router_head_fwd(x, m8, k, 1, True)
        assert fwd[6].numel() == _lib.router_head_workspace_bytes(B, T1 - 1, V, k, True)
        dx = kn.router_head_bwd(x, m8, k, 1, fwd[1], fwd[3], fwd[6], gr, gw, gs)
        dx2 = kn.router_head_bwd(x, m8, k, 1, fwd[1], fwd[3], fwd[6], gr, gw, None)
        outs[name] = fwd[:6] + (dx, dx2)
    monkeypatch.undo()
    assert g.check(f"router head {B}x{T1}x{V}") == 3 * 9
    for name in ("token view", "column slice"):
        for a, b in zip(outs["contiguous"], outs[name]):
            assert torch.equal(a, b), name


def test_two_runs_are_bit_identical_and_nothing_vocabulary_by_token_sized_is_allocated():
    from dpr_scale_amd.hotpath import router_head

    B, T1, V, k = 4, 65, 30522, 5
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((B, T1, V), generator=gen, device=DEV)
    tm = torch.ones((B, T1), dtype=torch.long, device=DEV)
    tm[1, 40:] = 0
    g = [torch.randn(s, generator=gen, device=DEV) for s in ((B, V), (B, T1 - 1, k), (B, V))]
    runs = []
    for _ in range(2):
        tl = x.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ret = router_head(tl, tm, topk=k)
        (ret["router_repr"] * g[0]).sum().add((ret["expert_weights"] * g[1]).sum()).add((ret["router_softmax_repr"] * g[2]).sum()).backward()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base - tl.grad.numel() * 4
        print(f"peak above inputs and dlogits: {extra / 2 ** 20:.2f} MiB; one [B, T, V] fp32 tensor: {B * (T1 - 1) * V * 4 / 2 ** 20:.2f} MiB")
        assert extra < B * (T1 - 1) * V * 4
        runs.append([ret[key] for key in sorted(ret)] + [tl.grad])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_nan_and_inf_logits():
    """a NaN logit has f = 0 (it never outranks a positive) and makes the softmax of its row NaN; a +inf logit
    has f = +inf (it wins its row's top-1 and its column's max) and makes the softmax of its row NaN.  Ids and argmax stay in range."""
    from dpr_scale_amd.hotpath import router_head

    B, T1, V, k = 3, 6, 509, 3
    rng = np.random.default_rng(9)
    x = O.grid_logits(rng, B, T1, V)
    x[0, 2, 100] = np.nan
    x[1, 3, 7] = np.inf
    tl = torch.from_numpy(x).to(DEV).requires_grad_(True)
    tm = torch.ones((B, T1), dtype=torch.long, device=DEV)
    ret, arg = _head_with_argmax(tl, tm, k, 1)
    ids = ret["expert_ids"]
    assert int(ids.min()) >= 0 and int(ids.max()) < V and int(arg.min()) >= 0 and int(arg.max()) < T1 - 1
    assert torch.isfinite(ret["router_repr"][0]).all() and torch.isfinite(ret["expert_weights"][0]).all()
    assert 100 not in ids[0, 1].tolist()                                    # the NaN column is an ordinary zero
    assert ret["router_repr"][1, 7] == math.inf and int(arg[1, 7]) == 2 and int(ids[1, 2, 0]) == 7
    assert ret["expert_weights"][1, 2, 0] == math.inf
    soft = ret["router_softmax_repr"]
    assert torch.isnan(soft[0]).all() and torch.isnan(soft[1]).all() and torch.isfinite(soft[2]).all()
    clean = O.forward(np.where(np.isfinite(x), x, 0.0), tm.cpu().numpy(), k=k, skip=1)
    assert np.array_equal(ids[2].cpu().numpy(), clean["expert_ids"][2])
    (ret["router_repr"][2].sum() + ret["expert_weights"][2].sum()).backward()
    assert torch.isfinite(tl.grad).all()                                    # without a softmax gradient nothing non-finite spreads


def _torch_head(logits, attention_mask, k):
    """The reference's formulation in torch ops (citadel_model.py:50-73)."""
    x = logits[:, 1:, :]
    am = attention_mask[:, 1:]
    full = torch.log(1 + torch.relu(x)) * am.unsqueeze(-1)
    w, ids = torch.topk(full, dim=2, k=k)
    rm = torch.zeros_like(full).scatter_(dim=2, index=ids, src=(w > 0.).to(w.dtype)).sum(1)
    return {"router_repr": full.max(1).values, "expert_ids": ids, "expert_weights": w, "router_mask": rm,
            "router_softmax_repr": torch.softmax(x, dim=-1).sum(1)}


def test_task_step_on_router_head_dicts():
    from types import SimpleNamespace

    from dpr_scale_amd.hotpath import router_head
    from dpr_scale_amd.task.citadel_task import MultiVecRetrieverTask

    B, M, T1, V, k = 4, 2, 7, 509, 2
    task = MultiVecRetrieverTask(query_topk=k, context_topk=k, query_expert_load_loss_coef=0.01, context_expert_load_loss_coef=0.02,
                                 query_router_marg_load_loss_coef=0.03, context_router_marg_load_loss_coef=0.04, transform=None,
                                 model=None, datamodule=None, optim=None)
    task.trainer = SimpleNamespace(strategy=object(), max_epochs=1)
    rng = np.random.default_rng(3)
    # distinct positives per sequence (multiples of 1/1024 in [-8, 8)): torch.topk / max of the torch arm are defined everywhere
    def logits(n):
        return torch.from_numpy(np.stack([rng.permutation(16384)[: T1 * V].reshape(T1, V) - 8192 for _ in range(n)]).astype(np.float32) / 1024).to(DEV)
    xq, xc = logits(B), logits(B * M)
    mq, mc = torch.from_numpy(O.masks(rng, B, T1)).to(DEV), torch.from_numpy(O.masks(rng, B * M, T1)).to(DEV)
    mq[-1, :3] = 1  # (no fully masked sequence here: its all-zero router vector is a degenerate in-batch row)
    mc[-1, :3] = 1
    mask = torch.zeros(B * M, dtype=torch.bool, device=DEV)
    pos = (torch.arange(B) * M).to(DEV)
    grads = {}
    for arm in ("fused", "torch"):
        lq, lc = xq.clone().requires_grad_(True), xc.clone().requires_grad_(True)
        if arm == "fused":
            qr, cr = router_head(lq, mq, topk=k), router_head(lc, mc, topk=k)
        else:
            qr, cr = _torch_head(lq, mq, k), _torch_head(lc, mc, k)
        loss = task.compute_loss(qr, cr, mask, pos, None)
        assert torch.isfinite(loss)
        loss.backward()
        grads[arm] = (lq.grad, lc.grad)
    for got, want in zip(grads["fused"], grads["torch"]):
        assert float(want.abs().max()) > 0
        err = (got - want).abs().max()
        print(f"task step: max |err| {float(err):.3e}, max |ref| {float(want.abs().max()):.3e}")
        assert float(err) <= 1e-5 * float(want.abs().max())
