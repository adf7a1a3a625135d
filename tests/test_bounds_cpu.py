"""The element-wise checker of tests/_bounds.py checked on CPU: an fp32 emulation of each rounding model must score well inside its
bounds, and each injected kernel bug far outside them -- while the suite's older bar (1e-2 of max |grad|) passes every one of those
bugs.  Then the plan table: the shapes just inside and just outside every dispatch gate of the training step, with the host-side plan
queries pinned (no GPU needed) so that a re-tune that moves a boundary fails here and names the row to move."""
import math

import pytest
import torch

import _bounds as BD

B, NC, D, T = 256, 2056, 128, 1.0  # Nc % 64 == 8: the last 64-deep K step of the dQ GEMM is a partial one of 8 contexts
STRIP = 64
GRAD_BAR = 1e-2  # tests/test_gpu_parity.py GRAD_RTOL: gradients within 1e-2 of max |grad|
FAITHFUL_MAX = 0.5
BUG_MIN = 10.0


def _problem(seed=3):
    gen = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, D, generator=gen) * D ** -0.25).to(torch.bfloat16).float()
    c = (torch.randn(NC, D, generator=gen) * D ** -0.25).to(torch.bfloat16).float()
    y = torch.randint(0, NC, (B,), generator=gen)
    mask = torch.rand(NC, generator=gen) < 0.05
    mask[NC - 8:] = False
    mask[y[B // 2:]] = False  # golds of the first half may be masked (loss +inf, G = -gs there)
    return q, c, y, mask


def _free_col(y, mask):
    taken = set(y.tolist())
    return next(j for j in range(7, NC) if j not in taken and not bool(mask[j]))


def _rne_bf16(x):
    return x.to(torch.bfloat16).float()


def _trunc_bf16(x):
    return (x.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)


def _slab_matmul(a, b, slabs):
    """fp32 a @ b with the contraction cut into `slabs` partial sums added in fp32 afterwards (split-K)."""
    K = a.shape[1]
    step = -(-K // slabs)
    out = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k0 in range(0, K, step):
        out = out + a[:, k0:k0 + step] @ b[k0:k0 + step]
    return out


def _emulate(model, q, c, y, mask, bug=None):
    """fp32 emulation of one plan of the step: forward, rounding at the model's point, split-K backward.  `bug` injects one kernel bug."""
    inv_T = float(torch.tensor(1.0 / T, dtype=torch.float32))
    gs = inv_T / B
    rows = torch.arange(B)
    S = (q @ c.T) * inv_T
    if bug == "drop_col":
        S[:, _free_col(y, mask)] = -math.inf  # the sim kernel loses one (unmasked, nobody's gold) context column
    S[:, mask] = -math.inf
    nt = -(-NC // STRIP)
    Sp = torch.nn.functional.pad(S, (0, nt * STRIP - NC), value=-math.inf).view(B, nt, STRIP)
    m_s = Sp.max(2).values
    mf = torch.where(torch.isfinite(m_s), m_s, torch.zeros_like(m_s))
    num = torch.exp(Sp - mf[..., None])
    s_s = num.sum(2)
    m_stored = m_s.clone()
    if bug == "strip":
        m_stored[:, 3] = m_s[:, 3] * 1.01  # one strip's statistic (its max) 1 % off
    msf = torch.where(torch.isfinite(m_stored), m_stored, torch.zeros_like(m_stored))
    M = m_stored.max(1).values
    Mf = torch.where(torch.isfinite(M), M, torch.zeros_like(M))
    tot = (s_s * torch.exp(msf - Mf[:, None]) * torch.isfinite(m_stored)).sum(1)
    lse = Mf + torch.log(tot)
    lse = torch.where(torch.isfinite(M), lse, torch.full_like(lse, -math.inf))
    if bug == "lse_block":
        lse[-64:] += 4e-3  # the last 64-row block's logsumexp off
    gold = S[rows, y]
    loss = lse - gold
    out = dict(row_lse=lse, row_loss=loss, loss_sum=float(loss.double().sum()))
    lsef = torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))
    rnd = _trunc_bf16 if bug == "trunc" else _rne_bf16
    onehot = torch.zeros(B, NC)
    onehot[rows, y] = 1.0
    if bug == "ragged_gold":
        onehot[B - 1, y[B - 1]] = 0.0  # the ragged last row loses its gold term
    if model in ("bf16_g", "bf16_g_f16num"):
        if model == "bf16_g":
            P = torch.exp(S - lsef[:, None])
        else:
            num16 = (num * 16384.0).to(torch.float16).float() * (1.0 / 16384.0)
            P = (num16 * torch.exp(msf - lsef[:, None])[..., None]).reshape(B, nt * STRIP)[:, :NC]
        P = torch.where(torch.isfinite(S) & torch.isfinite(lse)[:, None], P, torch.zeros_like(P))
        G = rnd((P - onehot) * gs)
        if bug == "masked":
            G[0, torch.nonzero(mask)[0, 0]] = G[0, 1]  # a gradient on a masked column
        Gf = G
    else:  # sk_tile_bf16: every 128-column tile's own softmax in bf16, gold column 0, gold term in fp32, tile factor in fp32
        W = 128
        ntt = -(-NC // W)
        St = torch.nn.functional.pad(S, (0, ntt * W - NC), value=-math.inf).view(B, ntt, W)
        mt = St.max(2).values
        mtf = torch.where(torch.isfinite(mt), mt, torch.zeros_like(mt))
        e = torch.exp(St - mtf[..., None])
        st = e.sum(2)
        tl = torch.where(torch.isfinite(mt), mtf + torch.log(st), torch.full_like(mt, -math.inf))
        Pt = rnd(e * (1.0 / st)[..., None]).reshape(B, ntt * W)[:, :NC]
        if bug == "strip":
            tl[:, 3] = tl[:, 3] * 1.01  # one tile's statistic 1 % off
        fac = torch.where(torch.isfinite(tl), torch.exp(tl - lsef[:, None]), torch.zeros_like(tl))
        Pt[rows, y] = 0.0
        if bug == "masked":
            Pt[0, torch.nonzero(mask)[0, 0]] = Pt[0, 1]
        Gf = gs * (Pt.view(B, -1)[:, :NC] * torch.nn.functional.pad(fac, (0, 0)).repeat_interleave(W, 1)[:, :NC])
        pg = torch.where(torch.isfinite(gold), torch.exp(gold - lsef), torch.zeros_like(gold))
        gterm = (pg - onehot[rows, y]) * gs  # (ragged_gold: the -1 of that row is lost)
        Gf[rows, y] = gterm
        G = None
    Gc = Gf.clone()
    if bug == "kstep_drop":
        Gc[:, NC - 8:] = 0.0  # the partial last K step of the dQ GEMM skipped
    if bug == "kstep_twice":
        Gc[:, NC - 8:] *= 2.0  # ... or counted twice
    out["dQ"] = _slab_matmul(Gc, c, 16)
    out["dC"] = Gf.T @ q
    out["G"] = G
    return out


MODELS = ["bf16_g", "bf16_g_f16num", "sk_tile_bf16"]
BUGS = ["trunc", "strip", "lse_block", "drop_col", "kstep_drop", "kstep_twice", "ragged_gold", "masked"]


def _scores(model, bug):
    q, c, y, mask = _problem()
    out = _emulate(model, q, c, y, mask, bug)
    inv_T = float(torch.tensor(1.0 / T, dtype=torch.float32))
    ref = BD.forward(q, c, y, mask.to(torch.uint8), inv_T, inv_T / B, f16=(model == "bf16_g_f16num"))
    sc, n_amb = BD.check_step(ref, row_loss=out["row_loss"], row_lse=out["row_lse"], loss_sum=out["loss_sum"], G=out["G"], dQ=out["dQ"],
                              dC=out["dC"], q=q, c=c, model=model, slabs_q=16)
    return sc, n_amb, out, ref


def _old_bar(out, ref, model, q, c):
    """The suite's older gradient bar: max |err| / max |ref| against the fp64 gradients of the exact softmax."""
    Gr = ref["G"]
    dQ = Gr @ c.double()
    dC = Gr.T @ q.double()
    e = [float((out["dQ"].double() - dQ).abs().max() / dQ.abs().max()), float((out["dC"].double() - dC).abs().max() / dC.abs().max())]
    return max(e)


@pytest.mark.parametrize("model", MODELS)
def test_faithful_emulation_is_well_inside_the_bounds(model):
    sc, n_amb, _, _ = _scores(model, None)
    print(f"[bound-ratio] emulation {model}: " + " ".join(f"{k} {v:.3g}" for k, v in sc.items()) + f"; ambiguous {n_amb}")
    assert max(sc.values()) <= FAITHFUL_MAX, sc
    assert n_amb > 0  # the inputs do reach rounding midpoints: the ambiguity rule is exercised


# Caught, but not by the factor of 10 (measured 5.0 and 4.3): on the two-pass plan a strip's maximum only enters the row logsumexp,
# weighted by the strip's share of the row (64 of 2056 columns); where G stays inside the kernel, truncation only shows through the
# gradients, next to the 2^-7 allowance of every ambiguous element.  These two stay above WEAK_MIN.
KNOWN_WEAK = {("bf16_g", "strip"), ("sk_tile_bf16", "trunc")}
WEAK_MIN = 3.0


@pytest.mark.parametrize("bug", BUGS)
@pytest.mark.parametrize("model", MODELS)
def test_injected_bug_is_far_outside_the_bounds(model, bug):
    sc, _, out, ref = _scores(model, bug)
    worst = max(sc.values())
    print(f"[bound-ratio] emulation {model} + {bug}: worst {worst:.3g} ({max(sc, key=sc.get)})")
    assert worst >= (WEAK_MIN if (model, bug) in KNOWN_WEAK else BUG_MIN), sc


@pytest.mark.parametrize("bug", BUGS)
@pytest.mark.parametrize("model", MODELS)
def test_the_older_gradient_bar_passes_the_injected_bug(model, bug):
    """Documents the gap these bounds close: 1e-2 of max |grad| passes every injected bug but the missing gold term of a row (that
    one moves the row's gradient by its largest term)."""
    q, c, _, _ = _problem()
    _, _, out, ref = _scores(model, bug)
    old = _old_bar(out, ref, model, q, c)
    if bug == "ragged_gold":
        assert old >= GRAD_BAR
    else:
        assert old < GRAD_BAR


def test_ambiguous_elements_may_round_either_way_but_not_further():
    """The G rule itself: at an ambiguous element the neighbour one ulp away passes and two ulps away fail; at a clear element one
    ulp away fails."""
    G = torch.tensor([[1.0 + 2 ** -8 + 1e-9, 1.0 + 2 ** -7 - 2 ** -10]], dtype=torch.float64)  # (first: just above a midpoint; second: clear)
    ref = dict(G=G, dG=torch.tensor([[1e-6, 1e-6]], dtype=torch.float64), mask=torch.zeros(2, dtype=torch.bool),
               yg=torch.tensor([1]))
    up = 1.0 + 2 ** -7
    for k, expect in [([1.0, 1.0], [True, False]), ([up, up], [True, True]), ([1.0 + 2 ** -6, 1.0 - 2 ** -8], [False, False])]:
        sc, amb = BD.g_scores(torch.tensor([k], dtype=torch.float64), ref)
        assert (sc[0] <= 1).tolist() == expect, (k, sc)
    assert amb.tolist() == [[True, False]]


def test_non_finite_patterns_must_match():
    q = torch.tensor([[1.0, 0.0], [0.0, 1.0]])
    c = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 0.0]])
    y = torch.tensor([0, 1])
    mask = torch.tensor([1, 0, 0, 1], dtype=torch.uint8)  # row 0's gold is masked: loss +inf
    ref = BD.forward(q, c, y, mask, 1.0, 0.5)
    assert math.isinf(float(ref["loss"][0])) and math.isfinite(float(ref["loss"][1]))
    assert ref["G"][0, 0] == -0.5 and ref["G"][0, 3] == 0.0
    assert BD.score_rows(ref["loss"].float(), ref["loss"], ref["e_loss"]) <= 1.0
    bad = ref["loss"].clone()
    bad[0] = 1e30
    assert BD.score_rows(bad, ref["loss"], ref["e_loss"]) == math.inf
    allm = BD.forward(q, c, y, torch.ones(4, dtype=torch.uint8), 1.0, 0.5)  # nothing unmasked: lse -inf, loss NaN, G = -gs at the gold
    assert torch.isneginf(allm["lse"]).all() and torch.isnan(allm["loss"]).all()
    assert allm["G"][0].tolist() == [-0.5, 0.0, 0.0, 0.0]
    assert BD.score_rows(allm["loss"], allm["loss"], allm["e_loss"]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# Plan table: every gate of the training step's dispatcher (csrc/dprhot.hip, default options), a shape just inside it and one just
# outside, with what the host-side plan queries answer: (fwd_one_pass, fwd_no_logits, step_wants_g, train_dq_slabs).  Gates that no
# query exposes (small_step_ok, wide_bwd_ok, pair128_use, big_bwd_ok, the long-axis rules) are pinned all the same: their rows are the
# shapes tests/test_plan_map.py runs on the GPU.  A re-tune that moves a boundary fails here -- move the row with it.
PLAN_TABLE = [
    ("small_step_ok rows", (32, 1152, 768), (0, 0, 1, 9), (33, 1152, 768), (0, 0, 1, 0)),
    ("small_step_ok two row blocks", (64, 256, 768), (0, 0, 1, 0), (65, 256, 768), (0, 0, 1, 0)),
    ("small_step_ok columns (32 rows)", (32, 1152, 768), (0, 0, 1, 9), (32, 1160, 768), (0, 0, 1, 10)),
    ("small_step_ok columns (64 rows)", (64, 256, 768), (0, 0, 1, 0), (64, 264, 768), (0, 0, 1, 0)),
    ("sk_plan rows", (128, 2048, 768), (0, 0, 1, 8), (160, 2048, 768), (2, 0, 1, 0)),
    ("sk_plan B % 32", (96, 2048, 768), (0, 0, 1, 8), (80, 2048, 768), (0, 0, 1, 0)),
    ("sk_plan d", (128, 2048, 1024), (0, 0, 1, 8), (128, 2048, 1152), (0, 0, 1, 0)),
    ("sk_plan d % 128", (128, 2048, 256), (0, 0, 1, 32), (128, 2048, 320), (0, 0, 1, 0)),
    ("sk_plan min columns (<= 64 rows)", (64, 512, 768), (0, 0, 1, 0), (64, 504, 768), (0, 0, 1, 0)),
    ("sk_plan min columns (> 64 rows)", (128, 256, 768), (0, 0, 1, 0), (128, 248, 768), (0, 0, 1, 0)),
    ("sk_plan max columns", (128, 16384, 768), (0, 0, 1, 10), (128, 16392, 768), (0, 0, 1, 0)),
    ("sk_fused", (128, 4096, 768), (0, 0, 0, 0), (128, 4088, 768), (0, 0, 1, 10)),
    ("wide_bwd_ok", (128, 1536, 4096), (0, 0, 1, 0), (128, 1544, 4096), (0, 0, 1, 0)),
    ("nl_ok tiles", (1024, 8192, 768), (2, 1, 1, 0), (1024, 7936, 768), (2, 0, 1, 0)),
    ("big_ok 256 tiles", (4096, 4096, 768), (1, 1, 1, 0), (4096, 3840, 768), (1, 1, 1, 0)),
    ("g8_ok K % 128", (4096, 4096, 768), (1, 1, 1, 0), (4096, 4096, 704), (2, 0, 1, 0)),
    ("g8_ok K % 128, backward above 2^25 scores", (4096, 16384, 768), (1, 1, 1, 0), (4096, 16384, 704), (2, 0, 1, 0)),
    ("nl128_ok min tiles", (256, 2048, 768), (2, 0, 1, 0), (256, 1920, 768), (0, 0, 1, 0)),
    ("nl128_ok N >= 1024", (1024, 1024, 768), (2, 0, 1, 0), (1024, 1016, 768), (0, 0, 1, 0)),
    ("nl128_ok K % 64 (K % 128 != 0)", (1024, 4096, 704), (2, 0, 1, 0), (1024, 4096, 736), (0, 0, 1, 0)),
    ("nl128_ok max tiles", (2048, 4096, 768), (2, 1, 1, 0), (2048, 4352, 768), (1, 1, 1, 0)),
    ("pair128_use Nc 2048 above 512 rows", (1024, 2048, 768), (2, 0, 1, 0), (1024, 2040, 768), (2, 0, 1, 0)),
    ("pair128_use B x Nc = 2^25", (2048, 16384, 768), (1, 1, 1, 0), (2048, 16448, 768), (1, 1, 1, 0)),
    ("pair128_use fill d 1024", (2048, 8192, 768), (1, 1, 1, 0), (2048, 8192, 1024), (1, 1, 1, 0)),
    ("big_bwd_ok B % 64", (1024, 4096, 768), (2, 0, 1, 0), (1000, 4096, 768), (2, 0, 1, 0)),
    ("big_bwd_ok Nc % 64", (1024, 4096, 768), (2, 0, 1, 0), (1024, 4104, 768), (2, 0, 1, 0)),
    ("long axis Nc >= 32 B", (1024, 32768, 768), (1, 1, 1, 0), (1024, 32704, 768), (1, 1, 1, 0)),
    ("long axis B < 512 Nc >= 56 Ki", (256, 57344, 768), (1, 1, 1, 0), (256, 57280, 768), (1, 1, 1, 0)),
    ("dc_alone_8p / p16_staged 128 KiB row pitch", (1024, 65536, 768), (1, 1, 1, 0), (1024, 65472, 768), (1, 1, 1, 0)),
]


@pytest.mark.parametrize("gate,inside,q_in,outside,q_out", PLAN_TABLE, ids=[r[0] for r in PLAN_TABLE])
def test_plan_table_host_queries(gate, inside, q_in, outside, q_out):
    from dpr_scale_amd import _lib

    def ask(s):
        return (_lib.fwd_one_pass(*s), int(_lib.fwd_no_logits(*s)), int(_lib.step_wants_g(*s)), _lib.train_dq_slabs(*s))

    assert ask(inside) == q_in, (gate, "inside", inside)
    assert ask(outside) == q_out, (gate, "outside", outside)
