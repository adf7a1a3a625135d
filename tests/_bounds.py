"""TEST-ONLY fp64 reference of the training step with a per-element error bound for every output (helper module, like
_oracle_kernels.py; not a conftest).  Works on torch tensors, so the reference runs in float64 on whatever device the inputs live on.

Every input is bf16-representable (q, c as bf16 values, possibly held in fp32).  A kernel output is scored element by element as
|kernel - reference| / bound; a score above 1 means the kernel is outside what fp32 arithmetic on these inputs can explain.

Error model (u = 2^-24, the unit roundoff of fp32 round-to-nearest-even; UA = 2^-23 per addition inside an accumulator, because the
MFMA adders are only specified as faithful -- within one ulp -- not as round-to-nearest):

  logits      the products of two bf16 values are exact in fp32 (8 + 8 significant bits), so S_ij = inv_T * sum_k q_ik c_jk carries only
              accumulation error: |dS_ij| <= (gamma(d) + u) * A_ij,  A = (|q| @ |c|^T) * inv_T,  gamma(n) = n UA / (1 - n UA)
              (the + u is the multiply by inv_T; the reference uses the same fp32 inv_T the kernel is given).
  exp         __expf(x) = v_exp_f32(x * log2 e): argument and constant rounding u|x| each, v_exp_f32 one ulp: 2u (1 + |x|) relative.
  lse         lse_i = m_i + log sum_j exp(S_ij - m_i): first order in the logit errors (weights P_ij), the exps of the terms (two per
              term on the strip-statistics plans: inside the strip and the strip's rescale, |x| adding up to at most lse_i - S_ij), the
              fp32 sum of Nc positive terms (gamma(Nc) relative -> absolute in the log), and the roundings of log and of the add.
  G           G_ij = (P_ij - [j == y_i]) * gs with P_ij = exp(S_ij - lse_i): relative error of P_ij is eps_ij = dS_ij + dlse_i +
              4u (1 + lse_i - S_ij) + 2u; the fp16-numerator plans add 2^-11 relative (RNE into an 11-bit significand; gemm8p.h:573-580
              says 2^-12, but half an ulp of an 11-bit significand is 2^-11 of the value at the bottom of a binade) and 2^-39 absolute
              (fp16 subnormals, 2^-25 of a numerator scaled by 2^14).  Then the subtraction and the scale: 2u |G|.
              The kernel's bf16 G must be the RNE rounding of the fp64 G; an element whose fp64 value lies within its bound of a rounding
              midpoint is AMBIGUOUS and may round either way.  Score: the distance the fp64 value would have to move to round to the
              kernel's value, over its bound (0 when they round alike).  Masked columns: exactly 0.  The gold column: (P - 1) * gs whether
              masked or not (P = 0 there when masked: gemm8p.h:1020).
  dQ, dC      against the kernel's own G in fp64 (where G is exposed): bf16 x bf16 products exact again, so
              |err| <= gamma_acc * (|G| @ |C|), gamma_acc = gamma(K + slabs) + 3u (K = contraction length, slabs = split-K partial sums
              added after it, 3u = the h_scale / d_scale / grad-output rescale multiplies).
              Where G is not exposed the plan's rounding point is emulated in fp64 (MODELS below) and each element that is ambiguous at
              that point adds (2^-7 (|G_ij| + band_ij) + band_ij) |C_jk|: the kernel rounds a value within the band of the fp64 one, so
              it lands within the band plus one bf16 ulp (at most 2^-7 of the value) of the emulated rounding -- one ulp where the band
              is narrower than the bf16 spacing, more where it is wider (the gold entry of a peaked row, P - 1 near 0).  Plus the
              relative error of whatever fp32 factor multiplies the rounded value.  (Emulating an ambiguous
              element unrounded with 2^-8 allowed measured no tighter: a flip then costs half an ulp against a 2^-8 allowance.)
"""
import math

import torch

U = 2.0 ** -24
UA = 2.0 ** -23
F16_REL, F16_ABS = 2.0 ** -11, 2.0 ** -39
BF16_ULP = 2.0 ** -7  # one bf16 ulp, relative to the value (at most)
TINY = 2.0 ** -126  # fp32 subnormals may flush to zero

# rounding models: where each plan rounds the softmax and what a hidden G is emulated by (source line restated)
MODELS = {
    # G (bf16) = RNE of the fp32 (softmax - onehot) * gs (dprhot.h: dprhot_softmax_ce_fwd_bwd; gemm8p.h Epi8G; step_small.h)
    "bf16_g": dict(f16=False, tile=0),
    # the one-pass forward: P = exp(S - strip max) * 2^14 as fp16, rescaled into bf16 G in place (gemm8p.h:573-580, g8_lse_p2g_kernel)
    "bf16_g_f16num": dict(f16=True, tile=0),
    # the few-rows step without its dScores launch: every 128-column tile's OWN softmax exp(S - tile_lse) as bf16, gold column stored
    # as 0 and its term (P_gold - 1) * gs added in fp32 (skinny.h:116); the backward multiplies tile t by exp(tile_lse - lse) in fp32
    "sk_tile_bf16": dict(f16=False, tile=128),
}


def gamma(n, ua=UA):
    n = float(n)
    assert n * ua < 0.5
    return n * ua / (1.0 - n * ua)


def _f64(x):
    return x.detach().to(torch.float64)


def _logsumexp(S):
    m = S.max(dim=1, keepdim=True).values
    mf = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    s = torch.exp(S - mf).sum(dim=1, keepdim=True)
    return (mf + torch.log(s)).squeeze(1), m.squeeze(1), s.squeeze(1)


def forward(q, c, y, colmask, inv_T, gs, y_offset=0, f16=False):
    """fp64 reference of the forward with its bounds.  q [B,d], c [Nc,d] (bf16 values), y [B] rank-local gold, colmask [Nc] (nonzero =
    masked) or None, inv_T the fp32 value the kernel gets, gs the G scale.  Returns a dict of fp64 tensors."""
    B, d = q.shape
    Nc = c.shape[0]
    inv_T = float(torch.tensor(inv_T, dtype=torch.float32))
    q64, c64 = _f64(q), _f64(c)
    S = (q64 @ c64.T) * inv_T
    A = (q64.abs() @ c64.abs().T) * abs(inv_T)
    eS = (gamma(d) + U) * A
    mk = colmask.to(torch.bool) if colmask is not None else torch.zeros(Nc, dtype=torch.bool, device=q.device)
    return dict(from_scores(S, y, gs, y_offset, mk, eS, f16=f16), A=A, inv_T=inv_T)


def _e_lse_strips(P, gap, eS, lse, m, s):
    """The lse bound of the strip-statistics plans of the training step (module docstring, "lse")."""
    return (P * (eS + 4 * U * (1 + gap))).sum(1) + gamma(P.shape[1]) + 2 * U * (lse.abs().nan_to_num(0.0, 0.0, 0.0) + m.abs().nan_to_num(0.0, 0.0, 0.0) + 1)


def from_scores(S, y, gs, y_offset=0, mask=None, eS=None, f16=False, e_lse=_e_lse_strips, exp_u=4, g_tiny=0.0):
    """The reference from the logits on: S [B, Nc] fp64 with the bound eS of its elements (None: the logits are given, eS = 0), mask
    [Nc] or -- one window per row -- [B, Nc] (True = the column counts as -inf), y [B] rank-local gold.  `e_lse(P, gap, eS, lse, m, s)`
    is the plan's bound of the row logsumexp (m, s: the row maximum and the sum of exp(S - m)); the exp of the G pass costs
    exp_u * u (1 + gap) relative; g_tiny: absolute allowance of a G product that is itself flushed.  The same keys as `forward`."""
    B, Nc = S.shape
    dev = S.device
    mk = torch.zeros(Nc, dtype=torch.bool, device=dev) if mask is None else mask.to(torch.bool)
    eS = torch.zeros_like(S) if eS is None else eS
    S = torch.where(mk.expand_as(S), torch.full_like(S, -math.inf), S)
    eS = torch.where(mk.expand_as(S), torch.zeros_like(eS), eS)
    yg = (y.to(torch.int64) + int(y_offset)).to(dev)
    rows = torch.arange(B, device=dev)
    lse, m, s = _logsumexp(S)
    fin = torch.isfinite(lse)
    P = torch.where(torch.isfinite(S) & fin[:, None], torch.exp(S - torch.where(fin, lse, 0.0)[:, None]), torch.zeros_like(S))
    gap = torch.where(torch.isfinite(S) & fin[:, None], lse[:, None] - S, torch.zeros_like(S))  # lse - S >= 0
    e_lse = e_lse(P, gap, eS, lse, m, s)
    gold = S[rows, yg]
    loss = lse - gold
    e_loss = e_lse + eS[rows, yg] + U * loss.abs().nan_to_num(0.0, 0.0, 0.0)
    eps = eS + e_lse[:, None] + exp_u * U * (1 + gap) + 2 * U
    if f16:
        eps = eps + F16_REL
    G = P * gs
    G[rows, yg] -= gs
    dG = abs(gs) * (P * eps + (F16_ABS if f16 else 0.0) + TINY) + 2 * U * G.abs()
    if g_tiny:
        dG = dG + g_tiny
    return dict(S=S, eS=eS, lse=lse, e_lse=e_lse, loss=loss, e_loss=e_loss, P=P, G=G, dG=dG, eps=eps, mask=mk, yg=yg, gs=gs)


def _ratio(err, bound):
    return torch.where(err == 0, torch.zeros_like(err), err / torch.clamp(bound, min=1e-300))


def finite_match(k, r):
    """isfinite patterns equal, and the non-finite values equal (same infinity, or NaN where the reference is NaN)."""
    k, r = _f64(k), _f64(r)
    fk, fr = torch.isfinite(k), torch.isfinite(r)
    if not torch.equal(fk, fr):
        return False
    nk, nr = k[~fk], r[~fr]
    return bool(torch.equal(torch.isnan(nk), torch.isnan(nr)) and torch.equal(nk[~torch.isnan(nk)], nr[~torch.isnan(nr)]))


def score_rows(kernel, ref, bound):
    """Worst |kernel - ref| / bound over the finite entries; inf when the isfinite patterns differ."""
    if not finite_match(kernel, ref):
        return math.inf
    k, r = _f64(kernel), _f64(ref)
    f = torch.isfinite(r)
    if not f.any():
        return 0.0
    return float(_ratio((k[f] - r[f]).abs(), bound[f]).max())


def loss_sum_bound(ref, scale=1.0):
    l = ref["loss"]
    f = torch.isfinite(l)
    return abs(scale) * (float(ref["e_loss"][f].sum()) + gamma(l.numel()) * float(l[f].abs().sum())) + U * abs(scale * float(l[f].sum()))


def score_loss_sum(value, ref, scale=1.0):
    r = scale * float(ref["loss"].sum())
    v = float(value)
    if not math.isfinite(r) or not math.isfinite(v):
        return 0.0 if (v == r or (math.isnan(v) and math.isnan(r))) else math.inf
    return abs(v - r) / max(loss_sum_bound(ref, scale), 1e-300)


def _bf16_interval(v):
    """[lo, hi]: the reals that round (RNE, ignoring ties) to each bf16 value v (fp64 tensor of bf16 values)."""
    vb = v.to(torch.bfloat16)
    up = torch.nextafter(vb, torch.full_like(vb, math.inf)).to(torch.float64)
    dn = torch.nextafter(vb, torch.full_like(vb, -math.inf)).to(torch.float64)
    return (v + dn) / 2, (v + up) / 2


def g_scores(Gk, ref):
    """Per-element G scores (fp64 tensor) and the ambiguity mask.  Masked non-gold columns must be exactly 0 (inf otherwise)."""
    Gr, dG = ref["G"], ref["dG"]
    gk = _f64(Gk)
    lo, hi = _bf16_interval(gk)
    dist = torch.clamp(torch.maximum(lo - Gr, Gr - hi), min=0.0)
    sc = _ratio(dist, dG)
    masked = ref["mask"].expand_as(Gr).clone()  # [Nc], or [B, Nc] where every row has a window of its own
    masked[torch.arange(Gr.shape[0], device=Gr.device), ref["yg"]] = False
    sc = torch.where(masked, torch.where(gk == 0, 0.0, math.inf), sc)
    sc = torch.where(torch.isfinite(gk), sc, torch.full_like(sc, math.inf))
    amb = ambiguous(Gr, dG) & ~masked
    return sc, amb


def ambiguous(x, band):
    """Elements whose fp64 value lies within `band` of a bf16 rounding midpoint."""
    r = x.to(torch.bfloat16).to(torch.float64)
    lo, hi = _bf16_interval(r)
    return torch.minimum((x - lo).abs(), (hi - x).abs()) <= band


def score_grad(kernel, ref, bound):
    k = _f64(kernel)
    if not torch.isfinite(k).all():
        return math.inf
    return float(_ratio((k - ref).abs(), bound).max())


def bwd_from_g(G, q, c, h=1.0, slabs_q=1, slabs_c=1):
    """dQ = h G @ C and dC = h G^T @ Q in fp64 from the kernel's G, with their bounds."""
    g, q64, c64 = _f64(G), _f64(q), _f64(c)
    B, Nc = g.shape
    ga = g.abs()
    dQ = h * (g @ c64)
    dC = h * (g.T @ q64)
    bQ = (gamma(Nc + slabs_q) + 3 * U) * abs(h) * (ga @ c64.abs()) + TINY
    bC = (gamma(B + slabs_c) + 3 * U) * abs(h) * (ga.T @ q64.abs()) + TINY
    return dQ, bQ, dC, bC


def hidden_g(ref, model):
    """The fp64 emulation of a plan whose G never leaves the kernel: the G the plan's backward effectively multiplies by, and per
    element the relative error allowance on top of the accumulation (ambiguous roundings, fp32 factors).  Returns (G, extra, n_amb)."""
    P, S, eS, gs, mk, yg = ref["P"], ref["S"], ref["eS"], ref["gs"], ref["mask"], ref["yg"]
    B, Nc = P.shape
    rows = torch.arange(B, device=P.device)
    gold = torch.zeros_like(P, dtype=torch.bool)
    gold[rows, yg] = True
    if MODELS[model]["tile"] == 0:
        G, dG = ref["G"], ref["dG"]
        Gb = G.to(torch.bfloat16).to(torch.float64)
        amb = ambiguous(G, dG) & ~mk[None, :]
        extra = amb * (BF16_ULP * (Gb.abs() + dG) + dG)
        return Gb, extra, int(amb.sum())
    W = MODELS[model]["tile"]
    nt = -(-Nc // W)
    pad = nt * W - Nc
    Sp = torch.nn.functional.pad(S, (0, pad), value=-math.inf).view(B, nt, W)
    ePp = torch.nn.functional.pad(eS, (0, pad)).view(B, nt, W)
    tl, tm, _ = _logsumexp(Sp.reshape(B * nt, W))
    tl, tm = tl.view(B, nt), tm.view(B, nt)
    tfin = torch.isfinite(tl)
    Pt = torch.where(torch.isfinite(Sp) & tfin[..., None], torch.exp(Sp - torch.where(tfin, tl, 0.0)[..., None]), torch.zeros_like(Sp))
    gap = torch.where(torch.isfinite(Sp) & tfin[..., None], tl[..., None] - Sp, torch.zeros_like(Sp))
    e_tl = (Pt * (ePp + 4 * U * (1 + gap))).sum(2) + gamma(W) + 2 * U * (tl.abs().nan_to_num(0.0, 0.0, 0.0) + tm.abs().nan_to_num(0.0, 0.0, 0.0) + 1)
    eps_t = ePp + e_tl[..., None] + 2 * U * (1 + gap) + 2 * U  # exp(S - m) and the multiply by 1 / sum
    Ptb = Pt.to(torch.bfloat16).to(torch.float64)
    band = eps_t * Pt + TINY
    ambt = ambiguous(Pt, band)
    arel = torch.where(ambt, BF16_ULP * (1 + band / torch.clamp(Ptb, min=1e-300)) + band / torch.clamp(Ptb, min=1e-300), torch.zeros_like(Pt))
    arel = arel.reshape(B, nt * W)[:, :Nc]
    amb = ambt.reshape(B, nt * W)[:, :Nc]
    lse = ref["lse"]
    fin = torch.isfinite(lse)
    fac = torch.where(tfin & fin[:, None], torch.exp(tl - torch.where(fin, lse, 0.0)[:, None]), torch.zeros_like(tl))
    e_fac = ref["e_lse"][:, None] + e_tl + 2 * U * (1 + (lse[:, None] - tl).abs().nan_to_num(0.0, 0.0, 0.0)) + 3 * U
    G = gs * (Ptb * fac[..., None]).reshape(B, nt * W)[:, :Nc]
    efac = e_fac[..., None].expand(B, nt, W).reshape(B, nt * W)[:, :Nc]
    extra = G.abs() * (arel + efac)
    amb = amb & ~gold & ~mk[None, :]
    # the gold column: 0 in the tile softmax, (P_gold - 1) * gs added in fp32
    Pg = P[rows, yg]
    G[rows, yg] = gs * (Pg - 1.0)
    extra[rows, yg] = abs(gs) * Pg * ref["eps"][rows, yg] + 2 * U * G[rows, yg].abs()
    G = torch.where(mk[None, :] & ~gold, torch.zeros_like(G), G)
    extra = torch.where(mk[None, :] & ~gold, torch.zeros_like(extra), extra)
    return G, extra, int(amb.sum())


def bwd_hidden(ref, model, q, c, h=1.0, slabs_q=1, slabs_c=1):
    """dQ / dC of a plan that keeps G to itself, with bounds: accumulation on the emulated G plus the per-element allowance."""
    G, extra, n_amb = hidden_g(ref, model)
    dQ, bQ, dC, bC = bwd_from_g(G, q, c, h, slabs_q, slabs_c)
    q64, c64 = _f64(q).abs(), _f64(c).abs()
    bQ = bQ + abs(h) * (extra @ c64)
    bC = bC + abs(h) * (extra.T @ q64)
    return dQ, bQ, dC, bC, n_amb


def check_step(ref, *, row_loss=None, row_lse=None, loss_sum=None, loss_scale=1.0, G=None, dQ=None, dC=None, q=None, c=None, h=1.0,
               model="bf16_g", slabs_q=16, slabs_c=1):
    """Every score of one step's outputs against the reference.  G given: the backward is checked against the kernel's own G;
    G None: against the plan's rounding model.  Returns (dict of worst scores, number of ambiguous G elements)."""
    sc = {}
    if row_lse is not None:
        sc["lse"] = score_rows(row_lse, ref["lse"], ref["e_lse"])
    if row_loss is not None:
        sc["loss"] = score_rows(row_loss, ref["loss"], ref["e_loss"])
    if loss_sum is not None:
        sc["loss_sum"] = score_loss_sum(loss_sum, ref, loss_scale)
    n_amb = 0
    if G is not None:
        g, amb = g_scores(G, ref)
        sc["G"] = float(g.max())
        n_amb = int(amb.sum())
        if dQ is not None or dC is not None:
            rQ, bQ, rC, bC = bwd_from_g(G, q, c, h, slabs_q, slabs_c)
    elif dQ is not None or dC is not None:
        rQ, bQ, rC, bC, n_amb = bwd_hidden(ref, model, q, c, h, slabs_q, slabs_c)
    if dQ is not None:
        sc["dQ"] = score_grad(dQ, rQ, bQ)
    if dC is not None:
        sc["dC"] = score_grad(dC, rC, bC)
    return sc, n_amb
