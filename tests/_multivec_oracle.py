"""TEST-ONLY checker of the late-interaction expert score: a float64 torch restatement of the reference's
dpr_scale/task/citadel_task.py:155-238 (gradients by autograd), and a seeded input generator for ColBERT, COIL and CITADEL.

Inputs live on a coarse grid so that every token score, every weight product and every pooled sum is exact in fp32 whatever the
summation order: features are multiples of 1/4 in [-1, 1], weights multiples of 1/8 in (0, 1].  So the HIP path must reproduce the
maxima and their argmax EXACTLY, exact ties included (padding zeros, unmatched slots, repeated tokens), and only gradients carry
fp32 rounding.  `grid=False` draws gaussian features instead (scores then agree to accumulation error only)."""
import numpy as np
import torch

KINDS = ("colbert", "coil", "citadel")


def make_inputs(seed, kind, B, LQ, Nc, LD, d, KQ=1, KD=1, n_experts=6, masked=(), pad_frac=0.3, grid=True, all_pad=()):
    """Returns (query_repr, context_repr, mask) as the reference's encoders would: padded tokens are zero vectors (and, for COIL, carry
    weight 0); `masked` lists context indices set in the [Nc] bool mask; `all_pad` lists contexts made of padding only."""
    g = np.random.default_rng(seed)

    def feats(n, L):
        if grid:
            x = g.integers(-4, 5, size=(n, L, d)).astype(np.float32) / 4.0
        else:
            x = g.standard_normal((n, L, d)).astype(np.float32)
            x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
        lens = np.maximum(1, np.round(L * (1 - pad_frac * g.random(n))).astype(int))
        att = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
        if n > 1 and L > 2:  # exact duplicate tokens: ties between real tokens
            x[0, 1] = x[0, 0]
        return x * att[..., None], att

    q, qatt = feats(B, LQ)
    c, catt = feats(Nc, LD)
    for a in all_pad:
        c[a] = 0.0
        catt[a] = 0
    qr = {"expert_repr": torch.from_numpy(q)}
    cr = {"expert_repr": torch.from_numpy(c)}
    if kind == "coil":
        qr["expert_ids"] = torch.from_numpy(g.integers(0, n_experts, size=(B, LQ)))
        cr["expert_ids"] = torch.from_numpy(g.integers(0, n_experts, size=(Nc, LD)))
        qr["expert_weights"] = torch.from_numpy(qatt)
        cr["expert_weights"] = torch.from_numpy(catt)
    elif kind == "citadel":
        def topk_ids(n, L, K):
            return np.stack([np.stack([g.permutation(n_experts)[:K] for _ in range(L)]) for _ in range(n)])

        qr["expert_ids"] = torch.from_numpy(topk_ids(B, LQ, KQ))
        cr["expert_ids"] = torch.from_numpy(topk_ids(Nc, LD, KD))
        qr["expert_weights"] = torch.from_numpy((g.integers(1, 9, size=(B, LQ, KQ)) / 8.0 * qatt[..., None]).astype(np.float32))
        cr["expert_weights"] = torch.from_numpy((g.integers(1, 9, size=(Nc, LD, KD)) / 8.0 * catt[..., None]).astype(np.float32))
    mask = torch.zeros(Nc, dtype=torch.bool)
    for m in masked:
        mask[m] = True
    return qr, cr, mask


def _tok_scores(q, c, pairwise):
    """citadel_task.py:155-166 (colbert_score): [B, LQ, Y, LD]."""
    if pairwise:
        M = c.shape[0] // q.shape[0]
        return torch.einsum("bid,bmjd->bimj", q, c.view(q.shape[0], M, c.shape[1], c.shape[2]))
    return torch.einsum("bid,cjd->bicj", q, c)


def expert_sim_score(qr, cr, mask=None, pairwise=False, query_pool="sum", return_argmax=False):
    """citadel_task.py:215-238 in float64 on whatever tensors are passed (leaf tensors may require grad)."""
    q, c = qr["expert_repr"].double(), cr["expert_repr"].double()
    B, Nc = q.shape[0], c.shape[0]
    M = Nc // B
    s = _tok_scores(q, c, pairwise)  # [B, LQ, Y, LD]
    if "expert_ids" in qr:
        qi, ci = qr["expert_ids"], cr["expert_ids"]
        if qi.dim() == 2:  # COIL (:168-189): one slot per token
            qi, ci = qi.unsqueeze(-1), ci.unsqueeze(-1)
        KQ, KD = qi.shape[-1], ci.shape[-1]
        if pairwise:  # (:193-198)
            ci = ci.view(B, M, ci.shape[1], KD)
            match = qi[:, :, :, None, None, None] == ci[:, None, None, :, :, :]
        else:  # (:199-200)
            match = qi[:, :, :, None, None, None] == ci[None, None, None, :, :, :]
        if "expert_weights" in qr:  # (:202-209): COIL weights are the integer mask, CITADEL's the router weights
            qw, cw = qr["expert_weights"].double(), cr["expert_weights"].double()
            if qw.dim() == 2:
                qw, cw = qw.unsqueeze(-1), cw.unsqueeze(-1)
            if pairwise:
                cw = cw.view(B, M, cw.shape[1], KD)
                w = qw[:, :, :, None, None, None] * cw[:, None, None, :, :, :]
            else:
                w = qw[:, :, :, None, None, None] * cw[None, None, None, :, :, :]
            coef = torch.where(match, w, torch.zeros((), dtype=w.dtype))
        else:
            coef = match.double()
        v = s[:, :, None, :, :, None] * coef  # [B, LQ, KQ, Y, LD, KD]
        v = v.reshape(B, v.shape[1] * KQ, v.shape[3], v.shape[4] * KD)  # (:211): slot order j * KD + kd
    else:
        v = s
    mx = v.max(-1)  # first maximal index on ties
    if query_pool == "sum":
        scores, parg = mx.values.sum(1), None
    elif query_pool == "max":
        pm = mx.values.max(1)
        scores, parg = pm.values, pm.indices
    else:
        raise NotImplementedError
    if mask is not None:  # (:230-238): index-put, no gradient through masked entries
        mm = mask.view(-1, M) if pairwise else mask.reshape(1, -1).expand(B, -1)
        scores = scores.masked_fill(mm, float("-inf"))
    if return_argmax:
        return scores, mx.indices, parg  # argmax [B, LQ*KQ, Y]
    return scores


def leaf(repr_, grad_weights=True):
    """float64 copies requiring grad (expert_repr, and CITADEL's float expert_weights when grad_weights)."""
    out = {}
    for k, t in repr_.items():
        t = t.detach().clone()
        if k == "expert_repr" or (k == "expert_weights" and grad_weights and t.is_floating_point()):
            t = t.double().requires_grad_(True)
        out[k] = t
    return out


def scores_and_grads(qr, cr, mask, pairwise, pool, dS, grad_weights=True):
    """(S, dict of grads) of the oracle with upstream gradient dS (masked entries ignored)."""
    lq, lc = leaf(qr, grad_weights), leaf(cr, grad_weights)
    S = expert_sim_score(lq, lc, mask, pairwise, pool)
    fin = torch.isfinite(S)
    (S.masked_fill(~fin, 0.0) * dS.double().masked_fill(~fin, 0.0)).sum().backward()
    grads = {"dq": lq["expert_repr"].grad, "dc": lc["expert_repr"].grad}
    if "expert_weights" in lq and lq["expert_weights"].requires_grad:
        grads["dwq"], grads["dwc"] = lq["expert_weights"].grad, lc["expert_weights"].grad
    return S.detach(), grads


# ---- exact gradients on grid inputs ---------------------------------------------------------------------------------------------------
# With the upstream gradient on a grid too, every term of every gradient is a multiple of a power of two (2^-11 for dq / dc with
# CITADEL weights: dS 1/8 x w_q 1/8 x w_c 1/8 x feature 1/4; 2^-10 for dwq / dwc: dS 1/8 x raw dot product 1/16 x weight 1/8), and as
# long as the sum of the terms' magnitudes stays below 2^24 of those units every fp32 partial sum is exact in ANY order.
# `exact_certificate` proves that for a given case, and a kernel must then match the fp64 gradients bit for bit.
GRADS = ("dq", "dc", "dwq", "dwc")


def grid_dS(seed, shape):
    """Upstream gradient on a grid: multiples of 1/8 in [-2, 2], fp32."""
    g = np.random.default_rng(seed)
    return torch.from_numpy((g.integers(-16, 17, size=tuple(shape)) / 8.0).astype(np.float32))


def gather_terms(qr, cr, mask, pairwise, pool, dS):
    """One entry per (query b, row slot rs = i * KQ + kq, column y) -- what flows back through that slot's argmax -- as float64 / int64
    numpy arrays of shape [B, LQ*KQ, Y]: the query token i, slot kq, context ctx, its selected token j and slot kd, the upstream
    gradient gr (0 at masked columns and, under max pooling, everywhere but at the pooled row slot), match (0 / 1), the two weights
    (1 without weights) and the raw dot product <q[b, i], c[ctx, j]>."""
    q, c = qr["expert_repr"].double().numpy(), cr["expert_repr"].double().numpy()
    B, LQ, _ = q.shape
    Nc, LD, _ = c.shape
    M = Nc // B
    _, arg, parg = expert_sim_score(qr, cr, mask, pairwise, pool, return_argmax=True)
    arg = arg.numpy()  # [B, LQ*KQ, Y]
    RS, Y = arg.shape[1], arg.shape[2]
    KQ = RS // LQ
    KD = 1
    if "expert_ids" in qr and cr["expert_ids"].dim() == 3:
        KD = cr["expert_ids"].shape[2]
    b = np.broadcast_to(np.arange(B)[:, None, None], arg.shape)
    rs = np.broadcast_to(np.arange(RS)[None, :, None], arg.shape)
    y = np.broadcast_to(np.arange(Y)[None, None, :], arg.shape)
    i, kq = rs // KQ, rs % KQ
    ctx = b * M + y if pairwise else y
    j, kd = arg // KD, arg % KD
    gr = np.broadcast_to(dS.double().numpy()[:, None, :], arg.shape).copy()
    if mask is not None:
        gr[mask.numpy()[ctx]] = 0.0
    if pool == "max":
        gr[parg.numpy()[:, None, :] != rs] = 0.0
    match = np.ones(arg.shape)
    wq = np.ones(arg.shape)
    wc = np.ones(arg.shape)
    if "expert_ids" in qr:
        qi, ci = qr["expert_ids"].numpy().reshape(B, LQ, KQ), cr["expert_ids"].numpy().reshape(Nc, LD, KD)
        match = (qi[b, i, kq] == ci[ctx, j, kd]).astype(np.float64)
        if "expert_weights" in qr:
            wq = qr["expert_weights"].double().numpy().reshape(B, LQ, KQ)[b, i, kq]
            wc = cr["expert_weights"].double().numpy().reshape(Nc, LD, KD)[ctx, j, kd]
    raw = (q[b, i] * c[ctx, j]).sum(-1)
    return dict(b=b, i=i, kq=kq, ctx=ctx, j=j, kd=kd, gr=gr, match=match, wq=wq, wc=wc, raw=raw)


def _granularity(x):
    """The coarsest power of two that every entry of x is a multiple of (1.0 when x is all zero)."""
    x = np.abs(np.asarray(x, dtype=np.float64).ravel())
    x = x[x != 0]
    if x.size == 0:
        return 1.0
    man, ex = np.frexp(x)  # x = man * 2^ex, man in [0.5, 1) with at most 53 significant bits
    m = (man * 2.0**53).astype(np.int64)
    low = m & -m  # lowest set bit
    return float(2.0 ** (np.log2(low.astype(np.float64)) + ex - 53).min())


def accumulate_terms(qr, cr, t, weights=None):
    """Adds the terms of `gather_terms` up in float64 (np.add.at).  Returns (grads, abs_sums, gran): per gradient the tensor, the
    per-element sum of the terms' magnitudes, and the power of two that every term is a multiple of.  dwq / dwc only when the
    representation carries float weights (or `weights` says so)."""
    q, c = qr["expert_repr"].double().numpy(), cr["expert_repr"].double().numpy()
    if weights is None:
        weights = "expert_weights" in qr and qr["expert_weights"].is_floating_point()
    KQ, KD = int(t["kq"].max()) + 1, 1
    if "expert_ids" in cr and cr["expert_ids"].dim() == 3:
        KD = cr["expert_ids"].shape[2]
    cf = t["gr"] * (t["match"] * (t["wq"] * t["wc"]))
    live = cf != 0
    b, i, kq, ctx, j, kd = (t[k][live] for k in ("b", "i", "kq", "ctx", "j", "kd"))
    terms = {"dq": ((b, i), cf[live][:, None] * c[ctx, j], q.shape), "dc": ((ctx, j), cf[live][:, None] * q[b, i], c.shape)}
    if weights:
        gm = t["gr"] * t["raw"] * t["match"]
        terms["dwq"] = ((b, i, kq), (gm * t["wc"])[live], q.shape[:2] + (KQ,))
        terms["dwc"] = ((ctx, j, kd), (gm * t["wq"])[live], c.shape[:2] + (KD,))
    grads, abs_sums, gran = {}, {}, {}
    for k, (idx, val, shape) in terms.items():
        out, mag = np.zeros(shape), np.zeros(shape)
        np.add.at(out, idx, val)
        np.add.at(mag, idx, np.abs(val))
        grads[k], abs_sums[k], gran[k] = torch.from_numpy(out), torch.from_numpy(mag), _granularity(val)
    return grads, abs_sums, gran


def explicit_grads(qr, cr, mask, pairwise, pool, dS):
    """The four gradients without autograd: from the argmax tables, by gathering the selected rows.  (grads, abs_sums, gran)."""
    grads, abs_sums, gran = accumulate_terms(qr, cr, gather_terms(qr, cr, mask, pairwise, pool, dS))
    qw = qr.get("expert_weights")
    if qw is not None and qw.is_floating_point():  # the weights' own shapes ([B, L] or [B, L, K])
        for k, r in (("dwq", qr), ("dwc", cr)):
            grads[k], abs_sums[k] = grads[k].reshape(r["expert_weights"].shape), abs_sums[k].reshape(r["expert_weights"].shape)
    return grads, abs_sums, gran


def _fits_fp32(name, x):
    x = np.asarray(x, dtype=np.float64)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x), f"{name}: a product does not fit fp32's 24 bits"


def exact_certificate(qr, cr, mask, pairwise, pool, dS):
    """Raises unless every fp32 product and every fp32 partial sum of the scores and of the four gradients is exact whatever the
    order of summation: each single product fits 24 bits, and per output the sum of the terms' magnitudes is below 2^24 units of
    the terms' common granularity.  A case that fails is a defect of the test's inputs.  Returns the per-gradient head room."""
    t = gather_terms(qr, cr, mask, pairwise, pool, dS)
    q, c = qr["expert_repr"].double().numpy(), cr["expert_repr"].double().numpy()
    f = t["match"] * (t["wq"] * t["wc"])
    val = t["raw"] * f  # the row slots' maxima
    cf = t["gr"] * f
    for name, x in (("raw", t["raw"]), ("wq*wc", t["wq"] * t["wc"]), ("raw*w", val), ("dS*w", cf), ("dS*raw", t["gr"] * t["raw"]),
                    ("dS*raw*wc", t["gr"] * t["raw"] * t["wc"]), ("dS*raw*wq", t["gr"] * t["raw"] * t["wq"]),
                    ("dS*w*c", cf[..., None] * c[t["ctx"], t["j"]]), ("dS*w*q", cf[..., None] * q[t["b"], t["i"]])):
        _fits_fp32(name, x)
    # the token dot products: d terms of granularity(q) * granularity(c)
    unit = _granularity(q) * _granularity(c)
    worst = np.abs(q).sum(-1).max() * np.abs(c).max()
    assert worst / unit < 2.0**24, f"token scores: {worst / unit:.3g} units"
    room = {}
    if pool == "sum":  # the pooled sum over a query's row slots
        room["S"] = np.abs(val).sum(1).max() / _granularity(val)
        assert room["S"] < 2.0**24, f"pooled scores: {room['S']:.3g} units"
    _, abs_sums, gran = accumulate_terms(qr, cr, t)
    for k, mag in abs_sums.items():
        room[k] = float(mag.max()) / gran[k]
        assert room[k] < 2.0**24, f"{k}: sum of |terms| is {room[k]:.3g} units of {gran[k]:.3g}"
    return room


def assert_exact(name, got, ref):
    """`got` (fp32) against the float64 reference cast to fp32, by torch.equal: every element, the non-finite pattern included.
    The reference must itself be an fp32 number everywhere (else the case is no exact case)."""
    ref32 = ref.to(torch.float32)
    assert got.dtype == torch.float32 and got.shape == ref32.shape, (name, got.dtype, tuple(got.shape), tuple(ref32.shape))
    assert torch.equal(ref32.double(), ref.double()), f"{name}: the reference is not representable in fp32"
    if not torch.equal(got, ref32):
        bad = (got != ref32).nonzero()
        at = tuple(bad[0].tolist())
        raise AssertionError(f"{name}: {bad.shape[0]} of {got.numel()} elements differ, first at {at}: got {got[at].item()!r}, "
                             f"expected {ref32[at].item()!r}; differing indices span {bad.min(0).values.tolist()} .. "
                             f"{bad.max(0).values.tolist()}")


# ---- the cases of the exact GPU tests (tests/test_multivec_exact_gpu.py; certified on the CPU in tests/test_multivec_exact.py) -------
def _case(kind, B, LQ, Nc, LD, d, KQ, KD, pairwise, pool, **kw):
    return dict(kind=kind, B=B, LQ=LQ, Nc=Nc, LD=LD, d=d, KQ=KQ, KD=KD, pairwise=pairwise, pool=pool, **kw)


# Tile edges: LQ / LD around MS_BM = MS_BN = 64; d = 40 (zero-padded to 64), 288 (a second 256-feature dq chunk, five 64-feature dc
# slices), 768; Ny (the dq kernel's 64-wide y loop in groups of 8) in {1, 8, 9, 63, 64, 65, 130}; row slots per dc sweep (in-batch
# Nq*LQ*KQ, pairwise LQ*KQ) around multiples of 64.  The first five are the shapes the premise was first checked on.
SWEEP = [
    _case("colbert", 3, 65, 65, 63, 40, 1, 1, False, "sum"),    # Ny 65, 195 row slots
    _case("citadel", 2, 63, 66, 65, 288, 2, 3, False, "sum"),   # Ny 66, 252 row slots
    _case("citadel", 3, 64, 9, 129, 256, 8, 2, True, "max"),    # Ny 3, 512 row slots per query
    _case("coil", 4, 17, 12, 64, 96, 1, 1, True, "sum"),        # Ny 3
    _case("citadel", 2, 9, 130, 21, 768, 3, 8, False, "max"),   # Ny 130, 54 row slots
    _case("colbert", 1, 63, 8, 1, 32, 1, 1, False, "max"),      # Ny 8, 63 row slots, LD 1
    _case("citadel", 1, 64, 9, 63, 40, 1, 1, False, "sum"),     # Ny 9, 64 row slots
    _case("coil", 5, 13, 63, 64, 32, 1, 1, False, "sum"),       # Ny 63, 65 row slots
    _case("citadel", 1, 1, 64, 65, 256, 2, 2, False, "max"),    # Ny 64, LQ 1
    _case("citadel", 3, 1, 3, 129, 32, 4, 1, True, "sum"),      # Ny 1 (M = 1), LQ 1
    _case("colbert", 2, 64, 128, 63, 40, 1, 1, True, "max"),    # Ny 64, 64 row slots per query
    _case("citadel", 2, 65, 16, 1, 768, 1, 3, True, "sum"),     # Ny 8, 65 row slots per query, LD 1
    _case("colbert", 1, 127, 10, 129, 40, 1, 1, False, "max"),  # 127 row slots
    _case("citadel", 1, 64, 65, 64, 288, 2, 2, False, "sum"),   # 128 row slots
    _case("coil", 3, 43, 9, 65, 256, 1, 1, False, "max"),       # 129 row slots
    _case("citadel", 2, 63, 18, 64, 32, 5, 2, True, "sum"),     # Ny 9, 315 row slots per query
    _case("colbert", 1, 65, 130, 63, 40, 1, 1, True, "max"),    # Ny 130 pairwise
    _case("colbert", 2, 1, 126, 65, 256, 1, 1, True, "sum"),    # Ny 63 pairwise
]
SLOT_COUNTS = [(1, 1), (2, 3), (3, 8), (4, 1), (5, 2), (7, 7), (8, 8)]  # every KQT text; the run-time break at KQ = 3, 5, 7
SLOTS = [_case("citadel", 2, 6, 6, 10, 64, kq, kd, False, "sum") for kq, kd in SLOT_COUNTS]
MODES = [(False, "sum"), (False, "max"), (True, "sum"), (True, "max")]
IDS_ONLY = [_case("citadel", 3, 20, 12, 33, 96, 2, 3, pw, pool, variant="ids_only") for pw, pool in MODES]
WEIGHTS_ONLY = [_case("citadel", 3, 20, 12, 33, 96, 1, 1, pw, pool, variant="weights_only") for pw, pool in MODES]
SUBSETS = _case("citadel", 3, 20, 12, 33, 96, 2, 3, False, "sum")
TIES = [_case(kind, 3, 20, 12, 33, 96, kq, kd, pw, "max", variant="pool_ties")
        for kind, kq, kd in (("colbert", 1, 1), ("citadel", 2, 3)) for pw in (False, True)]
EXACT_CASES = SWEEP + SLOTS + IDS_ONLY + WEIGHTS_ONLY + [SUBSETS] + TIES


def case_id(c):
    s = "{kind}-B{B}-LQ{LQ}-Nc{Nc}-LD{LD}-d{d}-K{KQ}x{KD}-".format(**c) + ("pairwise" if c["pairwise"] else "inbatch") + "-" + c["pool"]
    return s + ("-" + c["variant"] if c.get("variant") else "")


def tie_token(qr, cr, mask, pairwise):
    """The token of query 0 (not its last) that max pooling selects most often: the one the pool_ties variant repeats at the next position."""
    _, _, parg = expert_sim_score(qr, cr, mask, pairwise, "max", return_argmax=True)
    LQ = qr["expert_repr"].shape[1]
    KQ = qr["expert_ids"].shape[2] if "expert_ids" in qr and qr["expert_ids"].dim() == 3 else 1
    return int(torch.bincount(parg[0] // KQ, minlength=LQ)[:LQ - 1].argmax())


def build_case(c, pairwise=None, pool=None):
    """(qr, cr, mask, pairwise, pool, dS) of a case: grid inputs, one masked and one all-padding context, grid dS.  Variants:
    ids_only drops the expert weights; weights_only gives every slot the same expert id (what scoring without ids computes);
    pool_ties copies query 0's most often pooled token (features, ids, weights) to a later position, an exact tie of row slots."""
    pairwise = c["pairwise"] if pairwise is None else pairwise
    pool = c["pool"] if pool is None else pool
    B, Nc = c["B"], c["Nc"]
    seed = 1000 + sum(c[k] * m for k, m in zip(("B", "LQ", "Nc", "LD", "d", "KQ", "KD"), (1, 3, 5, 7, 11, 13, 17)))
    qr, cr, mask = make_inputs(seed, c["kind"], B=B, LQ=c["LQ"], Nc=Nc, LD=c["LD"], d=c["d"], KQ=c["KQ"], KD=c["KD"], n_experts=12,
                               masked=(1,) if Nc > 2 else (), all_pad=(Nc - 1,) if Nc > 1 else ())
    for r in (qr, cr):  # (make_inputs leaves float64 features; the values are fp32 numbers, and fp32 in gives fp32 gradients out)
        r["expert_repr"] = r["expert_repr"].float()
    variant = c.get("variant")
    if variant == "ids_only":
        del qr["expert_weights"], cr["expert_weights"]
    elif variant == "weights_only":
        qr["expert_ids"].zero_()
        cr["expert_ids"].zero_()
    elif variant == "pool_ties":
        tok = tie_token(qr, cr, mask, pairwise)
        for k in qr:
            qr[k][0, tok + 1] = qr[k][0, tok]
    Y = Nc // B if pairwise else Nc
    return qr, cr, mask, pairwise, pool, grid_dS(seed + 1, (B, Y))
