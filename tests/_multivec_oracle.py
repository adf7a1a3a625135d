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
