"""fp64 restatement of the CITADEL / SPLADE encoder head (reference: dpr_scale/models/citadel_models/citadel_model.py:46-82,
splade_model.py:26-32) with the tie rules of DESIGN.md section 11.  numpy only; the checker of tests/test_router_head*.py, never the
product.

    x[b,t,v] = logits[b, t + skip, v]      m[b,t] = attention_mask[b, t + skip]      T = T1 - skip      (citadel_model.py:50-52)
    f        = log(1 + relu(x)) * m                                                  (:55; the log of the FP32-rounded 1 + relu(x))
    router_repr = max_t f, argmax = the lowest such t                                (:56)
    expert_weights, expert_ids = top-k over v of f: value descending, then index ascending      (:58)
    router_mask = sum_t onehot(expert_ids) * (expert_weights > 0)                    (:63-64, :72)
    softmax_sum = sum_t softmax_v(x)  -- not masked                                  (:71, :73)
    avg_cond_num_experts / avg_marg_num_experts                                      (:66, :68)
"""
import numpy as np


def f_of(x, m):
    """log(1 + relu(x)) * m in fp64, of the fp32-rounded sum 1 + relu(x) (the reference adds in fp32 before its log)."""
    one_plus = (np.float32(1.0) + np.maximum(x, 0).astype(np.float32)).astype(np.float64)
    return np.log(one_plus) * m[..., None]


def forward(logits, attention_mask, k=1, skip=1, want_softmax=True):
    """logits [B, T1, V] (any float dtype: widened exactly), attention_mask [B, T1].  Returns a dict of fp64 / int64 arrays."""
    x = np.asarray(logits)[:, skip:, :].astype(np.float64)
    m = (np.asarray(attention_mask)[:, skip:] != 0).astype(np.float64)
    B, T, V = x.shape
    f = f_of(x, m)
    out = {"f": f, "router_repr": f.max(1), "argmax": f.argmax(1)}  # np.argmax: the first maximum = the lowest t
    if k > 0:
        order = np.argsort(-f, axis=2, kind="stable")[:, :, :k]     # stable on -f: value descending, then index ascending
        out["expert_ids"] = order.astype(np.int64)
        out["expert_weights"] = np.take_along_axis(f, order, 2)
        rm = np.zeros((B, V), np.float64)
        for b in range(B):
            np.add.at(rm[b], order[b].reshape(-1), (out["expert_weights"][b].reshape(-1) > 0).astype(np.float64))
        out["router_mask"] = rm
        out["avg_cond_num_experts"] = rm.sum(1, keepdims=True).mean(0, keepdims=True)
        out["avg_marg_num_experts"] = rm.max(0, keepdims=True).sum(1, keepdims=True)
    if want_softmax:
        e = np.exp(x - x.max(2, keepdims=True))
        p = e / e.sum(2, keepdims=True)
        out["p"] = p
        out["router_softmax_repr"] = p.sum(1)
    return out


def backward(logits, attention_mask, fwd, g_router=None, g_weights=None, g_soft=None, skip=1):
    """dlogits [B, T1, V] fp64 from the three incoming gradients (each may be None); `fwd` is forward()'s dict.
        dlogits[b, t+skip, v] = g_router[b,v] [t == argmax[b,v]] df + sum_j g_weights[b,t,j] [v == expert_ids[b,t,j]] df
                              + p (g_soft[b,v] - sum_u p[b,t,u] g_soft[b,u]),        df = m (x > 0) / (1 + x)"""
    x = np.asarray(logits)[:, skip:, :].astype(np.float64)
    m = (np.asarray(attention_mask)[:, skip:] != 0).astype(np.float64)
    B, T, V = x.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        df = np.where(x > 0, 1.0 / (1.0 + x), 0.0) * m[..., None]
    d = np.zeros((B, T, V))
    if g_router is not None:
        hit = np.arange(T)[None, :, None] == fwd["argmax"][:, None, :]
        d += np.where(hit, np.asarray(g_router, np.float64)[:, None, :], 0.0) * df
    if g_weights is not None:
        gw = np.zeros((B, T, V))
        np.put_along_axis(gw, fwd["expert_ids"], np.asarray(g_weights, np.float64), 2)  # the ids of a row are distinct
        d += gw * df
    if g_soft is not None:
        p, gs = fwd["p"], np.asarray(g_soft, np.float64)[:, None, :]
        d += p * (gs - (p * gs).sum(2, keepdims=True))
    full = np.zeros((B, T + skip, V))
    full[:, skip:] = d
    return full


def grid_logits(rng, B, T1, V):
    """Multiples of 1/64 in [-4, 4): ties are frequent, distinct values' logs lie far apart."""
    return (rng.integers(-256, 256, size=(B, T1, V)) / 64.0).astype(np.float32)


def masks(rng, B, T1):
    """A prefix mask per sequence; sequence 1 (if any) gets a hole, the last one (B >= 3) is fully masked."""
    m = np.zeros((B, T1), np.int64)
    for b in range(B):
        m[b, : int(rng.integers(1, T1 + 1))] = 1
    if B >= 2 and T1 >= 3:
        m[1, :] = 1
        m[1, T1 // 2] = 0
    if B >= 3:
        m[B - 1, :] = 0
    return m
