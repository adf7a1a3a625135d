"""The reference of the SPAR score (include/dprhot.h, dprhot_spar_score): s[w][i][j] = <q1[i], c1[j]> + lam[w] * <q2[i], c2[j]> in float64,
and the total-order top-k of tests/_topk_oracle.py on top of it.  numpy only.

Grid inputs (every feature a multiple of 1/8 in [-1, 1], d <= 256, lam in {0.25, 0.5, 1, 2, 4}): every product is a multiple of 1/64,
every partial sum a multiple of 1/64 below 2^8, lam * acc2 + acc1 a multiple of 1/256 below 2^11 -- all exact in fp32 in any order, so
a kernel's fp32 score must equal this float64 score bit for bit."""
import numpy as np

import _topk_oracle as TO

GRID_LAMS = (0.25, 0.5, 1.0, 2.0, 4.0)


def score(q1, q2, c1, c2, lams):
    """[W, nq, n] float64."""
    q1, q2, c1, c2 = (np.asarray(x, dtype=np.float64) for x in (q1, q2, c1, c2))
    lam = np.asarray(lams, dtype=np.float64).reshape(-1, 1, 1)
    return (q1 @ c1.T)[None] + lam * (q2 @ c2.T)[None]


def bound(q1, q2, c1, c2, lams):
    """Per-cell error bound of a kernel that accumulates exact bf16 products in fp32 and applies one fp32 fma:
    2^-23 * ((d1 + 1) * A1 + |lam| * (d2 + 1) * A2), A = |Q| |C|^T."""
    q1, q2, c1, c2 = (np.abs(np.asarray(x, dtype=np.float64)) for x in (q1, q2, c1, c2))
    lam = np.abs(np.asarray(lams, dtype=np.float64)).reshape(-1, 1, 1)
    return 2.0 ** -23 * ((q1.shape[1] + 1) * (q1 @ c1.T)[None] + lam * (q2.shape[1] + 1) * (q2 @ c2.T)[None])


def topk(S, k, col_offset=0):
    """S [..., n] fp32 -> (values [..., k] fp32, ids [..., k] int64) under the total order; NaN never selected, -inf / -1 tails."""
    S = np.asarray(S, dtype=np.float32)
    v, i = TO.fold(None, S.reshape(-1, S.shape[-1]), col_offset, k)
    return v.reshape(S.shape[:-1] + (k,)), i.reshape(S.shape[:-1] + (k,))


def grid(rng, *shape):
    """Multiples of 1/8 in [-1, 1], fp32."""
    return (rng.integers(-8, 9, size=shape) / 8.0).astype(np.float32)


def grid_lams(W):
    return [GRID_LAMS[w % len(GRID_LAMS)] for w in range(W)]
