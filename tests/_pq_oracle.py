"""TEST-ONLY restatement of the product quantiser's rules in numpy: the encode rule in float32 with every
operation rounded on its own, the float64 distances it is compared with, and the decode loop."""
import numpy as np


def encode(x, codebook):
    """codes uint8 [n, m]: x float32 [n, m * dsub] (bf16 values, widened), codebook float32 [m, 256, dsub].  Per subspace the
    centroids are scanned c = 0 .. 255 with a strict <; D(c) = sum over t in increasing order of (x_t - cb_t)^2, each subtract,
    multiply and add a float32 operation of its own.  A NaN distance never wins; a row of NaNs keeps code 0."""
    x, codebook = np.asarray(x, np.float32), np.asarray(codebook, np.float32)
    m, _, dsub = codebook.shape
    n = x.shape[0]
    codes = np.zeros((n, m), np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(m):
            best = np.full(n, np.inf, np.float32)
            for c in range(256):
                for t in range(dsub):
                    diff = x[:, j * dsub + t] - codebook[j, c, t]
                    sq = diff * diff
                    D = sq if t == 0 else D + sq
                assert D.dtype == np.float32
                win = D < best
                best[win] = D[win]
                codes[win, j] = c
    return codes


def distances64(x, codebook):
    """float64 [n, m, 256]: the squared distances of every sub-vector to every centroid of its subspace."""
    x, codebook = np.asarray(x, np.float64), np.asarray(codebook, np.float64)
    m, _, dsub = codebook.shape
    return ((x.reshape(-1, m, 1, dsub) - codebook[None]) ** 2).sum(-1)


def decode(codes, codebook):
    m, _, dsub = codebook.shape
    out = np.zeros((codes.shape[0], m * dsub), codebook.dtype)
    for p in range(codes.shape[0]):
        for j in range(m):
            for t in range(dsub):
                out[p, j * dsub + t] = codebook[j, codes[p, j], t]
    return out
