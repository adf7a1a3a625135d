"""The one reference of the per-row top-k fold every retrieval path ends in (include/dprhot.h: dprhot_topk, dprhot_topk_update,
dprhot_topk_update_wide), and the score matrices that are hard on a selection kernel.  numpy only.

The contract: candidates are the filled slots of the state (id >= 0) and the columns of the chunk (id = col_offset + j); a NaN score of
any sign or payload is no candidate; the rest is ordered by score descending under FLOAT comparison (+0 and -0 tie), then id
ascending; the first k are the new state, values with the candidates' own bit patterns; slots beyond the candidates hold -inf / -1."""
import numpy as np

_I64MAX = np.iinfo(np.int64).max


def fold(state, S, col_offset, k):
    """state: None or (values [rows, k] fp32, ids [rows, k] int64); S: [rows, cols] fp32 -> (values, ids) after folding S in."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    rows = S.shape[0]
    v = S
    ids = np.broadcast_to(np.int64(col_offset) + np.arange(S.shape[1], dtype=np.int64), S.shape)
    if state is not None:
        v = np.concatenate([np.asarray(state[0], dtype=np.float32), v], axis=1)
        ids = np.concatenate([np.asarray(state[1], dtype=np.int64), ids], axis=1)
    dropped = (ids < 0) | np.isnan(v)  # 1. unfilled slots, 2. NaN
    key = -np.where(dropped, np.float32(0), v).astype(np.float64)  # (fp32 -> fp64 is exact; -(+0) == -(-0) as floats: the id decides)
    order = np.lexsort((ids, key, dropped), axis=1)[:, :k]  # 3. real candidates first, score descending, id ascending
    real = ~np.take_along_axis(dropped, order, axis=1)
    out_v = np.full((rows, k), -np.inf, dtype=np.float32)
    out_i = np.full((rows, k), -1, dtype=np.int64)
    n = order.shape[1]
    out_v[:, :n] = np.where(real, np.take_along_axis(v, order, axis=1), np.float32(-np.inf))  # (np.where copies bit patterns)
    out_i[:, :n] = np.where(real, np.take_along_axis(ids, order, axis=1), -1)
    return out_v, out_i


def fold_pieces(S, edges, col_offset, k):
    """fold over the column pieces [edges[i], edges[i + 1]) of S in turn (empty pieces are left out), from an empty state."""
    st = None
    for a, b in zip(edges[:-1], edges[1:]):
        if b > a:
            st = fold(st, S[:, a:b], col_offset + a, k)
    return st


# bit patterns of the `specials` mode, about 2 % of the entries each: +NaN, -NaN, a signalling NaN, the all-ones NaN, +-inf, +-0, the
# smallest subnormals, the largest finite values
SPECIAL_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                0x7F7FFFFF, 0xFF7FFFFF)
MODES = ("gauss", "levels", "constant", "specials", "nan_rows")


def nan_keep(k, cols):
    """Non-NaN values per row (r % 6) of the `nan_rows` mode: more than k, exactly k, one short of k, a few, none, all."""
    return [min(n, cols) for n in (k + 40, k, k - 1, 5, 0, cols)]


def adversarial(rows, cols, seed, mode, k=None):
    """[rows, cols] fp32 scores.  gauss; levels: integers from 1-5 levels per row (thousands of ties, also at the k-th score); constant:
    one value per row, rows r % 6 == 1 and 5 all -inf, row 2 all NaN; specials: Gaussian with SPECIAL_BITS written in as bit patterns
    (the signs of NaN and zero survive); nan_rows (needs k): row r keeps exactly nan_keep(k, cols)[r % 6] non-NaN values at random
    places, the NaNs of both signs."""
    rng = np.random.default_rng(seed)
    if mode == "gauss":
        return rng.standard_normal((rows, cols)).astype(np.float32)
    if mode == "levels":
        nlev = rng.integers(1, 6, size=(rows, 1))
        return np.floor(rng.random((rows, cols)) * nlev).astype(np.float32)
    if mode == "constant":
        per_row = [7.0, -np.inf, 0.0, float(rng.standard_normal()), -0.0, -np.inf]
        S = np.array([per_row[r % 6] for r in range(rows)], dtype=np.float32)[:, None].repeat(cols, axis=1)
        if rows > 2:
            S[2] = np.nan
        return np.ascontiguousarray(S)
    if mode == "specials":
        u = rng.standard_normal((rows, cols)).astype(np.float32).view(np.uint32).copy()
        pick = rng.integers(0, 50, size=(rows, cols))  # value j < len(SPECIAL_BITS): 2 % each
        for j, bits in enumerate(SPECIAL_BITS):
            u[pick == j] = np.uint32(bits)
        return u.view(np.float32)
    if mode == "nan_rows":
        assert k is not None, "nan_rows needs k"
        u = rng.standard_normal((rows, cols)).astype(np.float32).view(np.uint32).copy()
        keep = nan_keep(k, cols)
        for r in range(rows):
            gone = rng.permutation(cols)[keep[r % 6]:]
            u[r, gone] = np.where(rng.random(gone.size) < 0.5, np.uint32(0x7FC00000), np.uint32(0xFFC00000))
        return u.view(np.float32)
    raise ValueError(mode)
