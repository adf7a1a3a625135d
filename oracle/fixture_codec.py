"""TEST INFRASTRUCTURE: compact, lossless storage of the reference's fp32 outputs next to an oracle that recomputes them.

A reference array x is stored as int16 offsets from `base` (the fp64 oracle, rounded to fp32) on the fp32 grid (shift 0:
units in the last place) or on the bf16 grid (shift 16, for bf16-representable x); an element whose offset does not fit in
int16 is stored as its own value.  Because the base is recomputed by the code under test, x also carries a fingerprint that
does not depend on it: the positions of its non-finite elements and eight projections of its finite values on fixed random
+-1 vectors (fp64).  decode() rebuilds x and checks it against that fingerprint, so a changed oracle cannot carry the
reference along with it: one element off by more than ~1e-9 of the array's L2 norm fails the check, while an fp64 oracle
recomputed on another host (~1e-16 of the largest value) passes it.  Stored per name: <name>_ulp, <name>_at (flat indices of
the elements stored as values), <name>_val, <name>_inf, <name>_proj, <name>_norm.
"""
import numpy as np

_PROJ_TOL = 1e-9  # of the array's L2 norm


def _grid(base, shift):
    b = np.array(base, np.float64).astype(np.float32)
    if shift:
        import torch

        b = torch.from_numpy(b.reshape(-1)).to(torch.bfloat16).float().numpy().reshape(b.shape)  # round to nearest even
    return b.view(np.int32).astype(np.int64) >> shift


def _fingerprint(x):
    v = np.array(x, np.float64).reshape(-1)
    fin = np.isfinite(v)
    v = np.where(fin, v, 0.0)
    signs = np.random.default_rng(v.size).integers(0, 2, (8, v.size)) * 2.0 - 1.0
    return np.flatnonzero(~fin).astype(np.int32), signs @ v, np.sqrt(np.sum(v * v))


def encode(name, x, base, shift=0):
    x = np.array(x, np.float32)
    off = np.array((x.view(np.int32).astype(np.int64) >> shift) - _grid(base, shift))  # (np.array: 0-d stays an array)
    far = np.flatnonzero(np.abs(off) > np.iinfo(np.int16).max)
    off.reshape(-1)[far] = 0
    inf, proj, norm = _fingerprint(x)
    return {name + "_ulp": off.astype(np.int16), name + "_at": far.astype(np.int32), name + "_val": x.reshape(-1)[far],
            name + "_inf": inf, name + "_proj": proj, name + "_norm": np.float64(norm)}


def decode(arrays, name, base, shift=0):
    x = np.array((_grid(base, shift) + arrays[name + "_ulp"]) << shift).astype(np.int32).view(np.float32)
    x.reshape(-1)[arrays[name + "_at"]] = arrays[name + "_val"]
    inf, proj, norm = _fingerprint(x)
    assert np.array_equal(inf, arrays[name + "_inf"]), f"{name}: the base no longer decodes to the stored array (non-finite set)"
    assert np.abs(proj - arrays[name + "_proj"]).max() <= _PROJ_TOL * max(float(arrays[name + "_norm"]), 1e-30), \
        f"{name}: the base no longer decodes to the stored array (projections)"
    return x
