"""TEST-ONLY inputs for the postings / query-batch builders: the repr dicts the tests/golden/ivf_*.npz fixtures were made from, rebuilt
from the fixture's seed as scripts/make_ivf_golden.py built them, and gaussian repr dicts of any shape and dtype."""
import numpy as np
import torch

import _ivf_fixture as F
import _multivec_oracle as MO

NQ, LQ, NDOC, LD, D, NEXP = 4, 6, 20, 7, 32, 6  # scripts/make_ivf_golden.py


def pad_last(r):
    """The last token of every sequence becomes padding: zero vector, weight 0 (scripts/make_ivf_golden.py:pad_last)."""
    r = {k: v.clone() for k, v in r.items()}
    r["expert_repr"][:, -1] = 0
    r["expert_weights"][:, -1] = 0
    w = r["expert_weights"]
    r["attention_mask"] = (w.reshape(w.shape[0], w.shape[1], -1).sum(-1) > 0).long()
    return r


def golden_inputs(name):
    """(meta, arrays, query repr dict, context repr dict) of a fixture; CLS vectors come from the fixture's own arrays."""
    meta, z = F.load(name)
    qr, cr, _ = MO.make_inputs(meta["seed"], meta["kind"], B=NQ, LQ=LQ, Nc=NDOC, LD=LD, d=D, KQ=meta["KQ"], KD=meta["KD"], n_experts=NEXP)
    qr, cr = pad_last(qr), pad_last(cr)
    for r in (qr, cr):
        r["expert_repr"], r["expert_weights"] = r["expert_repr"].float(), r["expert_weights"].float()
    if "cls_q" in z:
        qr["cls_repr"], cr["cls_repr"] = torch.from_numpy(z["cls_q"]), torch.from_numpy(z["cls_doc"])
    return meta, z, qr, cr


def gaussian_repr(seed, B, L, K, d, dtype=torch.float32, wdtype=None, n_experts=50, coil=False, pad=True):
    """A repr dict of gaussian vectors and uniform weights; about a fifth of the CITADEL weights are exactly 0; ragged lengths."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, d, generator=g).to(dtype)
    shape = (B, L) if coil else (B, L, K)
    ids = torch.randint(0, n_experts, shape, generator=g)
    w = torch.rand(shape, generator=g)
    if not coil:
        w = w * (torch.rand(shape, generator=g) > 0.2)
    lens = torch.randint(1, L + 1, (B,), generator=g) if pad else torch.full((B,), L)
    att = (torch.arange(L)[None, :] < lens[:, None]).long()
    return {"expert_repr": x, "expert_ids": ids, "expert_weights": w.to(wdtype if wdtype is not None else dtype), "attention_mask": att}


def to_device(r, dev):
    return {k: v.to(dev) for k, v in r.items()}


def same_batch(a, b):
    """QueryBatch a == QueryBatch b, tensor for tensor (bf16 compared by bits)."""
    assert a.nq == b.nq
    for k in ("ent_vec", "ent_q", "bexp", "boff", "cls"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is None:
            continue
        x, y = x.cpu(), y.cpu()
        assert x.dtype == y.dtype and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        if x.dtype == torch.bfloat16:
            x, y = x.view(torch.int16), y.view(torch.int16)
        assert torch.equal(x, y), k
    return True


def same_index(a, b):
    """IVFIndex a == IVFIndex b, tensor for tensor."""
    assert (a.corpus_len, a.d, a.dp, a.dc, a.n_experts, a.n_postings) == (b.corpus_len, b.d, b.dp, b.dc, b.n_experts, b.n_postings)
    for k in ("post_doc", "post_vec", "exp_off", "cls"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is None:
            continue
        x, y = x.cpu(), y.cpu()
        assert x.dtype == y.dtype and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        if x.dtype == torch.bfloat16:
            x, y = x.view(torch.int16), y.view(torch.int16)
        assert torch.equal(x, y), k
    return True


def read_tree(root, rank=0):
    """{expert id: (ids, weights, reprs)} of expert_{rank:04}, and the CLS tensor or None."""
    import glob
    import os
    import pickle

    out = {}
    for path in glob.glob(os.path.join(root, f"expert_{rank:04}", "*.pkl")):
        with open(path, "rb") as f:
            out[int(os.path.basename(path)[:-4])] = pickle.load(f)
    cls = None
    p = os.path.join(root, f"cls_{rank:04}.pkl")
    if os.path.exists(p):
        with open(p, "rb") as f:
            cls = pickle.load(f)
    return out, cls


def check_tree_against_fixture(root, z):
    files, cls = read_tree(root)
    assert sorted(files) == sorted(int(e) for e in np.unique(z["post_expert"]))
    for e, (ids, w, v) in files.items():
        sel = z["post_expert"] == e
        assert ids.dtype == torch.int64 and w.dtype == torch.float32 and v.dtype == torch.float32
        assert np.array_equal(ids.numpy(), z["post_doc"][sel]) and np.array_equal(w.numpy(), z["post_weight"][sel])
        assert np.array_equal(v.numpy(), z["post_vec"][sel])
        assert ids.untyped_storage().nbytes() == ids.numel() * 8 and v.untyped_storage().nbytes() == v.numel() * 4  # no shared storage
    if "cls_doc" in z:
        assert cls.dtype == torch.float32 and np.array_equal(cls.numpy(), z["cls_doc"])
    else:
        assert cls is None
