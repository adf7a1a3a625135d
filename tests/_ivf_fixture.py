"""TEST-ONLY helpers around the tests/golden/ivf_*.npz fixtures: the unpacked structures the oracle takes, and the on-disk index
tree rebuilt from the arrays (pickles are not committed)."""
import os
import pickle

import numpy as np
import torch

from conftest import load_golden

NAMES = ["ivf_coil", "ivf_coil_cls", "ivf_citadel11", "ivf_citadel11_cls", "ivf_citadel23", "ivf_citadel23_cls"]


def load(name):
    meta, z = load_golden(name)
    return meta, z


def postings(z):
    out = {}
    for e in np.unique(z["post_expert"]):
        sel = z["post_expert"] == e
        out[int(e)] = (z["post_doc"][sel], z["post_vec"][sel])
    return out


def queries(meta, z, dtype=None):
    """The per-query dictionaries in the listed order; vectors in the dtype the reference's task produced (or `dtype`)."""
    dt = dtype if dtype is not None else (torch.float16 if meta["entry_dtype"] == ["torch.float16"] else torch.float32)
    emb = [dict() for _ in range(meta["nq"])]
    wts = [dict() for _ in range(meta["nq"])]
    for n, e, v, w in zip(z["ent_query"], z["ent_expert"], z["ent_vec"], z["ent_weight"]):
        emb[int(n)].setdefault(int(e), []).append(torch.from_numpy(v).to(dt))
        wts[int(n)].setdefault(int(e), []).append(torch.tensor(float(w)).to(dt))
    cls = torch.from_numpy(z["cls_q"]) if "cls_q" in z else []
    return cls, emb, wts


def write_tree(root, z, splits=1):
    """expert_{rank:04}/{id}.pkl + cls_{rank:04}.pkl as the index writer lays them out; `splits` ranks own consecutive doc ranges."""
    n_docs = int(z["scores"].shape[1])
    edges = [n_docs * r // splits for r in range(splits + 1)]
    for r in range(splits):
        lo, hi = edges[r], edges[r + 1]
        d = os.path.join(root, f"expert_{r:04}")
        os.makedirs(d, exist_ok=True)
        for e in np.unique(z["post_expert"]):
            sel = (z["post_expert"] == e) & (z["post_doc"] >= lo) & (z["post_doc"] < hi)
            if sel.any():
                with open(os.path.join(d, f"{int(e)}.pkl"), "wb") as f:
                    pickle.dump((torch.from_numpy(z["post_doc"][sel]), torch.from_numpy(z["post_weight"][sel]),
                                 torch.from_numpy(z["post_vec"][sel])), f, protocol=4)
        if "cls_doc" in z:
            with open(os.path.join(root, f"cls_{r:04}.pkl"), "wb") as f:
                pickle.dump(torch.from_numpy(z["cls_doc"][lo:hi]), f, protocol=4)
    return root
