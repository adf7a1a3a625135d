#!/usr/bin/env python3
"""Writes tests/golden/router_head_*.npz from the REFERENCE's own encoder heads, run unmodified on the CPU:
dpr_scale/models/citadel_models/citadel_model.py:46-82 (CITADELEncoder.forward) and splade_model.py:26-32 (SPLADEEncoder.forward).

    DPR_REFERENCE_ROOT=/path/to/dpr-scale python scripts/make_router_head_golden.py

The encoders' constructors load a checkpoint (citadel_model.py:22-28); nothing is downloaded here: the instance is made without
__init__, its projections are the Identity of :30 / :38, and `self.transformer` is a stub that returns stored tensors (logits
[B, T1, V] and one hidden-state layer).  `dpr_scale.utils.utils` (PathManager, unused by forward) is stubbed for the import.

Shape: B = 3, T1 = 8, V = 509, k in {1, 3}; sequence 1 has a hole in its mask, sequence 2 a fully padded tail.  The logits of one
sequence are DISTINCT multiples of 1/1024 in [-8, 8): 1 + x is exact in fp32, so no two positive f tie within a row or a column and the
reference's own topk / max are defined wherever they are compared.  The gradient is that of the fixed scalar
    L = sum(router_repr * g_router) + sum(expert_weights * g_weights) + sum(router_softmax_repr * g_soft)
with respect to the full logits (the three weight tensors are stored)."""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("DPR_REFERENCE_ROOT", "/root/reference")
B, T1, V, H = 3, 8, 509, 16


def load_reference_encoders():
    stub = types.ModuleType("dpr_scale.utils.utils")
    stub.PathManager = type("PathManager", (), {"get_local_path": staticmethod(lambda p: p)})
    sys.modules["dpr_scale.utils.utils"] = stub
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    from dpr_scale.models.citadel_models.citadel_model import CITADELEncoder
    from dpr_scale.models.citadel_models.splade_model import SPLADEEncoder

    for cls in (CITADELEncoder, SPLADEEncoder):
        path = os.path.realpath(sys.modules[cls.__module__].__file__)
        assert path.startswith(os.path.realpath(REFERENCE_ROOT)), f"{cls.__name__} resolved outside the reference tree: {path}"
    return CITADELEncoder, SPLADEEncoder


class StubTransformer(torch.nn.Module):
    def __init__(self, logits, hidden):
        super().__init__()
        self.logits, self.hidden = logits, hidden

    def forward(self, return_dict=True, **tokens):
        return types.SimpleNamespace(logits=self.logits, hidden_states=(self.hidden,))


def bare(cls, transformer):
    enc = cls.__new__(cls)
    torch.nn.Module.__init__(enc)
    enc.transformer = transformer
    enc.cls_project = torch.nn.Identity()
    enc.tok_project = torch.nn.Identity()
    return enc


def inputs(seed):
    rng = np.random.default_rng(seed)
    logits = np.stack([rng.permutation(16384)[: T1 * V].reshape(T1, V) - 8192 for _ in range(B)]).astype(np.float32) / 1024.0
    hidden = rng.standard_normal((B, T1, H)).astype(np.float32)
    mask = np.ones((B, T1), np.int64)
    mask[1, 4] = 0   # a hole
    mask[2, 5:] = 0  # a fully padded tail
    return logits, hidden, mask


def main():
    CITADELEncoder, SPLADEEncoder = load_reference_encoders()
    out_dir = os.path.join(ROOT, "tests", "golden")
    for name, k in (("citadel_k1", 1), ("citadel_k3", 3), ("splade", 0)):
        logits, hidden, mask = inputs(20240 + k)
        assert ((logits[:, 1:] > 0).sum(2) >= max(k, 1)).all()
        rng = np.random.default_rng(77 + k)
        tl = torch.from_numpy(logits).requires_grad_(True)
        tokens = {"input_ids": torch.zeros((B, T1), dtype=torch.long), "attention_mask": torch.from_numpy(mask)}
        stub = StubTransformer(tl, torch.from_numpy(hidden))
        arrays = {"logits": logits, "hidden": hidden, "attention_mask": mask}
        if k:
            ret = bare(CITADELEncoder, stub)(tokens, topk=k, add_cls=True)
            g = {"router_repr": rng.standard_normal((B, V)).astype(np.float32),
                 "expert_weights": rng.standard_normal((B, T1 - 1, k)).astype(np.float32),
                 "router_softmax_repr": rng.standard_normal((B, V)).astype(np.float32)}
            scalar = sum((ret[key] * torch.from_numpy(w)).sum() for key, w in g.items())
            arrays.update({f"g_{key}": w for key, w in g.items()})
        else:
            ret = {"router_repr": bare(SPLADEEncoder, stub)(tokens)}
            g = rng.standard_normal((B, V)).astype(np.float32)
            scalar = (ret["router_repr"] * torch.from_numpy(g)).sum()
            arrays["g_router_repr"] = g
        scalar.backward()
        arrays.update({f"ret_{key}": v.detach().numpy() for key, v in ret.items()})
        arrays["dlogits"] = tl.grad.numpy()
        meta = {"B": B, "T1": T1, "V": V, "H": H, "k": k, "skip": 1, "encoder": "citadel" if k else "splade",
                "source": "citadel_model.py:46-82" if k else "splade_model.py:26-32", "torch": torch.__version__}
        path = os.path.join(out_dir, f"router_head_{name}.npz")
        np.savez_compressed(path, meta=json.dumps(meta), **arrays)
        print(f"{path}: {os.path.getsize(path)} bytes, keys {sorted(arrays)}")


if __name__ == "__main__":
    main()
