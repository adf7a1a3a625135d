"""The CITADEL / SPLADE encoder head without a GPU: the fp64 oracle of tests/_router_head_oracle.py reproduces what the reference's own
CITADELEncoder.forward / SPLADEEncoder.forward returned (tests/golden/router_head_*.npz, written by scripts/make_router_head_golden.py),
and the three C-ABI entry points validate on the host."""
import ctypes

import numpy as np
import pytest
import torch

import _router_head_oracle as O
from conftest import load_golden

FIXTURES = ["router_head_citadel_k1", "router_head_citadel_k3", "router_head_splade"]


def _rel(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    err = np.abs(a - b)
    assert (err <= tol * np.abs(b)).all(), f"max relative error {np.max(err / np.maximum(np.abs(b), 1e-300)):.3e} > {tol}"


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_reference_fixture(name):
    meta, z = load_golden(name)
    k, skip = meta["k"], meta["skip"]
    fwd = O.forward(z["logits"], z["attention_mask"], k=k, skip=skip, want_softmax=k > 0)
    _rel(fwd["router_repr"], z["ret_router_repr"], 1e-6)
    # argmax: exact wherever the maximum is > 0.  The reference returns only the values of its max (citadel_model.py:56); the tokens
    # are those of the same expression in torch on the CPU
    tl, tm = torch.from_numpy(z["logits"][:, skip:]), torch.from_numpy(z["attention_mask"][:, skip:])
    ref_max = torch.max(torch.log(1 + torch.relu(tl)) * tm.unsqueeze(-1), dim=1)
    assert np.array_equal(ref_max.values.numpy(), z["ret_router_repr"])
    pos = z["ret_router_repr"] > 0
    assert pos.any() and np.array_equal(fwd["argmax"][pos], ref_max.indices.numpy()[pos])
    g_router = z["g_router_repr"]
    g_w = g_soft = None
    if k:
        live = z["ret_expert_weights"] > 0
        assert live.any() and np.array_equal(fwd["expert_ids"][live], z["ret_expert_ids"][live])
        _rel(fwd["expert_weights"], z["ret_expert_weights"], 1e-6)
        assert np.array_equal(fwd["router_mask"], z["ret_router_mask"])
        _rel(fwd["router_softmax_repr"], z["ret_router_softmax_repr"], 1e-6)
        _rel(fwd["avg_cond_num_experts"], z["ret_avg_cond_num_experts"], 1e-6)
        _rel(fwd["avg_marg_num_experts"], z["ret_avg_marg_num_experts"], 1e-6)
        g_w, g_soft = z["g_expert_weights"], z["g_router_softmax_repr"]
    d = O.backward(z["logits"], z["attention_mask"], fwd, g_router, g_w, g_soft, skip=skip)
    ref = z["dlogits"].astype(np.float64)
    assert d.shape == ref.shape and np.abs(ref).max() > 0
    assert np.abs(d - ref).max() <= 1e-6 * np.abs(ref).max()
    assert not d[:, :skip].any()


def test_oracle_tie_rules():
    """All-equal rows: the first k columns in order; all-equal columns: token 0; a masked token routes to columns 0 .. k-1, weight 0."""
    x = np.full((2, 4, 6), 0.5, np.float32)
    m = np.ones((2, 4), np.int64)
    m[1, 2] = 0
    fwd = O.forward(x, m, k=3, skip=1)
    assert np.array_equal(fwd["expert_ids"], np.broadcast_to(np.arange(3), (2, 3, 3)))
    assert not fwd["argmax"].any()
    assert not fwd["expert_weights"][1, 1].any() and fwd["expert_weights"][1, 0].all()
    assert np.array_equal(fwd["router_mask"][1], [2, 2, 2, 0, 0, 0])


def _fwd_args(lib, buf, dtype=2, B=2, T1=4, V=16, skip=1, k=2, null=False):
    p = None if null else ctypes.cast(buf, ctypes.c_void_p)
    return lib.dprhot_router_head_fwd(p, dtype, B, T1, V, T1 * V, V, p, skip, k, 1, p, p, p, p, p, p, p, 1 << 20, None)


def _bwd_args(lib, buf, dtype=2, B=2, T1=4, V=16, skip=1, k=2, null=False):
    p = None if null else ctypes.cast(buf, ctypes.c_void_p)
    return lib.dprhot_router_head_bwd(p, dtype, B, T1, V, T1 * V, V, p, skip, k, p, p, p, 1 << 20, p, p, p, p, None)


def test_entry_points_validate_on_the_host():
    """Nothing here reaches a launch: every call is refused by the host-side checks (the pointers are host memory)."""
    from dpr_scale_amd import _lib

    lib = _lib.lib
    buf = (ctypes.c_float * 16)()
    for call in (_fwd_args, _bwd_args):
        assert call(lib, buf, null=True) == -1 and b"NULL" in lib.dprhot_last_error()
        assert call(lib, buf, k=9) == -1 and b"k=9" in lib.dprhot_last_error()
        assert call(lib, buf, V=2, k=3) == -1 and b"V=2" in lib.dprhot_last_error()
        assert call(lib, buf, T1=1, skip=1) == -1 and b"T >= 1" in lib.dprhot_last_error()   # T = 0
        assert call(lib, buf, T1=0, skip=0) == -1
        assert call(lib, buf, dtype=3) == -1 and b"dtype=3" in lib.dprhot_last_error()
        assert call(lib, buf, dtype=-1) == -1
    out = ctypes.c_size_t(0)
    assert lib.dprhot_router_head_workspace_bytes(2, 4, 16, 2, 1, None) == -1
    assert lib.dprhot_router_head_workspace_bytes(2, 4, 16, 9, 1, ctypes.byref(out)) == -1
    assert lib.dprhot_router_head_workspace_bytes(2, 4, 2, 3, 1, ctypes.byref(out)) == -1
    assert lib.dprhot_router_head_workspace_bytes(2, 0, 16, 2, 1, ctypes.byref(out)) == -1
    assert lib.dprhot_router_head_workspace_bytes(0, 4, 16, 2, 1, ctypes.byref(out)) == -1


def test_workspace_query_is_total():
    from dpr_scale_amd import _lib

    for B in (1, 300):
        for T in (1, 511):
            for V in (8, 30522):
                for k in (0, 1, 8):
                    n = _lib.router_head_workspace_bytes(B, T, V, k, True)
                    assert n >= B * T * 4 and n % 256 == 0          # the rows' logsumexp
                    assert n <= B * T * 4 + 256                      # nothing vocabulary-sized
                    assert _lib.router_head_workspace_bytes(B, T, V, k, False) == 0
