"""The routes of InBatchContrastive, pinned on CPU: for every way through forward / backward that needs no GPU, the exact sequence
of kernel-set calls (name, tensor shapes and dtypes, scalars), the loss and the gradients against the numpy oracle, and -- for the
routes whose gradients are computed in forward -- that the operator lets go of the gradient tensors it hands to autograd.

The kernel set is tests/_oracle_kernels.OracleKernels behind a recorder; a case sets what the library's plan would decide for its
shape (keep_G, slabs, bf16_dc) on the instance.  The multi-rank code path runs on a one-rank gloo world through dist.force_dist."""
import gc
import os
import sys
import weakref

import numpy as np
import pytest
import torch
import torch.distributed as dist

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
from _oracle_kernels import OracleKernels  # noqa: E402
from oracle import inbatch_oracle as O  # noqa: E402

from dpr_scale_amd import dist as D  # noqa: E402
from dpr_scale_amd import hotpath  # noqa: E402
from dpr_scale_amd.hotpath import ContextGather, defer_context_grad, inbatch_contrastive_loss  # noqa: E402

_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.uint8: "u8", torch.int64: "i64", torch.bool: "bool"}
T = 1.0


def _enc(a):
    if isinstance(a, torch.Tensor):
        return f"{_DT[a.dtype]}{list(a.shape)}"
    if isinstance(a, torch.dtype):
        return _DT[a]
    if isinstance(a, (tuple, list)):
        return "(" + ", ".join(_enc(x) for x in a) + ("," if len(a) == 1 else "") + ")"
    if isinstance(a, float):
        return f"{a:.6g}"
    return repr(a)


class Recorder:
    """Logs every kn.* call of the operator."""

    name = "recorder"

    def __init__(self, inner):
        self._inner, self.log = inner, []
        self.handed = {}  # what the last train step returned: data pointers and weak references, never the tensors

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        f = getattr(self._inner, name)
        if not callable(f):
            return f

        def call(*a, **k):
            self.log.append(f"{name}(" + ", ".join([_enc(x) for x in a] + [f"{n}={_enc(v)}" for n, v in sorted(k.items())]) + ")")
            out = f(*a, **k)
            if name in ("train_step_f32", "train_step_packed_f32"):
                dQ, dC = out[4], out[5]
                dQ = dQ[0] if isinstance(dQ, tuple) else dQ
                self.handed = {"dq_ptr": dQ.data_ptr(), "dc_ptr": dC.data_ptr(), "dq": weakref.ref(dQ), "dc": weakref.ref(dC)}
            return out

        return call


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# name -> dict(kn: the plan attributes of the kernel set, B / K: shape (d = 16), dtype: of q and c, env: variables set,
#              multi: the multi-rank path on a one-rank world, overlap: ContextGather + defer_context_grad, grads: backward runs)
CASES = {
    "single_bf16": dict(dtype=torch.bfloat16),
    "single_fp16": dict(dtype=torch.float16),
    "single_no_grad": dict(grads=False),
    "single_train_step_G": dict(kn=dict(keep_G=True)),
    "single_train_step_noG": dict(kn=dict(keep_G=False)),
    "single_train_step_slabs_noG": dict(kn=dict(keep_G=False, slabs=True)),
    "single_padded": dict(B=3),
    "single_fp32g_debug": dict(env={"DPRHOT_FP32_G": "1"}),
    "single_fp32g_debug_bf16": dict(env={"DPRHOT_FP32_G": "1"}, dtype=torch.bfloat16),
    "multi_train_fp32wire_G": dict(multi=True, kn=dict(keep_G=True), env={"DPRHOT_DC_WIRE": "fp32"}),
    "multi_train_fp32wire_noG": dict(multi=True, kn=dict(keep_G=False, slabs=True), env={"DPRHOT_DC_WIRE": "fp32"}),
    "multi_train_fp32wire_noG_overlap": dict(multi=True, overlap=True, kn=dict(keep_G=False), env={"DPRHOT_DC_WIRE": "fp32"}),
    "multi_train_bf16wire_G": dict(multi=True, kn=dict(keep_G=True), env={"DPRHOT_DC_WIRE": "bf16"}),
    "multi_train_bf16wire_noG_overlap": dict(multi=True, overlap=True, kn=dict(keep_G=False), env={"DPRHOT_DC_WIRE": "bf16"}),
    "multi_train_bf16wire_fallback_noG": dict(multi=True, kn=dict(keep_G=False, bf16_dc=False), env={"DPRHOT_DC_WIRE": "bf16"}),
    "multi_train_bf16wire_fallback_G_overlap": dict(multi=True, overlap=True, kn=dict(keep_G=True, bf16_dc=False),
                                                    env={"DPRHOT_DC_WIRE": "bf16"}),
    "multi_bf16_inputs": dict(multi=True, dtype=torch.bfloat16, env={"DPRHOT_DC_WIRE": "fp32"}),
    "multi_no_grad": dict(multi=True, grads=False, env={"DPRHOT_DC_WIRE": "fp32"}),
    "multi_no_grad_overlap": dict(multi=True, overlap=True, grads=False, env={"DPRHOT_DC_WIRE": "fp32"}),
}
PRESCALED = {n for n in CASES if "train" in n}

# The call logs: forward, backward, second backward through the retained graph (the same for grad_output 1 and 3).
EXPECTED = {
    "single_bf16": [
        "empty((4, 16), bf16, bf16[4, 16])",
        "empty((8, 16), bf16, bf16[8, 16])",
        "prep(bf16[4, 16], bf16[4, 16], bf16[8, 16], bf16[8, 16])",
        "inbatch_fwd(bf16[4, 16], bf16[8, 16], i64[4], 0, u8[8], 1, 0.25)",
        "-- backward",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
        "-- second backward",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
    ],
    "single_fp16": [
        "empty((4, 16), bf16, f16[4, 16])",
        "empty((8, 16), bf16, f16[8, 16])",
        "prep(f16[4, 16], bf16[4, 16], f16[8, 16], bf16[8, 16])",
        "inbatch_fwd(bf16[4, 16], bf16[8, 16], i64[4], 0, u8[8], 1, 0.25)",
        "-- backward",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
        "-- second backward",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
    ],
    "single_no_grad": [
        "empty((4, 16), bf16, f32[4, 16])",
        "empty((8, 16), bf16, f32[8, 16])",
        "inbatch_fwd_f32(f32[4, 16], f32[8, 16], bf16[4, 16], bf16[8, 16], i64[4], 0, u8[8], 1, 0.25)",
    ],
    "single_train_step_G": [
        "empty((4, 16), bf16, f32[4, 16])",
        "empty((8, 16), bf16, f32[8, 16])",
        "train_step_f32(f32[4, 16], f32[8, 16], bf16[4, 16], bf16[8, 16], i64[4], 0, u8[8], 1, 0.25, 0.25, f32[1], defer_dq=True, want_G='auto')",
        "-- backward",
        "rescale_grads(f32[4, 16], f32[8, 16], f32[1], f32[1])",
        "-- second backward",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
    ],
    "single_train_step_noG": [
        "empty((4, 16), bf16, f32[4, 16])",
        "empty((8, 16), bf16, f32[8, 16])",
        "train_step_f32(f32[4, 16], f32[8, 16], bf16[4, 16], bf16[8, 16], i64[4], 0, u8[8], 1, 0.25, 0.25, f32[1], defer_dq=True, want_G='auto')",
        "-- backward",
        "rescale_grads(f32[4, 16], f32[8, 16], f32[1], f32[1])",
        "-- second backward",
        "inbatch_fwd(bf16[4, 16], bf16[8, 16], i64[4], 0, u8[8], 1, 0.25)",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
    ],
    "single_train_step_slabs_noG": [
        "empty((4, 16), bf16, f32[4, 16])",
        "empty((8, 16), bf16, f32[8, 16])",
        "train_step_f32(f32[4, 16], f32[8, 16], bf16[4, 16], bf16[8, 16], i64[4], 0, u8[8], 1, 0.25, 0.25, f32[1], defer_dq=True, want_G='auto')",
        "-- backward",
        "rescale_grads((f32[4, 16], f32[2, 4, 16]), f32[8, 16], f32[1], f32[1])",
        "-- second backward",
        "inbatch_fwd(bf16[4, 16], bf16[8, 16], i64[4], 0, u8[8], 1, 0.25)",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
    ],
    "single_padded": [
        "empty((3, 16), bf16, f32[3, 16])",
        "empty((8, 16), bf16, f32[6, 16])",
        "empty((8,), u8, f32[6, 16])",
        "prep(f32[3, 16], bf16[3, 16], f32[6, 16], bf16[6, 16])",
        "inbatch_fwd(bf16[3, 16], bf16[8, 16], i64[3], 0, u8[8], 1, 0.333333)",
        "-- backward",
        "inbatch_bwd(bf16[3, 8], bf16[3, 16], bf16[8, 16], 1, f32[1], True, True)",
        "-- second backward",
        "inbatch_bwd(bf16[3, 8], bf16[3, 16], bf16[8, 16], 1, f32[1], True, True)",
    ],
    "single_fp32g_debug": [
        "empty((4, 16), bf16, f32[4, 16])",
        "empty((8, 16), bf16, f32[8, 16])",
        "inbatch_fwd_f32(f32[4, 16], f32[8, 16], bf16[4, 16], bf16[8, 16], i64[4], 0, u8[8], 1, 0.25, want_logits=True)",
        "-- backward",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
        "-- second backward",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
    ],
    "single_fp32g_debug_bf16": [
        "empty((4, 16), bf16, bf16[4, 16])",
        "empty((8, 16), bf16, bf16[8, 16])",
        "prep(bf16[4, 16], bf16[4, 16], bf16[8, 16], bf16[8, 16])",
        "inbatch_fwd(bf16[4, 16], bf16[8, 16], i64[4], 0, u8[8], 1, 0.25, want_logits=True)",
        "-- backward",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
        "-- second backward",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
        "inbatch_bwd(bf16[4, 8], bf16[4, 16], bf16[8, 16], 1, f32[1], True, True)",
    ],
    "multi_train_fp32wire_G": [
        "empty((4, 16), bf16, f32[4, 16])",
        "packed_rows(8, 16)",
        "empty((16, 16), bf16, f32[8, 16])",
        "pack_ctx(f32[8, 16], u8[8], bf16[16, 16])",
        "empty((16, 16), bf16, f32[8, 16])",
        "train_step_packed_f32(f32[4, 16], bf16[16, 16], bf16[4, 16], 1, 0, 8, i64[4], 1, 0.25, 0.25, f32[1], f32, defer_dq=True, want_G='auto')",
        "-- backward",
        "rescale_grads(f32[4, 16], f32[16, 16], f32[1], f32[1])",
        "empty((16, 16), f32, f32[16, 16])",
        "-- second backward",
        "inbatch_bwd(bf16[4, 16], bf16[4, 16], bf16[16, 16], 1, f32[1], True, True)",
        "empty((16, 16), f32, f32[16, 16])",
    ],
    "multi_train_fp32wire_noG": [
        "empty((4, 16), bf16, f32[4, 16])",
        "packed_rows(8, 16)",
        "empty((16, 16), bf16, f32[8, 16])",
        "pack_ctx(f32[8, 16], u8[8], bf16[16, 16])",
        "empty((16, 16), bf16, f32[8, 16])",
        "train_step_packed_f32(f32[4, 16], bf16[16, 16], bf16[4, 16], 1, 0, 8, i64[4], 1, 0.25, 0.25, f32[1], f32, defer_dq=True, want_G='auto')",
        "-- backward",
        "rescale_grads((f32[4, 16], f32[2, 4, 16]), f32[16, 16], f32[1], f32[1])",
        "empty((16, 16), f32, f32[16, 16])",
        "-- second backward",
        "empty((16,), u8, bf16[16, 16])",
        "unpack_mask(bf16[16, 16], 1, 8, u8[16])",
        "inbatch_fwd(bf16[4, 16], bf16[16, 16], i64[4], 0, u8[16], 1, 0.25)",
        "inbatch_bwd(bf16[4, 16], bf16[4, 16], bf16[16, 16], 1, f32[1], True, True)",
        "empty((16, 16), f32, f32[16, 16])",
    ],
    "multi_train_fp32wire_noG_overlap": [
        "packed_rows(8, 16)",
        "empty((16, 16), bf16, f32[8, 16])",
        "pack_ctx(f32[8, 16], u8[8], bf16[16, 16])",
        "empty((16, 16), bf16, f32[8, 16])",
        "empty((4, 16), bf16, f32[4, 16])",
        "packed_rows(8, 16)",
        "train_step_packed_f32(f32[4, 16], bf16[16, 16], bf16[4, 16], 1, 0, 8, i64[4], 1, 0.25, 0.25, f32[1], f32, defer_dq=True, want_G='auto')",
        "-- backward",
        "rescale_grads(f32[4, 16], f32[16, 16], f32[1], f32[1])",
        "empty((16, 16), f32, f32[16, 16])",
        "-- second backward",
        "empty((16,), u8, bf16[16, 16])",
        "unpack_mask(bf16[16, 16], 1, 8, u8[16])",
        "inbatch_fwd(bf16[4, 16], bf16[16, 16], i64[4], 0, u8[16], 1, 0.25)",
        "inbatch_bwd(bf16[4, 16], bf16[4, 16], bf16[16, 16], 1, f32[1], True, True)",
        "empty((16, 16), f32, f32[16, 16])",
    ],
    "multi_train_bf16wire_G": [
        "empty((4, 16), bf16, f32[4, 16])",
        "packed_rows(8, 16)",
        "empty((16, 16), bf16, f32[8, 16])",
        "pack_ctx(f32[8, 16], u8[8], bf16[16, 16])",
        "empty((16, 16), bf16, f32[8, 16])",
        "train_step_packed_f32(f32[4, 16], bf16[16, 16], bf16[4, 16], 1, 0, 8, i64[4], 1, 0.25, 0.25, f32[1], bf16, defer_dq=True, want_G='auto')",
        "-- backward",
        "rescale_grads(f32[4, 16], bf16[16, 16], f32[1], f32[1])",
        "empty((16, 16), bf16, bf16[16, 16])",
        "empty((8, 16), f32, bf16[16, 16])",
        "widen(bf16[16, 16], f32[8, 16])",
        "-- second backward",
        "inbatch_bwd(bf16[4, 16], bf16[4, 16], bf16[16, 16], 1, f32[1], True, True)",
        "empty((16, 16), bf16, f32[16, 16])",
        "empty((8, 16), f32, bf16[16, 16])",
        "widen(bf16[16, 16], f32[8, 16])",
    ],
    "multi_train_bf16wire_noG_overlap": [
        "packed_rows(8, 16)",
        "empty((16, 16), bf16, f32[8, 16])",
        "pack_ctx(f32[8, 16], u8[8], bf16[16, 16])",
        "empty((16, 16), bf16, f32[8, 16])",
        "empty((4, 16), bf16, f32[4, 16])",
        "packed_rows(8, 16)",
        "train_step_packed_f32(f32[4, 16], bf16[16, 16], bf16[4, 16], 1, 0, 8, i64[4], 1, 0.25, 0.25, f32[1], bf16, defer_dq=True, want_G='auto')",
        "-- backward",
        "rescale_grads(f32[4, 16], bf16[16, 16], f32[1], f32[1])",
        "empty((16, 16), bf16, bf16[16, 16])",
        "empty((8, 16), f32, bf16[16, 16])",
        "widen(bf16[16, 16], f32[8, 16])",
        "-- second backward",
        "empty((16,), u8, bf16[16, 16])",
        "unpack_mask(bf16[16, 16], 1, 8, u8[16])",
        "inbatch_fwd(bf16[4, 16], bf16[16, 16], i64[4], 0, u8[16], 1, 0.25)",
        "inbatch_bwd(bf16[4, 16], bf16[4, 16], bf16[16, 16], 1, f32[1], True, True)",
        "empty((16, 16), bf16, f32[16, 16])",
        "empty((8, 16), f32, bf16[16, 16])",
        "widen(bf16[16, 16], f32[8, 16])",
    ],
    "multi_train_bf16wire_fallback_noG": [
        "empty((4, 16), bf16, f32[4, 16])",
        "packed_rows(8, 16)",
        "empty((16, 16), bf16, f32[8, 16])",
        "pack_ctx(f32[8, 16], u8[8], bf16[16, 16])",
        "empty((16, 16), bf16, f32[8, 16])",
        "train_step_packed_f32(f32[4, 16], bf16[16, 16], bf16[4, 16], 1, 0, 8, i64[4], 1, 0.25, 0.25, f32[1], bf16, defer_dq=True, want_G='auto')",
        "train_step_packed_f32(f32[4, 16], bf16[16, 16], bf16[4, 16], 1, 0, 8, i64[4], 1, 0.25, 0.25, f32[1], f32, defer_dq=True, want_G='auto')",
        "-- backward",
        "rescale_grads(f32[4, 16], f32[16, 16], f32[1], f32[1])",
        "empty((16, 16), bf16, f32[16, 16])",
        "empty((8, 16), f32, bf16[16, 16])",
        "widen(bf16[16, 16], f32[8, 16])",
        "-- second backward",
        "empty((16,), u8, bf16[16, 16])",
        "unpack_mask(bf16[16, 16], 1, 8, u8[16])",
        "inbatch_fwd(bf16[4, 16], bf16[16, 16], i64[4], 0, u8[16], 1, 0.25)",
        "inbatch_bwd(bf16[4, 16], bf16[4, 16], bf16[16, 16], 1, f32[1], True, True)",
        "empty((16, 16), bf16, f32[16, 16])",
        "empty((8, 16), f32, bf16[16, 16])",
        "widen(bf16[16, 16], f32[8, 16])",
    ],
    "multi_train_bf16wire_fallback_G_overlap": [
        "packed_rows(8, 16)",
        "empty((16, 16), bf16, f32[8, 16])",
        "pack_ctx(f32[8, 16], u8[8], bf16[16, 16])",
        "empty((16, 16), bf16, f32[8, 16])",
        "empty((4, 16), bf16, f32[4, 16])",
        "packed_rows(8, 16)",
        "train_step_packed_f32(f32[4, 16], bf16[16, 16], bf16[4, 16], 1, 0, 8, i64[4], 1, 0.25, 0.25, f32[1], bf16, defer_dq=True, want_G='auto')",
        "train_step_packed_f32(f32[4, 16], bf16[16, 16], bf16[4, 16], 1, 0, 8, i64[4], 1, 0.25, 0.25, f32[1], f32, defer_dq=True, want_G='auto')",
        "-- backward",
        "rescale_grads(f32[4, 16], f32[16, 16], f32[1], f32[1])",
        "empty((16, 16), bf16, f32[16, 16])",
        "empty((8, 16), f32, bf16[16, 16])",
        "widen(bf16[16, 16], f32[8, 16])",
        "-- second backward",
        "inbatch_bwd(bf16[4, 16], bf16[4, 16], bf16[16, 16], 1, f32[1], True, True)",
        "empty((16, 16), bf16, f32[16, 16])",
        "empty((8, 16), f32, bf16[16, 16])",
        "widen(bf16[16, 16], f32[8, 16])",
    ],
    "multi_bf16_inputs": [
        "empty((4, 16), bf16, bf16[4, 16])",
        "packed_rows(8, 16)",
        "empty((16, 16), bf16, bf16[8, 16])",
        "pack_ctx(bf16[8, 16], u8[8], bf16[16, 16])",
        "empty((16, 16), bf16, bf16[8, 16])",
        "empty((16,), u8, bf16[8, 16])",
        "unpack_mask(bf16[16, 16], 1, 8, u8[16])",
        "cast_bf16(bf16[4, 16], bf16[4, 16])",
        "inbatch_fwd(bf16[4, 16], bf16[16, 16], i64[4], 0, u8[16], 1, 0.25)",
        "-- backward",
        "inbatch_bwd(bf16[4, 16], bf16[4, 16], bf16[16, 16], 1, f32[1], True, True)",
        "empty((16, 16), f32, f32[16, 16])",
        "-- second backward",
        "inbatch_bwd(bf16[4, 16], bf16[4, 16], bf16[16, 16], 1, f32[1], True, True)",
        "empty((16, 16), f32, f32[16, 16])",
    ],
    "multi_no_grad": [
        "empty((4, 16), bf16, f32[4, 16])",
        "packed_rows(8, 16)",
        "empty((16, 16), bf16, f32[8, 16])",
        "pack_ctx(f32[8, 16], u8[8], bf16[16, 16])",
        "empty((16, 16), bf16, f32[8, 16])",
        "empty((16,), u8, f32[8, 16])",
        "unpack_mask(bf16[16, 16], 1, 8, u8[16])",
        "inbatch_fwd_f32(f32[4, 16], None, bf16[4, 16], bf16[16, 16], i64[4], 0, u8[16], 1, 0.25)",
    ],
    "multi_no_grad_overlap": [
        "packed_rows(8, 16)",
        "empty((16, 16), bf16, f32[8, 16])",
        "pack_ctx(f32[8, 16], u8[8], bf16[16, 16])",
        "empty((16, 16), bf16, f32[8, 16])",
        "empty((4, 16), bf16, f32[4, 16])",
        "packed_rows(8, 16)",
        "empty((16,), u8, f32[8, 16])",
        "unpack_mask(bf16[16, 16], 1, 8, u8[16])",
        "inbatch_fwd_f32(f32[4, 16], None, bf16[4, 16], bf16[16, 16], i64[4], 0, u8[16], 1, 0.25)",
    ],
}


@pytest.fixture(scope="module")
def one_rank_world(tmp_path_factory):
    store = dist.FileStore(str(tmp_path_factory.mktemp("pg") / "store"), 1)
    dist.init_process_group("gloo", store=store, rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def _inputs(B, K, d=16):
    q, c, y, m = O.synth_embeddings(7, B, K, d, "U", True)
    return q, c, y, m, O.training_step_global(q, c, y, m, T)


_REF = {}  # (B, K) -> inputs and the oracle's answer, computed once


def _check(loss, tq, tc, go, ref):
    assert abs(loss.item() - ref["loss"]) <= 1e-3 * max(1.0, abs(ref["loss"]))
    # G travels as bf16 (2^-9 relative rounding per element), hence the 1e-2-of-max bar on gradients (tests/test_dist_gloo.py)
    dq, dc = tq.grad.float().numpy() / go, tc.grad.float().numpy() / go
    assert np.abs(dq - ref["dQ"]).max() <= 1e-2 * np.abs(ref["dQ"]).max()
    assert np.abs(dc - ref["dC"]).max() <= 1e-2 * np.abs(ref["dC"]).max()


def run_case(name, go, monkeypatch):
    """Forward, backward(grad_output = go) with the graph retained, a second backward; returns the call log."""
    case = CASES[name]
    B, K = case.get("B", 4), 2
    if (B, K) not in _REF:
        _REF[(B, K)] = _inputs(B, K)
    q, c, y, m, ref = _REF[(B, K)]
    for k in ("DPRHOT_FP32_G", "DPRHOT_DC_WIRE", "DPRHOT_FORCE_DIST", "DPRHOT_PATH_COLLECTIVES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    if case.get("multi"):
        monkeypatch.setattr(D, "force_dist", lambda: True)
    hotpath._ExpectedGradScale._cur.clear()
    inner = OracleKernels()
    for k, v in case.get("kn", {}).items():
        setattr(inner, k, v)
    kn = Recorder(inner)
    dtype = case.get("dtype", torch.float32)
    grads = case.get("grads", True)
    tq = torch.from_numpy(q).to(dtype).requires_grad_(grads)
    tc = torch.from_numpy(c).to(dtype).requires_grad_(grads)
    ty, tm = torch.from_numpy(y), torch.from_numpy(m)
    if case.get("overlap"):
        c1 = tc * 1.0 if grads else tc
        c2, pending = defer_context_grad(c1)
        g = ContextGather(c2, tm, None, kn)
        loss = inbatch_contrastive_loss(tq, c2, ty, tm, T, None, kn, g, pending)
    else:
        loss = inbatch_contrastive_loss(tq, tc, ty, tm, T, None, kn)
    if not grads:
        assert abs(loss.item() - ref["loss"]) <= 1e-3 * max(1.0, abs(ref["loss"]))
        return kn.log
    kn.log.append("-- backward")
    (loss * go).backward(retain_graph=True)
    _check(loss, tq, tc, go, ref)
    if name in PRESCALED:
        # the gradients were computed in forward; backward hands those very tensors to autograd and forgets them, so AccumulateGrad
        # takes them as .grad instead of cloning them
        h = kn.handed
        assert tq.grad.data_ptr() == h["dq_ptr"]
        if not case.get("multi"):
            assert tc.grad.data_ptr() == h["dc_ptr"]
        gc.collect()
        dq_alive = h["dq"]()
        assert dq_alive is None or dq_alive is tq.grad
        if case.get("multi"):
            assert h["dc"]() is None  # the partials went into the reduce-scatter; nobody holds them afterwards
        del dq_alive
    tq.grad = tc.grad = None
    kn.log.append("-- second backward")
    (loss * go).backward()
    _check(loss, tq, tc, go, ref)
    return kn.log


@pytest.mark.parametrize("go", [1.0, 3.0])
@pytest.mark.parametrize("name", [n for n in CASES if not CASES[n].get("multi")])
def test_single_rank_route(name, go, monkeypatch):
    assert run_case(name, go, monkeypatch) == EXPECTED[name]


@pytest.mark.parametrize("go", [1.0, 3.0])
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n].get("multi")])
def test_multi_rank_route_on_a_one_rank_world(name, go, monkeypatch, one_rank_world):
    assert run_case(name, go, monkeypatch) == EXPECTED[name]
