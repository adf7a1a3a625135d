"""The in-batch contrastive step of dpr-scale on MI355X: host side of the operator boundary.

Replaces, for one rank, dpr_scale/task/dpr_task.py:163-212 (gather -> sim_score -> /T -> CrossEntropyLoss) and
its autograd backward by:  fp32->bf16 cast | RCCL all-gather of context rows | HIP sim + softmax-CE + dScores |
HIP dQ / dC GEMMs | RCCL reduce-scatter of dC.  All device work goes through the C ABI of libdprhot.so
(include/dprhot.h); this file only moves pointers.  There is NO CPU path here: CPU tensors raise.

`kernels` arguments exist so that the CPU test-suite can exercise the distributed orchestration (gather
layout, label offsets, reduce-scatter, loss all-reduce) on gloo with a stand-in; the default -- and the only
thing the product ever passes -- is the HIP library.  A kernel set offers every entry point HipKernels offers: nothing
below asks what it was given, so a stand-in takes the routes production takes.
"""
import ctypes
import os

import torch

from . import dist as D

_BF16 = torch.bfloat16
_KIND = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}  # storage kinds of include/dprhot.h


class _ExpectedGradScale:
    """Per device: the DEVICE scalar the next training step should scale its gradients by -- the grad_output the previous backward
    saw (AMP's loss scale; 1 for a plain backward()).  Every backward publishes a FRESH one-float tensor (written once by
    dprhot_rescale_grads, never modified afterwards), so a step that read an older one can still compare against it.

    Lifetime under graph capture (the same rule as g_scale in csrc/opx.cpp).  A captured graph bakes in the address of the scalar its
    forward read, so an entry handed out while the current stream is capturing is kept for the life of the process (_kept): replacing
    it later never frees memory a replay reads.  Eager steps and captured steps keep separate chains: a scalar published under capture
    lives in the graph's pool and holds nothing until the first replay, so only steps of THAT capture see it (_cap, by capture id).
    Replays read the kept eager scalar as `used` for ever; dprhot_rescale_grads makes the gradients right whatever it holds.
    Two things that look like leaks and are not: _cap keeps the last scalar of a finished capture (a block of that graph's pool, even
    after the graph is gone) until the next capture at the same site overwrites it -- nobody reads it, its id matches no other capture;
    and a capture whose id query fails gets the id -1 (_lib.capture_id), so two such captures would share one chain: the second would
    then read the first one's last scalar as `used`, which the rescale makes right like any other value."""

    _cur = {}
    _cap = {}   # (dev, site) -> (capture id, the scalar the capture's last backward wrote)
    _kept = {}  # data_ptr -> tensor: eager entries whose address a captured graph holds

    @staticmethod
    def _capture_id(dev):
        if torch.device(dev).type != "cuda" or not torch.cuda.is_current_stream_capturing():
            return 0
        from . import _lib
        return _lib.capture_id(torch.cuda.current_stream(dev).cuda_stream)

    @classmethod
    def get(cls, dev, site=None):
        """`site`: what tells the operator's call sites of one model apart -- the step's shape (B, Nc, d).  CITADEL's router loss and the
        main loss receive different constant upstream factors in the same step; one shared prediction made each of them mispredict
        the other every step (and pay the full rescale pass)."""
        k = (dev, site)
        cid = cls._capture_id(dev)
        if cid:
            e = cls._cap.get(k)
            if e is not None and e[0] == cid:
                return e[1]
        t = cls._cur.get(k)
        if t is None:
            t = torch.ones(1, dtype=torch.float32, device=dev)
            if cid:  # no eager step came first: the fill is part of the graph, the scalar belongs to this capture
                cls._cap[k] = (cid, t)
                return t
            cls._cur[k] = t
        if cid:
            cls._kept[t.data_ptr()] = t
        return t

    @classmethod
    def publish(cls, dev, t, site=None):
        cid = cls._capture_id(dev)
        if cid:
            cls._cap[(dev, site)] = (cid, t)
        else:
            cls._cur[(dev, site)] = t


def _fp32_g_mode():
    """DPRHOT_FP32_G=1: debug mode of SURVEY.md section 8 c5 -- dScores no longer travel as ONE bf16 value (2^-9 relative
    rounding, the source of the ~2e-3 gradient deviation) but as a bf16 pair hi + lo (G = hi + lo to 2^-17), and each
    backward GEMM runs twice on the same MFMA kernels; gradients then agree with the fp32 reference to <= 1e-3.  Single
    rank only; costs a second pass over the logits and two more GEMM launches."""
    return os.environ.get("DPRHOT_FP32_G") == "1"


def _dc_wire_dtype(group=None):
    """The format the dC partials travel in.  DPRHOT_DC_WIRE=bf16: the reduce-scatter ships bf16 (10.5 MiB per rank at cfg3 instead of
    21 MiB; one more rounding per partial); =fp32: never.  Unset / auto: what dist.choose_path_collectives
    MEASURED for this group when it was given both wires (DenseRetrieverTask.on_pretrain_routine_start; bf16 only where it won by 5 %),
    fp32 where no probe ran."""
    env = os.environ.get("DPRHOT_DC_WIRE", "auto")
    if env == "bf16":
        return _BF16
    if env == "fp32" or group is False:
        return torch.float32
    return D.path_wire(group, torch.float32)


_ZERO_ROW = {}  # device -> one fp32 zero, never written: `expand`ed it is a gradient of zeros that costs no launch


def _zeros_view(shape, device):
    z = _ZERO_ROW.get(device)
    if z is None:
        z = _ZERO_ROW[device] = torch.zeros((1, 1), dtype=torch.float32, device=device)
    return z.expand(*shape)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_RH_DTYPE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}  # the dtype codes of dprhot_router_head_*
_IVF_ROUND = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # DPRHOT_IVF_FP32 / _BF16 / _FP16 of dprhot_ivf_gather
TOPK_KWIDE = 4096  # largest k of the streaming top-k kernel (dprhot_topk_update: 8192 sort slots in 96 KB of LDS); beyond: the HBM-resident selection


class HipKernels:
    """Thin, allocation-aware wrapper over libdprhot.  Every tensor must live on a HIP device."""

    name = "hip"

    def __init__(self):
        from . import _lib  # raises ImportError if libdprhot.so is missing -- loudly, by design

        self._lib = _lib
        self.lib = _lib.lib
        self._ws = {}
        self._ws_kept = {}
        self._nslabs = {}
        self._wg = {}

    # -- plumbing --------------------------------------------------------------------------------------
    @staticmethod
    def _require_gpu(*ts):
        for t in ts:
            if t is not None and not t.is_cuda:
                raise RuntimeError(
                    "dpr_scale_amd hot path needs HIP device tensors (got a CPU tensor); there is no CPU fallback")

    @staticmethod
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _workspace(self, device, nbytes):
        """The cached step workspace, one per (device, stream) as in csrc/opx.cpp: steps on two streams never share one.  A buffer handed
        out while the stream is capturing is kept for the life of the process (_ws_kept): the graph bakes its address in, and a larger
        shape that replaces the entry later must not free what a replay still writes into."""
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            self._ws[key] = ws
        if torch.cuda.is_current_stream_capturing():
            self._ws_kept[ws.data_ptr()] = ws
        return ws

    def empty(self, shape, dtype, like):
        return torch.empty(shape, dtype=dtype, device=like.device)

    def _wants_g(self, B, Nc, d):
        key = (B, Nc, d, self._lib.options_epoch())
        w = self._wg.get(key)
        if w is None:
            w = self._wg[key] = self._lib.step_wants_g(B, Nc, d)
        return w

    # -- ops -------------------------------------------------------------------------------------------
    def cast_bf16(self, src, dst):
        """dst (bf16, contiguous, may be a row-slice of the gather buffer) <- src (fp32 or bf16)."""
        self._require_gpu(src, dst)
        src = src.detach()
        if src.dtype == _BF16:
            dst.copy_(src)
            return dst
        src = src.contiguous().float()
        n = src.numel()
        assert dst.is_contiguous() and dst.numel() == n and n % 8 == 0
        self._lib.check(self.lib.dprhot_cast_bf16(_ptr(src), _ptr(dst), n, self._stream()), "dprhot_cast_bf16")
        return dst

    def prep(self, q, Qb, c, Cdst):
        """Both producer-side casts in one launch (fp32 inputs); other dtypes take the per-tensor path."""
        self._require_gpu(q, Qb, c, Cdst)
        if q.dtype != torch.float32 or c.dtype != torch.float32:
            self.cast_bf16(q, Qb)
            self.cast_bf16(c, Cdst)
            return
        q = q.detach().contiguous()
        c = c.detach().contiguous()
        assert Qb.is_contiguous() and Cdst.is_contiguous() and Qb.numel() == q.numel() and Cdst.numel() == c.numel()
        self._lib.check(self.lib.dprhot_prep(_ptr(q), q.numel(), _ptr(Qb), _ptr(c), c.numel(), _ptr(Cdst), self._stream()),
                        "dprhot_prep")

    def packed_rows(self, n_ctx, d):
        return self._lib.packed_rows(n_ctx, d)

    def pack_ctx(self, c, m8, send):
        """send [rows_c, d] bf16 <- context rows (fp32 -> bf16) followed by the mask bytes (one all-gather moves both)."""
        self._require_gpu(c, m8, send)
        c = c.detach().float().contiguous()
        n_ctx, d = c.shape
        assert send.is_contiguous() and send.shape == (self.packed_rows(n_ctx, d), d)
        self._lib.check(self.lib.dprhot_pack_ctx(_ptr(c), _ptr(m8.contiguous()), n_ctx, d, _ptr(send), self._stream()),
                        "dprhot_pack_ctx")

    def unpack_mask(self, gathered, W, n_ctx, colmask):
        self._require_gpu(gathered, colmask)
        d = gathered.shape[1]
        assert colmask.numel() == W * self.packed_rows(n_ctx, d)
        self._lib.check(self.lib.dprhot_unpack_mask(_ptr(gathered), W, n_ctx, d, _ptr(colmask), self._stream()),
                        "dprhot_unpack_mask")

    def _step_outputs(self, B, Nc, d, dev, want_G, want_S=False, grads=False, loss_len=1, dc_dtype=torch.float32, defer_dq=False):
        """What the six step entry points allocate, in the order they always have, and the workspace -> (row_loss, row_lse, loss, G, S,
        dQ, dC, part, ws).  grads False, a forward: G by truth value, S when want_S.  grads True, a step: G as want_G says, dQ, dC in
        dc_dtype, the split-K slabs (`part`) when defer_dq and the plan leaves some.  (Plain addresses go on: _lib's argtypes make pointers.)"""
        f32 = torch.float32
        row_loss = torch.empty(B, dtype=f32, device=dev)
        row_lse = torch.empty(B, dtype=f32, device=dev)
        loss = torch.empty(loss_len, dtype=f32, device=dev)
        S = dQ = dC = part = None
        if grads:
            # the dScores buffer: True -> always (the plan then materialises G); "auto" -> only where the shape's plan needs one
            # (dprhot_step_wants_g; elsewhere the step never writes the dScores: one launch less at cfg3 per rank); False -> none
            G = torch.empty((B, Nc), dtype=_BF16, device=dev) if want_G is True or (want_G == "auto" and self._wants_g(B, Nc, d)) else None
            dQ = torch.empty((B, d), dtype=f32, device=dev)
            dC = torch.empty((Nc, d), dtype=dc_dtype, device=dev)
            if defer_dq:  # caller-owned buffer for the split-K partial sums of dQ, where this shape's plan leaves any
                key = (B, Nc, d, self._lib.options_epoch())  # the plan depends on process-wide options (dprhot_set_option)
                n = self._nslabs.get(key)
                if n is None:
                    n = self._nslabs[key] = self._lib.train_dq_slabs(B, Nc, d)
                if n > 0:
                    part = torch.empty((n, B, d), dtype=f32, device=dev)
        else:
            G = torch.empty((B, Nc), dtype=_BF16, device=dev) if want_G else None
            S = torch.empty((B, Nc), dtype=f32, device=dev) if want_S else None
        return row_loss, row_lse, loss, G, S, dQ, dC, part, self._workspace(dev, self._lib.workspace_bytes(B, Nc, d))

    def inbatch_fwd(self, Qb, Cb, y, y_offset, colmask, inv_T, grad_scale, want_logits=False, want_G=True):
        self._require_gpu(Qb, Cb, y, colmask)
        (B, d), Nc = Qb.shape, Cb.shape[0]
        row_loss, row_lse, loss_sum, G, S, _, _, _, ws = self._step_outputs(B, Nc, d, Qb.device, want_G, want_S=want_logits)
        self._lib.check(self.lib.dprhot_inbatch_fwd(
            Qb.data_ptr(), B, Cb.data_ptr(), Nc, d, _ptr(y), int(y_offset), _ptr(colmask), float(inv_T), float(grad_scale), _ptr(S), row_loss.data_ptr(),
            row_lse.data_ptr(), loss_sum.data_ptr(), _ptr(G), ws.data_ptr(), ws.numel(), self._stream()), "dprhot_inbatch_fwd")
        return row_loss, row_lse, loss_sum, G, S

    def inbatch_fwd_f32(self, q, c, Qb, Cb, y, y_offset, colmask, inv_T, grad_scale, want_logits=False, want_G=True):
        """Forward straight from the fp32 encoder outputs: q [B,d] fp32; c [Nc,d] fp32 or None (Cb already holds
        the gathered bf16 rows).  Fills Qb (and Cb when c is given) with the bf16 images the backward reads."""
        self._require_gpu(q, c, Qb, Cb, y, colmask)
        (B, d), Nc = Qb.shape, Cb.shape[0]
        q = q.detach().contiguous()
        c = c.detach().contiguous() if c is not None else None
        assert q.dtype == torch.float32 and (c is None or (c.dtype == torch.float32 and c.shape[0] == Nc))
        row_loss, row_lse, loss_sum, G, S, _, _, _, ws = self._step_outputs(B, Nc, d, Qb.device, want_G, want_S=want_logits)
        self._lib.check(self.lib.dprhot_inbatch_fwd_f32(
            q.data_ptr(), _ptr(c), Qb.data_ptr(), Cb.data_ptr(), B, Nc, d, _ptr(y), int(y_offset), _ptr(colmask), float(inv_T), float(grad_scale), _ptr(S),
            row_loss.data_ptr(), row_lse.data_ptr(), loss_sum.data_ptr(), _ptr(G), ws.data_ptr(), ws.numel(), self._stream()), "dprhot_inbatch_fwd_f32")
        return row_loss, row_lse, loss_sum, G, S

    def inbatch_step_f32(self, q, c, Qb, Cb, y, y_offset, colmask, inv_T, grad_scale, want_G=True):
        """Forward AND backward in one library call (dprhot_inbatch_step_f32; two launches at the BASELINE training
        shapes).  Gradients come back for grad_output = 1: returns (row_loss, row_lse, loss_sum, G, dQ, dC_part)."""
        self._require_gpu(q, c, Qb, Cb, y, colmask)
        (B, d), Nc = Qb.shape, Cb.shape[0]
        q = q.detach().contiguous()
        c = c.detach().contiguous() if c is not None else None
        assert q.dtype == torch.float32 and (c is None or (c.dtype == torch.float32 and c.shape[0] == Nc))
        row_loss, row_lse, loss_sum, G, _, dQ, dC, _, ws = self._step_outputs(B, Nc, d, Qb.device, want_G, grads=True)
        self._lib.check(self.lib.dprhot_inbatch_step_f32(
            q.data_ptr(), _ptr(c), Qb.data_ptr(), Cb.data_ptr(), B, Nc, d, _ptr(y), int(y_offset), _ptr(colmask), float(inv_T), float(grad_scale), 1.0,
            None, None, row_loss.data_ptr(), row_lse.data_ptr(), loss_sum.data_ptr(), _ptr(G), dQ.data_ptr(), dC.data_ptr(), ws.data_ptr(), ws.numel(),
            self._stream()), "dprhot_inbatch_step_f32")
        return row_loss, row_lse, loss_sum, G, dQ, dC

    def inbatch_step_packed_f32(self, q, gathered, Qb, W, rank, n_ctx, y, inv_T, grad_scale, want_G=True):
        """World size > 1: everything between the all-gather and the reduce-scatter in one library call.  `gathered` is
        the all-gathered packed buffer; the mask is read from it, and dC_part carries this rank's loss numerator at
        [k * rows_c + n_ctx][0] of every chunk k (see include/dprhot.h).  Returns (row_loss, row_lse, loss_sum, G, dQ,
        dC_part)."""
        self._require_gpu(q, gathered, Qb, y)
        (B, d), Nc = Qb.shape, gathered.shape[0]
        q = q.detach().contiguous()
        assert q.dtype == torch.float32 and gathered.dtype == _BF16 and Nc == W * self.packed_rows(n_ctx, d)
        row_loss, row_lse, loss_sum, G, _, dQ, dC, _, ws = self._step_outputs(B, Nc, d, Qb.device, want_G, grads=True)
        self._lib.check(self.lib.dprhot_inbatch_step_packed_f32(
            q.data_ptr(), gathered.data_ptr(), Qb.data_ptr(), B, int(W), int(rank), int(n_ctx), d, _ptr(y), float(inv_T), float(grad_scale), 1.0, None,
            row_loss.data_ptr(), row_lse.data_ptr(), loss_sum.data_ptr(), _ptr(G), dQ.data_ptr(), dC.data_ptr(), ws.data_ptr(), ws.numel(),
            self._stream()), "dprhot_inbatch_step_packed_f32")
        return row_loss, row_lse, loss_sum, G, dQ, dC

    def train_step_f32(self, q, c, Qb, Cb, y, y_offset, colmask, inv_T, grad_scale, loss_scale, d_scale, dc_dtype=torch.float32,
                       defer_dq=False, want_G=True):
        """The operator's step (dprhot_train_step_f32): forward AND backward in one library call, the loss already multiplied by
        loss_scale, the gradients scaled by the DEVICE scalar d_scale (the grad_output backward() is expected to deliver).
        Returns (row_loss, row_lse, loss_out [2], G, dQ, dC_part); loss_out[0] is the loss.  defer_dq: where the plan splits dQ over
        the contexts, dQ comes back as (dQ buffer, slabs) and rescale_grads() adds the slabs up (one launch less in the step)."""
        self._require_gpu(q, c, Qb, Cb, y, colmask, d_scale)
        (B, d), Nc = Qb.shape, Cb.shape[0]
        q = q.detach().contiguous()
        c = c.detach().contiguous() if c is not None else None
        assert q.dtype == torch.float32 and (c is None or (c.dtype == torch.float32 and c.shape[0] == Nc))
        outs = self._step_outputs(B, Nc, d, Qb.device, want_G, grads=True, loss_len=2, dc_dtype=dc_dtype, defer_dq=defer_dq)
        row_loss, row_lse, loss_out, G, _, dQ, dC, part, ws = outs
        self._lib.check(self.lib.dprhot_train_step_f32(
            q.data_ptr(), _ptr(c), Qb.data_ptr(), Cb.data_ptr(), B, Nc, d, _ptr(y), int(y_offset), _ptr(colmask), float(inv_T), float(grad_scale),
            float(loss_scale), _ptr(d_scale), row_loss.data_ptr(), row_lse.data_ptr(), loss_out.data_ptr(), _ptr(G), dQ.data_ptr(), _ptr(part),
            dC.data_ptr(), _KIND[dc_dtype], ws.data_ptr(), ws.numel(), self._stream()), "dprhot_train_step_f32")
        return row_loss, row_lse, loss_out, G, (dQ if part is None else (dQ, part)), dC

    def train_step_packed_f32(self, q, gathered, Qb, W, rank, n_ctx, y, inv_T, grad_scale, loss_scale, d_scale, dc_dtype=torch.float32,
                              defer_dq=False, want_G=True):
        """World size > 1 (dprhot_train_step_packed_f32): as train_step_f32 on the all-gathered packed buffer."""
        self._require_gpu(q, gathered, Qb, y, d_scale)
        (B, d), Nc = Qb.shape, gathered.shape[0]
        q = q.detach().contiguous()
        assert q.dtype == torch.float32 and gathered.dtype == _BF16 and Nc == W * self.packed_rows(n_ctx, d)
        outs = self._step_outputs(B, Nc, d, Qb.device, want_G, grads=True, loss_len=2, dc_dtype=dc_dtype, defer_dq=defer_dq)
        row_loss, row_lse, loss_out, G, _, dQ, dC, part, ws = outs
        self._lib.check(self.lib.dprhot_train_step_packed_f32(
            q.data_ptr(), gathered.data_ptr(), Qb.data_ptr(), B, int(W), int(rank), int(n_ctx), d, _ptr(y), float(inv_T), float(grad_scale),
            float(loss_scale), _ptr(d_scale), row_loss.data_ptr(), row_lse.data_ptr(), loss_out.data_ptr(), _ptr(G), dQ.data_ptr(), _ptr(part),
            dC.data_ptr(), _KIND[dc_dtype], ws.data_ptr(), ws.numel(), self._stream()), "dprhot_train_step_packed_f32")
        return row_loss, row_lse, loss_out, G, (dQ if part is None else (dQ, part)), dC

    def rescale_grads(self, dQ, dC, go, used):
        """backward() of the operator (dprhot_rescale_grads): the gradients were computed for grad_output = used; multiply by
        go / used only if they differ (decided on the device).  Returns out2: [0] what the gradients are scaled by now, [1] the
        scale the next forward should expect."""
        part = None
        if isinstance(dQ, tuple):  # (dQ buffer, split-K slabs left by a train step with defer_dq): summed here, scaled by go
            dQ, part = dQ
        self._require_gpu(dQ, part, dC, go, used)
        out2 = torch.empty(2, dtype=torch.float32, device=go.device)
        self._lib.check(self.lib.dprhot_rescale_grads(
            _ptr(dQ), dQ.numel() if dQ is not None else 0, _ptr(part), part.shape[0] if part is not None else 0, _ptr(dC),
            dC.numel() if dC is not None else 0, _KIND[dC.dtype] if dC is not None else 2, _ptr(go), _ptr(used), _ptr(out2),
            self._stream()), "dprhot_rescale_grads")
        return out2

    def widen(self, src, dst):
        """dst (fp32, contiguous) <- src (bf16 / fp16 / fp32, contiguous), one pass (dprhot_grad_unpack)."""
        self._require_gpu(src, dst)
        assert src.is_contiguous() and dst.is_contiguous() and dst.dtype == torch.float32 and src.numel() >= dst.numel()
        self._lib.check(self.lib.dprhot_grad_unpack(_ptr(src), _KIND[src.dtype], _ptr(dst), dst.numel(), self._stream()), "dprhot_grad_unpack")
        return dst

    def inbatch_bwd(self, G, Qb, Cb, h_scale, d_scale, need_dq=True, need_dc=True):
        self._require_gpu(G, Qb, Cb, d_scale)
        B, d = Qb.shape
        Nc = Cb.shape[0]
        dev = Qb.device
        dQ = torch.empty((B, d), dtype=torch.float32, device=dev) if need_dq else None
        dC = torch.empty((Nc, d), dtype=torch.float32, device=dev) if need_dc else None
        ws = self._workspace(dev, self._lib.workspace_bytes(B, Nc, d))
        self._lib.check(self.lib.dprhot_inbatch_bwd(
            _ptr(G), _ptr(Qb), _ptr(Cb), B, Nc, d, float(h_scale), _ptr(d_scale), _ptr(dQ), _ptr(dC), _ptr(ws),
            ws.numel(), self._stream()), "dprhot_inbatch_bwd")
        return dQ, dC

    def sim(self, Qb, Cb, colmask=None, inv_T=1.0):
        self._require_gpu(Qb, Cb, colmask)
        B, d = Qb.shape
        Nc = Cb.shape[0]
        S = torch.empty((B, Nc), dtype=torch.float32, device=Qb.device)
        self._lib.check(self.lib.dprhot_sim_fwd(_ptr(Qb), B, _ptr(Cb), Nc, d, _ptr(colmask), float(inv_T), _ptr(S),
                                                self._stream()), "dprhot_sim_fwd")
        return S

    def softmax_ce(self, S, y, y_offset=0, grad_scale=1.0, want_G=False, row_win_start=None, win_len=0):
        self._require_gpu(S, y, row_win_start)
        B, Nc = S.shape
        dev = S.device
        row_loss = torch.empty(B, dtype=torch.float32, device=dev)
        row_lse = torch.empty(B, dtype=torch.float32, device=dev)
        G = torch.empty((B, Nc), dtype=_BF16, device=dev) if want_G else None
        self._lib.check(self.lib.dprhot_softmax_ce_fwd_bwd(
            _ptr(S), B, Nc, _ptr(y), int(y_offset), float(grad_scale), _ptr(row_win_start), int(win_len),
            _ptr(row_loss), _ptr(row_lse), _ptr(G), self._stream()), "dprhot_softmax_ce_fwd_bwd")
        return row_loss, row_lse, G

    def reduce_sum(self, x, scale=1.0):
        self._require_gpu(x)
        out = torch.empty(1, dtype=torch.float32, device=x.device)
        self._lib.check(self.lib.dprhot_reduce_sum(_ptr(x), x.numel(), float(scale), _ptr(out), self._stream()),
                        "dprhot_reduce_sum")
        return out

    def dq(self, G, Cb, h_scale=1.0, d_scale=None):
        B, Nc = G.shape
        d = Cb.shape[1]
        out = torch.empty((B, d), dtype=torch.float32, device=G.device)
        ws = self._workspace(G.device, self._lib.workspace_bytes(B, Nc, d))
        self._lib.check(self.lib.dprhot_dq(_ptr(G), _ptr(Cb), B, Nc, d, float(h_scale), _ptr(d_scale), _ptr(out), _ptr(ws),
                                           ws.numel(), self._stream()), "dprhot_dq")
        return out

    def dc(self, G, Qb, h_scale=1.0, d_scale=None):
        B, Nc = G.shape
        d = Qb.shape[1]
        out = torch.empty((Nc, d), dtype=torch.float32, device=G.device)
        self._lib.check(self.lib.dprhot_dc(_ptr(G), _ptr(Qb), B, Nc, d, float(h_scale), _ptr(d_scale), _ptr(out),
                                           self._stream()), "dprhot_dc")
        return out

    def pairwise_fwd(self, q, c, m8):
        self._require_gpu(q, c, m8)
        B, d = q.shape
        M = c.shape[0] // B
        S = torch.empty((B, M), dtype=torch.float32, device=q.device)
        self._lib.check(self.lib.dprhot_pairwise_fwd(_ptr(q), _ptr(c), _ptr(m8), B, M, d, _ptr(S), self._stream()), "dprhot_pairwise_fwd")
        return S

    def pairwise_bwd(self, g, q, c, need_dq=True, need_dc=True):
        self._require_gpu(g, q, c)
        B, d = q.shape
        M = c.shape[0] // B
        dq = torch.empty_like(q) if need_dq else None
        dc = torch.empty_like(c) if need_dc else None
        self._lib.check(self.lib.dprhot_pairwise_bwd(_ptr(g), _ptr(q), _ptr(c), B, M, d, _ptr(dq), _ptr(dc), self._stream()),
                        "dprhot_pairwise_bwd")
        return dq, dc

    def maxsim_fwd(self, Qb, Cb, qids, cids, qw, cw, KQ, KD, pool, M, m8):
        """Late-interaction expert scores (dprhot_maxsim_fwd).  Qb [Nq, LQ, dp] / Cb [Nc, LD, dp] bf16 with dp % 32 == 0; ids int32 and
        weights fp32 flattened per token slot (or None); pool 0 sum / 1 max; M = 0 in-batch, else contexts per query; m8 uint8 [Nc]
        or None.  Returns (S fp32 [Nq, M or Nc], state): `state` is what maxsim_bwd needs (the argmax tables)."""
        self._require_gpu(Qb, Cb, qids, cids, qw, cw, m8)
        Nq, LQ, dp = Qb.shape
        Nc, LD, _ = Cb.shape
        Ny = M if M else Nc
        ws = torch.empty(self._lib.maxsim_workspace_bytes(Nq, LQ, KQ, Ny, qw is not None), dtype=torch.uint8, device=Qb.device)
        S = torch.empty((Nq, Ny), dtype=torch.float32, device=Qb.device)
        self._lib.check(self.lib.dprhot_maxsim_fwd(_ptr(Qb), _ptr(Cb), Nq, LQ, Nc, LD, dp, _ptr(qids), _ptr(cids), _ptr(qw), _ptr(cw),
                                                   KQ, KD, pool, M, _ptr(m8), _ptr(S), _ptr(ws), ws.numel(), self._stream()),
                        "dprhot_maxsim_fwd")
        return S, ws

    def maxsim_score(self, Qb, Cb, qids, cids, qw, cw, KQ, KD, pool, M, m8):
        """maxsim_fwd's pairwise scores for inference (dprhot_maxsim_score): same operands, M >= 1, one launch, no workspace and no
        state.  Returns S fp32 [Nq, M], bit-equal to maxsim_fwd's."""
        self._require_gpu(Qb, Cb, qids, cids, qw, cw, m8)
        Nq, LQ, dp = Qb.shape
        Nc, LD, _ = Cb.shape
        S = torch.empty((Nq, M), dtype=torch.float32, device=Qb.device)
        self._lib.check(self.lib.dprhot_maxsim_score(_ptr(Qb), _ptr(Cb), Nq, LQ, Nc, LD, dp, _ptr(qids), _ptr(cids), _ptr(qw), _ptr(cw),
                                                     KQ, KD, pool, M, _ptr(m8), _ptr(S), self._stream()),
                        "dprhot_maxsim_score")
        return S

    def maxsim_bwd(self, dS, Qb, Cb, qids, cids, qw, cw, KQ, KD, pool, M, m8, state, need_dq=True, need_dc=True, need_dw=False):
        """Backward of maxsim_fwd from dS [Nq, Ny] fp32: (dq fp32 [Nq, LQ, dp], dc fp32 [Nc, LD, dp], dwq [Nq, LQ, KQ], dwc [Nc, LD, KD]),
        each None unless asked for."""
        self._require_gpu(dS, Qb, Cb)
        Nq, LQ, dp = Qb.shape
        Nc, LD, _ = Cb.shape
        dev = Qb.device
        dq = torch.empty((Nq, LQ, dp), dtype=torch.float32, device=dev) if need_dq else None
        dc = torch.empty((Nc, LD, dp), dtype=torch.float32, device=dev) if need_dc else None
        dwq = torch.empty((Nq, LQ, KQ), dtype=torch.float32, device=dev) if need_dw and qw is not None else None
        dwc = torch.empty((Nc, LD, KD), dtype=torch.float32, device=dev) if need_dw and qw is not None else None
        self._lib.check(self.lib.dprhot_maxsim_bwd(_ptr(dS), _ptr(Qb), _ptr(Cb), Nq, LQ, Nc, LD, dp, _ptr(qids), _ptr(cids), _ptr(qw),
                                                   _ptr(cw), KQ, KD, pool, M, _ptr(m8), _ptr(state), state.numel(), _ptr(dq), _ptr(dc),
                                                   _ptr(dwq), _ptr(dwc), self._stream()),
                        "dprhot_maxsim_bwd")
        return dq, dc, dwq, dwc

    def router_head_fwd(self, logits, m8, k, skip, want_softmax):
        """The encoder head behind the MLM logits (dprhot_router_head_fwd).  logits [B, T1, V] fp32 / bf16 / fp16 with unit column stride
        (any row strides: views pass without a copy), m8 uint8 [B, T1].  Returns (router_repr [B, V], argmax int32 [B, V],
        expert_weights [B, T, k], expert_ids int32 [B, T, k], router_mask [B, V], softmax_sum [B, V], state); the k = 0 / want_softmax =
        False outputs are None.  `state` (the rows' logsumexp) is what router_head_bwd needs."""
        self._require_gpu(logits, m8)
        B, T1, V = logits.shape
        T, dev, dt = T1 - skip, logits.device, logits.dtype
        nbytes = self._lib.router_head_workspace_bytes(B, max(T, 1), V, k, want_softmax)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        repr_ = torch.empty((B, V), dtype=dt, device=dev)
        arg = torch.empty((B, V), dtype=torch.int32, device=dev)
        w = torch.empty((B, T, k), dtype=dt, device=dev) if k else None
        ids = torch.empty((B, T, k), dtype=torch.int32, device=dev) if k else None
        rmask = torch.empty((B, V), dtype=dt, device=dev) if k else None
        ssum = torch.empty((B, V), dtype=dt, device=dev) if want_softmax else None
        self._lib.check(self.lib.dprhot_router_head_fwd(_ptr(logits), _RH_DTYPE[dt], B, T1, V, logits.stride(0), logits.stride(1), _ptr(m8),
                                                        skip, k, int(want_softmax), _ptr(repr_), _ptr(arg), _ptr(w), _ptr(ids), _ptr(rmask),
                                                        _ptr(ssum), _ptr(ws), nbytes, self._stream()), "dprhot_router_head_fwd")
        return repr_, arg, w, ids, rmask, ssum, ws

    def router_head_bwd(self, logits, m8, k, skip, arg, ids, state, g_repr, g_w, g_soft):
        """dlogits [B, T1, V] (contiguous, the logits' dtype) from the fp32 gradients of router_repr / expert_weights / softmax_sum, each
        of which may be None (dprhot_router_head_bwd)."""
        self._require_gpu(logits, m8, g_repr, g_w, g_soft)
        B, T1, V = logits.shape
        dx = torch.empty((B, T1, V), dtype=logits.dtype, device=logits.device)
        self._lib.check(self.lib.dprhot_router_head_bwd(_ptr(logits), _RH_DTYPE[logits.dtype], B, T1, V, logits.stride(0), logits.stride(1),
                                                        _ptr(m8), skip, k, _ptr(arg), _ptr(ids), _ptr(state),
                                                        state.numel() if state is not None else 0, _ptr(g_repr), _ptr(g_w), _ptr(g_soft),
                                                        _ptr(dx), self._stream()), "dprhot_router_head_bwd")
        return dx

    def rank_of_gold(self, S, y, y_offset=0):
        self._require_gpu(S, y)
        rows, cols = S.shape
        out = torch.empty(rows, dtype=torch.int64, device=S.device)
        self._lib.check(self.lib.dprhot_rank_of_gold(_ptr(S), rows, cols, _ptr(y), int(y_offset), _ptr(out), self._stream()),
                        "dprhot_rank_of_gold")
        return out

    def sim_rank(self, Qb, Cb, y, colmask=None, inv_T=1.0, y_offset=0):
        """rank_of_gold of the scores Qb x Cb^T * inv_T (masked columns -inf) without the score matrix at large shapes."""
        self._require_gpu(Qb, Cb, y, colmask)
        B, d = Qb.shape
        Nc = Cb.shape[0]
        rank = torch.empty(B, dtype=torch.int64, device=Qb.device)
        ws = self._workspace(Qb.device, self._lib.workspace_bytes(B, Nc, d))
        self._lib.check(self.lib.dprhot_sim_rank(_ptr(Qb), B, _ptr(Cb), Nc, d, _ptr(y), int(y_offset), _ptr(colmask), float(inv_T),
                                                 _ptr(rank), _ptr(ws), ws.numel(), self._stream()), "dprhot_sim_rank")
        return rank

    def sim_rank_loss(self, Qb, Cb, y, colmask=None, inv_T=1.0, y_offset=0):
        """(rank [B] int64, loss_sum [1]) of the scores Qb x Cb^T * inv_T -- dprhot_sim_rank_loss: one GEMM pass at large shapes."""
        self._require_gpu(Qb, Cb, y, colmask)
        B, d = Qb.shape
        Nc = Cb.shape[0]
        rank = torch.empty(B, dtype=torch.int64, device=Qb.device)
        loss_sum = torch.empty(1, dtype=torch.float32, device=Qb.device)
        ws = self._workspace(Qb.device, self._lib.workspace_bytes(B, Nc, d))
        self._lib.check(self.lib.dprhot_sim_rank_loss(_ptr(Qb), B, _ptr(Cb), Nc, d, _ptr(y), int(y_offset), _ptr(colmask), float(inv_T),
                                                      _ptr(rank), None, None, _ptr(loss_sum), _ptr(ws), ws.numel(), self._stream()),
                        "dprhot_sim_rank_loss")
        return rank, loss_sum

    def topk(self, S, k):
        self._require_gpu(S)
        rows, cols = S.shape
        v = torch.empty((rows, k), dtype=torch.float32, device=S.device)
        i = torch.empty((rows, k), dtype=torch.int64, device=S.device)
        self._lib.check(self.lib.dprhot_topk(_ptr(S), rows, cols, k, _ptr(v), _ptr(i), self._stream()), "dprhot_topk")
        return v, i

    def topk_update(self, S, cols, col_offset, values, indices, first):
        self._require_gpu(S, values, indices)
        rows, k = values.shape
        self._lib.check(self.lib.dprhot_topk_update(_ptr(S), rows, int(cols), S.stride(0), int(col_offset), k, _ptr(values),
                                                    _ptr(indices), int(bool(first)), self._stream()), "dprhot_topk_update")

    def topk_update_wide(self, S, cols, col_offset, values, indices, first, ws):
        """Any k (csrc/wideselect.h): state in HBM.  ws: uint8 workspace of dprhot_topk_wide_workspace_bytes(rows, k) bytes.  No host sync:
        the ABI reserves word 5 of every row's record as an error word ("keeps its old state"), but no such condition is defined (always 0,
        include/dprhot.h) -- CorpusSearch.result() checks the words of the LAST call once instead of syncing after every chunk."""
        self._require_gpu(S, values, indices, ws)
        rows, k = values.shape
        self._lib.check(self.lib.dprhot_topk_update_wide(_ptr(S), rows, int(cols), S.stride(0), int(col_offset), k, _ptr(values), _ptr(indices),
                                                         1 if first else 0, _ptr(ws), ws.numel(), self._stream()), "dprhot_topk_update_wide")

    @staticmethod
    def topk_wide_errors(ws, rows):
        """The error words of the last dprhot_topk_update_wide call on `ws` (one int32 per row; host sync when inspected)."""
        return ws[: rows * 32].view(torch.int32).view(rows, 8)[:, 5]

    def _topk_wide_bytes(self, rows, k):
        n = ctypes.c_size_t(0)
        self._lib.check(self.lib.dprhot_topk_wide_workspace_bytes(int(rows), int(k), ctypes.byref(n)), "dprhot_topk_wide_workspace_bytes")
        return n.value

    def topk_wide_workspace(self, rows, k, like):
        return torch.empty(self._topk_wide_bytes(rows, k), dtype=torch.uint8, device=like.device)

    def _chunk_workspace(self, score_bytes, nq, k, like):
        """The workspace of a chunked search (the chunk driver of csrc/dprhot.hip): one chunk's score buffer, then the HBM-resident
        selection's state when k is beyond the streaming kernel's."""
        wide = self._topk_wide_bytes(nq, k) if k > TOPK_KWIDE else 0
        return torch.empty(score_bytes + wide, dtype=torch.uint8, device=like.device)

    def _topk_tail(self, id_begin, id_end, values, indices, first, chunk, ws):
        """id_begin, id_end, k, chunk, values, indices, first, ws, len, stream: the arguments every chunked search ends with."""
        return (int(id_begin), int(id_end), values.shape[1], int(chunk), _ptr(values), _ptr(indices), int(bool(first)), _ptr(ws), ws.numel(),
                self._stream())

    def search_workspace(self, nq, chunk, like):
        return torch.empty(self._lib.search_workspace_bytes(nq, chunk), dtype=torch.uint8, device=like.device)

    def search(self, Qb, Cb, id_offset, values, indices, first, chunk, ws):
        self._require_gpu(Qb, Cb, values, indices, ws)
        nq, d = Qb.shape
        k = values.shape[1]
        self._lib.check(self.lib.dprhot_search(_ptr(Qb), nq, _ptr(Cb), Cb.shape[0], d, int(id_offset), k, int(chunk),
                                               _ptr(values), _ptr(indices), int(bool(first)), _ptr(ws), ws.numel(),
                                               self._stream()), "dprhot_search")

    # -- inverted-index retrieval (csrc/ivf.h; dpr_scale_amd/ivf.py owns the packing) ---------------------
    def ivf_workspace(self, nq, n_entries, chunk, has_cls, k, like):
        return self._chunk_workspace(self._lib.ivf_workspace_bytes(nq, n_entries, chunk, has_cls), nq, k, like)

    def _ivf_batch(self, qb):
        """ent_vec, ent_q, n_entries, bexp, bexp_off, n_bexp, nq: the query-batch arguments of the four IVF entry points."""
        self._require_gpu(qb.ent_vec, qb.ent_q, qb.bexp, qb.boff)
        return _ptr(qb.ent_vec), _ptr(qb.ent_q), qb.n_entries, _ptr(qb.bexp), _ptr(qb.boff), int(qb.bexp.shape[0]), qb.nq

    @staticmethod
    def _ivf_cls(index, qb):
        """cls_q, cls_doc, dc, cls_rows, corpus_len: what the two IVF searches pass between the query batch and the top-k tail."""
        return _ptr(qb.cls), _ptr(index.cls), index.dc, 0 if index.cls is None else index.cls.shape[0], index.corpus_len

    def ivf_score(self, index, qb, doc_begin, cols, S):
        """Adds the expert part of doc ids doc_begin .. doc_begin + cols into S [nq, >= cols] fp32 (dprhot_ivf_score)."""
        self._require_gpu(index.post_vec, index.post_doc, index.exp_off, S)
        self._lib.check(self.lib.dprhot_ivf_score(_ptr(index.post_vec), _ptr(index.post_doc), _ptr(index.exp_off), index.n_postings,
                                                  index.n_experts, index.dp, *self._ivf_batch(qb), int(doc_begin), int(cols), _ptr(S),
                                                  S.stride(0), self._stream()), "dprhot_ivf_score")

    def ivf_search(self, index, qb, id_begin, id_end, values, indices, first, chunk, ws):
        """Folds doc ids [id_begin, id_end) of a device-resident index into the running top-k (dprhot_ivf_search)."""
        self._require_gpu(index.post_vec, index.post_doc, index.exp_off, index.cls, qb.cls, values, indices, ws)
        self._lib.check(self.lib.dprhot_ivf_search(_ptr(index.post_vec), _ptr(index.post_doc), _ptr(index.exp_off), index.n_postings,
                                                   index.n_experts, index.dp, *self._ivf_batch(qb), *self._ivf_cls(index, qb),
                                                   *self._topk_tail(id_begin, id_end, values, indices, first, chunk, ws)),
                        "dprhot_ivf_search")

    # -- exhaustive ColBERT search (csrc/colbert.h; dpr_scale_amd/colbert.py owns the index) -------------
    def colbert_workspace(self, nq, chunk, k, like):
        return self._chunk_workspace(self._lib.colbert_workspace_bytes(nq, chunk), nq, k, like)

    def colbert_score(self, index, q, pool, doc_begin, cols, S):
        """Writes the scores of doc ids doc_begin .. doc_begin + cols into S [nq, >= cols] fp32 (dprhot_colbert_score); q bf16 [nq, LQ, dp]."""
        self._require_gpu(index.tok, index.doc_blk, q, S)
        nq, LQ, dp = q.shape
        self._lib.check(self.lib.dprhot_colbert_score(_ptr(index.tok), _ptr(index.doc_blk), index.n_blk, index.corpus_len, dp, _ptr(q), nq, LQ,
                                                      int(pool), int(doc_begin), int(cols), _ptr(S), S.stride(0), self._stream()),
                        "dprhot_colbert_score")

    def colbert_search(self, index, q, pool, id_begin, id_end, values, indices, first, chunk, ws):
        """Folds doc ids [id_begin, id_end) of a device-resident token index into the running top-k (dprhot_colbert_search)."""
        self._require_gpu(index.tok, index.doc_blk, q, values, indices, ws)
        nq, LQ, dp = q.shape
        self._lib.check(self.lib.dprhot_colbert_search(_ptr(index.tok), _ptr(index.doc_blk), index.n_blk, index.corpus_len, dp, _ptr(q), nq, LQ,
                                                       int(pool), *self._topk_tail(id_begin, id_end, values, indices, first, chunk, ws)),
                        "dprhot_colbert_search")

    # -- MaxSim over candidate lists (csrc/colbert_cand.h) ---------------------------------------------
    def colbert_cand_workspace(self, nq, chunk, k, like):
        return self._chunk_workspace(self._lib.colbert_cand_workspace_bytes(nq, chunk), nq, k, like)

    def _colbert_cand_head(self, index, q, pool, cand_off, cand_doc):
        """tok .. n_cand: the arguments both candidate entry points begin with; cand_off int64 [nq + 1], cand_doc int32 [n_cand]."""
        self._require_gpu(index.tok, index.doc_blk, q, cand_off, cand_doc)
        nq, LQ, dp = q.shape
        assert cand_off.dtype == torch.int64 and cand_doc.dtype == torch.int32 and cand_off.shape == (nq + 1,)
        assert cand_off.is_contiguous() and cand_doc.is_contiguous()
        return (_ptr(index.tok), _ptr(index.doc_blk), index.n_blk, index.corpus_len, dp, _ptr(q), nq, LQ, int(pool), _ptr(cand_off),
                _ptr(cand_doc), int(cand_doc.shape[0]))

    def colbert_cand_score(self, index, q, pool, cand_off, cand_doc, pos_begin, cols, S):
        """Writes the scores of candidate positions pos_begin .. pos_begin + cols of every query's list into S [nq, >= cols] fp32; a
        position without a candidate is NaN (dprhot_colbert_cand_score)."""
        self._require_gpu(S)
        self._lib.check(self.lib.dprhot_colbert_cand_score(*self._colbert_cand_head(index, q, pool, cand_off, cand_doc), int(pos_begin),
                                                           int(cols), _ptr(S), S.stride(0), self._stream()), "dprhot_colbert_cand_score")

    def colbert_cand_search(self, index, q, pool, cand_off, cand_doc, max_count, values, indices, chunk, ws):
        """The top-k of every query's candidate list, as doc ids (dprhot_colbert_cand_search); always from an empty state."""
        self._require_gpu(values, indices, ws)
        self._lib.check(self.lib.dprhot_colbert_cand_search(*self._colbert_cand_head(index, q, pool, cand_off, cand_doc), int(max_count),
                                                            values.shape[1], int(chunk), _ptr(values), _ptr(indices), _ptr(ws), ws.numel(),
                                                            self._stream()), "dprhot_colbert_cand_search")

    # -- the candidate lists themselves (csrc/colbert_union.h) ------------------------------------------
    def colbert_union_workspace(self, nq, corpus_len, like):
        """The membership state of `nq` queries over `corpus_len` passages: the cached workspace of the current stream (at least
        dprhot_colbert_union_workspace_bytes), written by colbert_union_count and read by the colbert_union_fill behind it."""
        return self._workspace(like.device, self._lib.colbert_union_workspace_bytes(nq, corpus_len))

    def colbert_union_count(self, index, cids, qb, cand_off, totals, ws):
        """Marks every query's candidate set in `ws` and writes cand_off int64 [nq + 1] and totals int64 [2] = (n_cand, the longest
        list) (dprhot_colbert_union_count); cids int64 [nq, LQ, nprobe], qb bf16 [nq, LQ, dp]."""
        self._require_gpu(cids, qb, index.cen_off, index.cen_doc, cand_off, totals, ws)
        nq, LQ, dp = qb.shape
        assert cids.dtype == torch.int64 and cids.is_contiguous() and cids.shape[:2] == (nq, LQ) and qb.dtype == _BF16 and qb.is_contiguous()
        assert index.cen_off.dtype == torch.int64 and index.cen_doc.dtype == torch.int32
        assert cand_off.dtype == torch.int64 and cand_off.shape == (nq + 1,) and totals.dtype == torch.int64 and totals.shape == (2,)
        assert cand_off.is_contiguous() and totals.is_contiguous()
        n_list = int(index.cen_doc.shape[0])
        self._lib.check(self.lib.dprhot_colbert_union_count(_ptr(cids), _ptr(qb), dp, nq, LQ, int(cids.shape[2]), int(index.cen_off.shape[0]) - 1,
                                                            _ptr(index.cen_off), _ptr(index.cen_doc) if n_list else None, n_list,
                                                            index.corpus_len, _ptr(cand_off), _ptr(totals), _ptr(ws), ws.numel(), self._stream()),
                        "dprhot_colbert_union_count")

    def colbert_union_fill(self, index, cand_off, cand_doc, ws):
        """Writes every query's sorted candidate list at cand_doc[cand_off[n] ..] from the state colbert_union_count left in `ws`; the
        length of cand_doc int32 is a capacity, nothing behind it is written (dprhot_colbert_union_fill)."""
        self._require_gpu(cand_off, cand_doc, ws)
        assert cand_off.dtype == torch.int64 and cand_doc.dtype == torch.int32 and cand_off.is_contiguous() and cand_doc.is_contiguous()
        n_cand = int(cand_doc.shape[0])
        self._lib.check(self.lib.dprhot_colbert_union_fill(int(cand_off.shape[0]) - 1, index.corpus_len, _ptr(cand_off),
                                                           _ptr(cand_doc) if n_cand else None, n_cand, _ptr(ws), ws.numel(), self._stream()),
                        "dprhot_colbert_union_fill")

    # -- centroid interaction over candidate lists (csrc/colbert_cen.h) --------------------------------
    def colbert_cen_workspace(self, nq, chunk, k, like):
        return self._chunk_workspace(self._lib.colbert_cen_workspace_bytes(nq, chunk), nq, k, like)

    def colbert_cen_table(self, index, q, T):
        """Writes T fp32 [nq, C, LT], LT = 16 * ceil(LQ / 16): T[n, c, i] = <q[n, i], centroid_c>, zeros behind LQ
        (dprhot_colbert_cen_table); q bf16 [nq, LQ, dp]."""
        self._require_gpu(index.centroids, q, T)
        nq, LQ, dp = q.shape
        C = int(index.centroids.shape[0])
        assert T.dtype == torch.float32 and T.is_contiguous() and T.shape == (nq, C, (LQ + 15) // 16 * 16)
        self._lib.check(self.lib.dprhot_colbert_cen_table(_ptr(index.centroids), C, dp, _ptr(q), nq, LQ, _ptr(T), self._stream()),
                        "dprhot_colbert_cen_table")

    def _colbert_cen_head(self, index, T, LQ, pool, cand_off, cand_doc):
        """doc_cen_off .. n_cand: the arguments both centroid-interaction entry points begin with; T fp32 [nq, C, LT]."""
        doc_cen_off, doc_cen = index.doc_centroids()
        self._require_gpu(doc_cen_off, doc_cen, T, cand_off, cand_doc)
        nq, C, LT = T.shape
        assert T.dtype == torch.float32 and T.is_contiguous() and LT == (int(LQ) + 15) // 16 * 16
        assert cand_off.dtype == torch.int64 and cand_doc.dtype == torch.int32 and cand_off.shape == (nq + 1,)
        assert cand_off.is_contiguous() and cand_doc.is_contiguous()
        return (_ptr(doc_cen_off), _ptr(doc_cen), int(doc_cen.shape[0]), index.corpus_len, C, _ptr(T), nq, int(LQ), int(pool),
                _ptr(cand_off), _ptr(cand_doc), int(cand_doc.shape[0]))

    def colbert_cen_score(self, index, T, LQ, pool, cand_off, cand_doc, pos_begin, cols, S):
        """Writes the approximate scores of candidate positions pos_begin .. pos_begin + cols of every query's list into S [nq, >= cols]
        fp32; a position without a candidate is NaN (dprhot_colbert_cen_score)."""
        self._require_gpu(S)
        self._lib.check(self.lib.dprhot_colbert_cen_score(*self._colbert_cen_head(index, T, LQ, pool, cand_off, cand_doc), int(pos_begin),
                                                          int(cols), _ptr(S), S.stride(0), self._stream()), "dprhot_colbert_cen_score")

    def colbert_cen_search(self, index, T, LQ, pool, cand_off, cand_doc, max_count, values, indices, chunk, ws):
        """The top-k of every query's candidate list by approximate score, as doc ids (dprhot_colbert_cen_search); always from an empty
        state."""
        self._require_gpu(values, indices, ws)
        self._lib.check(self.lib.dprhot_colbert_cen_search(*self._colbert_cen_head(index, T, LQ, pool, cand_off, cand_doc), int(max_count),
                                                           values.shape[1], int(chunk), _ptr(values), _ptr(indices), _ptr(ws), ws.numel(),
                                                           self._stream()), "dprhot_colbert_cen_search")

    # -- residual-compressed token index under the pruned search (csrc/colbert_res.h) -------------------
    def colbert_res_workspace(self, nq, chunk, k, like):
        return self._chunk_workspace(self._lib.colbert_cand_workspace_bytes(nq, chunk), nq, k, like)

    def colbert_res_encode(self, rows, cutoffs, nbits, tok_centroid=None, centroids=None):
        """uint8 [n, dp * nbits / 8]: the residual codes of bf16 rows [n, dp] under their centroid ids int32 [n] among centroids bf16
        [C, dp] (dprhot_colbert_res_encode); a row whose id lies outside [0, C) gets zero bytes.  `rows` may be a ColBERTIndex with
        centroids instead: its tok, tok_centroid and centroids are taken."""
        if tok_centroid is None:
            rows, tok_centroid, centroids = rows.tok, rows.tok_centroid, rows.centroids
        self._require_gpu(rows, tok_centroid, centroids, cutoffs)
        n, dp = rows.shape
        nbits = int(nbits)
        assert rows.dtype == torch.bfloat16 and centroids.dtype == torch.bfloat16 and centroids.shape[1] == dp
        assert tok_centroid.dtype == torch.int32 and tok_centroid.shape == (n,) and cutoffs.dtype == torch.float32
        assert cutoffs.shape == ((1 << nbits) - 1,) and all(t.is_contiguous() for t in (rows, tok_centroid, centroids, cutoffs))
        codes = torch.empty((n, dp * nbits // 8), dtype=torch.uint8, device=rows.device)
        self._lib.check(self.lib.dprhot_colbert_res_encode(_ptr(rows), _ptr(tok_centroid), n, dp, _ptr(centroids), int(centroids.shape[0]),
                                                           _ptr(cutoffs), nbits, _ptr(codes), self._stream()), "dprhot_colbert_res_encode")
        return codes

    def _colbert_res_head(self, index, q, pool, cand_off, cand_doc):
        """res_code .. n_cand: the arguments both residual entry points begin with; cand_off int64 [nq + 1], cand_doc int32 [n_cand]."""
        self._require_gpu(index.res_code, index.tok_centroid, index.centroids, index.weights, index.doc_blk, q, cand_off, cand_doc)
        nq, LQ, dp = q.shape
        assert cand_off.dtype == torch.int64 and cand_doc.dtype == torch.int32 and cand_off.shape == (nq + 1,)
        assert cand_off.is_contiguous() and cand_doc.is_contiguous()
        return (_ptr(index.res_code), _ptr(index.tok_centroid), _ptr(index.centroids), int(index.centroids.shape[0]), _ptr(index.weights),
                index.nbits, _ptr(index.doc_blk), index.n_blk, index.corpus_len, dp, _ptr(q), nq, LQ, int(pool), _ptr(cand_off),
                _ptr(cand_doc), int(cand_doc.shape[0]))

    def colbert_res_score(self, index, q, pool, cand_off, cand_doc, pos_begin, cols, S):
        """colbert_cand_score over the decoded rows of a ColBERTResidualIndex (dprhot_colbert_res_score)."""
        self._require_gpu(S)
        self._lib.check(self.lib.dprhot_colbert_res_score(*self._colbert_res_head(index, q, pool, cand_off, cand_doc), int(pos_begin),
                                                          int(cols), _ptr(S), S.stride(0), self._stream()), "dprhot_colbert_res_score")

    def colbert_res_search(self, index, q, pool, cand_off, cand_doc, max_count, values, indices, chunk, ws):
        """colbert_cand_search over the decoded rows of a ColBERTResidualIndex (dprhot_colbert_res_search); always from an empty state."""
        self._require_gpu(values, indices, ws)
        self._lib.check(self.lib.dprhot_colbert_res_search(*self._colbert_res_head(index, q, pool, cand_off, cand_doc), int(max_count),
                                                           values.shape[1], int(chunk), _ptr(values), _ptr(indices), _ptr(ws), ws.numel(),
                                                           self._stream()), "dprhot_colbert_res_search")

    # -- SPAR: two resident indexes, a grid of weights in one pass (csrc/spar.h; dpr_scale_amd/spar.py) ----
    def spar_workspace(self, nq, W, chunk, k, like):
        return self._chunk_workspace(self._lib.spar_workspace_bytes(nq, W, chunk), W * nq, k, like)

    def _spar_operands(self, index, q1, q2, lam):
        """Q1, Q2, nq, d1, d2, C1, C2, n_ctx, lam, W: what both SPAR entry points begin with; lam is a host sequence of floats."""
        self._require_gpu(q1, q2, index.c1, index.c2)
        assert q1.dtype == _BF16 and q2.dtype == _BF16 and q1.is_contiguous() and q2.is_contiguous() and q1.shape[0] == q2.shape[0]
        assert q1.shape[1] == index.c1.shape[1] and q2.shape[1] == index.c2.shape[1], "query widths must be the index's padded widths"
        W = len(lam)
        return (_ptr(q1), _ptr(q2), q1.shape[0], q1.shape[1], q2.shape[1], _ptr(index.c1), _ptr(index.c2), index.corpus_len,
                (ctypes.c_float * W)(*[float(x) for x in lam]), W)

    def spar_score(self, index, q1, q2, lam, doc_begin, cols, S):
        """Writes s[w][i][j] = fma(lam[w], <q2[i], c2[j]>, <q1[i], c1[j]>) of passages doc_begin .. doc_begin + cols into S [W * nq, >= cols]
        fp32, row w * nq + i (dprhot_spar_score)."""
        self._require_gpu(S)
        self._lib.check(self.lib.dprhot_spar_score(*self._spar_operands(index, q1, q2, lam), int(doc_begin), int(cols), _ptr(S), S.stride(0),
                                                   self._stream()), "dprhot_spar_score")

    def spar_search(self, index, q1, q2, lam, id_begin, id_end, values, indices, first, chunk, ws):
        """Folds passage ids [id_begin, id_end) into the running top-k of every weight, values / indices [W * nq, k] (dprhot_spar_search)."""
        self._require_gpu(values, indices, ws)
        self._lib.check(self.lib.dprhot_spar_search(*self._spar_operands(index, q1, q2, lam),
                                                    *self._topk_tail(id_begin, id_end, values, indices, first, chunk, ws)),
                        "dprhot_spar_search")

    # -- the fp8 dense index: e4m3fn rows, one power-of-two scale per row (csrc/dense_fp8.h; dense_fp8.py) ----
    def fp8_encode(self, rows, codes, scale):
        """codes uint8 [n, dp] and scale fp32 [n] (both contiguous, written in full) <- rows fp32 or bf16 [n, d] (dprhot_fp8_encode)."""
        self._require_gpu(rows, codes, scale)
        assert rows.dtype in (torch.float32, _BF16) and rows.dim() == 2 and rows.is_contiguous(), "rows: contiguous fp32 or bf16 [n, d]"
        n, d = rows.shape
        assert codes.dtype == torch.uint8 and codes.is_contiguous() and codes.shape[0] == n and scale.dtype == torch.float32
        assert scale.is_contiguous() and scale.shape == (n,)
        self._lib.check(self.lib.dprhot_fp8_encode(_ptr(rows), int(rows.dtype == _BF16), n, d, codes.shape[1], _ptr(codes), _ptr(scale),
                                                   self._stream()), "dprhot_fp8_encode")

    def dense_fp8_workspace(self, nq, chunk, k, like):
        return self._chunk_workspace(self._lib.dense_fp8_workspace_bytes(nq, chunk), nq, k, like)

    def _dense_fp8_operands(self, index, qc, qs):
        """Qc, qs, nq, Cc, cs, n_ctx, dp: what both entry points of the fp8 dense index begin with."""
        self._require_gpu(qc, qs, index.codes, index.scale)
        assert qc.dtype == torch.uint8 and qs.dtype == torch.float32 and qc.is_contiguous() and qs.shape == (qc.shape[0],)
        assert qc.shape[1] == index.codes.shape[1], "query codes must have the index's padded width"
        return _ptr(qc), _ptr(qs), qc.shape[0], _ptr(index.codes), _ptr(index.scale), index.corpus_len, qc.shape[1]

    def dense_fp8_score(self, index, qc, qs, doc_begin, cols, S):
        """Writes s[i][j] = (<value(qc[i]), value(codes[j])> * qs[i]) * scale[j] of passages doc_begin .. doc_begin + cols into
        S [nq, >= cols] fp32 (dprhot_dense_fp8_score)."""
        self._require_gpu(S)
        self._lib.check(self.lib.dprhot_dense_fp8_score(*self._dense_fp8_operands(index, qc, qs), int(doc_begin), int(cols), _ptr(S),
                                                        S.stride(0), self._stream()), "dprhot_dense_fp8_score")

    def dense_fp8_search(self, index, qc, qs, id_begin, id_end, values, indices, first, chunk, ws):
        """Folds passage ids [id_begin, id_end) into the running top-k, values / indices [nq, k] (dprhot_dense_fp8_search)."""
        self._require_gpu(values, indices, ws)
        self._lib.check(self.lib.dprhot_dense_fp8_search(*self._dense_fp8_operands(index, qc, qs),
                                                         *self._topk_tail(id_begin, id_end, values, indices, first, chunk, ws)),
                        "dprhot_dense_fp8_search")

    # -- product-quantised postings (csrc/ivf_pq.h; dpr_scale_amd/ivf.py owns training and the index) ----
    def pq_encode(self, vec, codebook, entry="dprhot_pq_encode"):
        """codes uint8 [n, m] of the rows vec bf16 [n, dp] under codebook bf16 [m, 256, dsub] (dprhot_pq_encode)."""
        self._require_gpu(vec, codebook)
        assert vec.dtype == torch.bfloat16 and codebook.dtype == torch.bfloat16 and vec.dim() == 2 and codebook.dim() == 3
        vec, codebook = vec.contiguous(), codebook.contiguous()
        n, dp = vec.shape
        m, _, dsub = codebook.shape
        assert codebook.shape[1] == 256 and m * dsub == dp, f"codebook {tuple(codebook.shape)} for rows of width {dp}"
        codes = torch.empty((n, m), dtype=torch.uint8, device=vec.device)
        self._lib.check(getattr(self.lib, entry)(_ptr(vec), n, dp, _ptr(codebook), dsub, _ptr(codes), self._stream()), entry)
        return codes

    def _ivf_pq_index(self, index):
        self._require_gpu(index.post_code, index.codebook, index.post_doc, index.exp_off)
        return (_ptr(index.post_code), _ptr(index.codebook), index.dsub, _ptr(index.post_doc), _ptr(index.exp_off), index.n_postings,
                index.n_experts, index.dp)

    def ivf_pq_score(self, index, qb, doc_begin, cols, S):
        """ivf_score for an IVFPQIndex (dprhot_ivf_pq_score)."""
        self._require_gpu(S)
        self._lib.check(self.lib.dprhot_ivf_pq_score(*self._ivf_pq_index(index), *self._ivf_batch(qb), int(doc_begin), int(cols), _ptr(S),
                                                     S.stride(0), self._stream()), "dprhot_ivf_pq_score")

    def ivf_pq_search(self, index, qb, id_begin, id_end, values, indices, first, chunk, ws):
        """ivf_search for an IVFPQIndex (dprhot_ivf_pq_search); the workspace is ivf_workspace's."""
        self._require_gpu(index.cls, qb.cls, values, indices, ws)
        self._lib.check(self.lib.dprhot_ivf_pq_search(*self._ivf_pq_index(index), *self._ivf_batch(qb), *self._ivf_cls(index, qb),
                                                      *self._topk_tail(id_begin, id_end, values, indices, first, chunk, ws)),
                        "dprhot_ivf_pq_search")

    # -- product-quantised ColBERT token index (csrc/colbert_pq.h; dpr_scale_amd/colbert.py owns the index) ----
    def colbert_pq_encode(self, vec, codebook):
        """pq_encode for rows of padded width up to 128 (dprhot_colbert_pq_encode: the same rule, the same kernel)."""
        return self.pq_encode(vec, codebook, entry="dprhot_colbert_pq_encode")

    def _colbert_pq_index(self, index):
        self._require_gpu(index.tok_code, index.blk_rows, index.codebook, index.doc_blk)
        return (_ptr(index.tok_code), _ptr(index.blk_rows), _ptr(index.codebook), index.dsub, _ptr(index.doc_blk), index.n_blk,
                index.corpus_len, index.dp)

    def colbert_pq_score(self, index, q, pool, doc_begin, cols, S):
        """colbert_score for a ColBERTPQIndex (dprhot_colbert_pq_score)."""
        self._require_gpu(q, S)
        nq, LQ, dp = q.shape
        assert dp == index.dp
        self._lib.check(self.lib.dprhot_colbert_pq_score(*self._colbert_pq_index(index), _ptr(q), nq, LQ, int(pool), int(doc_begin), int(cols),
                                                         _ptr(S), S.stride(0), self._stream()), "dprhot_colbert_pq_score")

    def colbert_pq_search(self, index, q, pool, id_begin, id_end, values, indices, first, chunk, ws):
        """colbert_search for a ColBERTPQIndex (dprhot_colbert_pq_search); the workspace is colbert_workspace's."""
        self._require_gpu(q, values, indices, ws)
        nq, LQ, dp = q.shape
        assert dp == index.dp
        self._lib.check(self.lib.dprhot_colbert_pq_search(*self._colbert_pq_index(index), _ptr(q), nq, LQ, int(pool),
                                                          *self._topk_tail(id_begin, id_end, values, indices, first, chunk, ws)),
                        "dprhot_colbert_pq_search")

    # -- postings and query batches from encoder outputs (csrc/ivf_pack.h; dpr_scale_amd/ivf.py drives them) ----
    def ivf_compact(self, expert_ids, weights, att, row_ids, test_weight, min_weight=0.0, capacity=None):
        """The kept slots of a repr dict in (b, t, k) order (dprhot_ivf_compact).  expert_ids [B, L, K] of any integer type, weights
        [B, L, K] or None (all 1), att [B, L] (> 0 = a real token), row_ids [B].  Returns (n, largest count of one sequence, seq_off
        int32 [B + 1], expert, row, slot int32 [m], weight fp32 [m]) with m = min(n, capacity); capacity defaults to the worst case
        B L K.  n and the largest count come to the host in ONE transfer (the call's only synchronisation)."""
        self._require_gpu(expert_ids, weights, att, row_ids)
        B, L, K = expert_ids.shape
        dev = expert_ids.device
        ids = expert_ids.detach().to(torch.int32).contiguous()
        w = None if weights is None else weights.detach().to(torch.float32).contiguous()
        a8 = (att.detach() > 0).to(torch.uint8).contiguous()
        rows = row_ids.detach().to(torch.int32).contiguous()
        assert a8.shape == (B, L) and rows.shape == (B,) and (w is None or w.shape == ids.shape)
        cap = B * L * K if capacity is None else int(capacity)
        seq_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
        expert, row, slot = (torch.empty(max(cap, 1), dtype=torch.int32, device=dev) for _ in range(3))  # (never a NULL pointer)
        weight = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
        self._lib.check(self.lib.dprhot_ivf_compact(_ptr(ids), _ptr(w), _ptr(a8), _ptr(rows), B, L, K, int(bool(test_weight)),
                                                    float(min_weight), _ptr(seq_off), _ptr(expert), _ptr(row), _ptr(slot), _ptr(weight),
                                                    cap, self._stream()), "dprhot_ivf_compact")
        n, most = torch.stack([seq_off[B], (seq_off[1:] - seq_off[:-1]).max()]).tolist()
        m = min(n, cap)
        return n, most, seq_off, expert[:m], row[:m], slot[:m], weight[:m]

    def ivf_gather(self, expert_repr, weights, slot, perm, K, entry_fp16, out_dtype, out_ld=None):
        """out [n, out_ld] (fp32 or bf16): row i = weight * token row of record perm[i] (record i without perm), rounded as torch rounds
        in the host loops -- the product to P, then to fp16 when entry_fp16, then to out_dtype (dprhot_ivf_gather).  P is the dtype of
        `one weight * one token row`, torch.result_type of a 0-dim weight and the row: the row's dtype, and torch casts the weight to
        it before it multiplies.  expert_repr [..., d] and weights [..., K] come in their own dtypes; the widening of P to fp32 done
        here is exact."""
        self._require_gpu(expert_repr, weights, slot, perm)
        d = int(expert_repr.shape[-1])
        prod = expert_repr.dtype if weights is None else torch.result_type(weights.new_zeros(()), expert_repr)
        if prod not in _IVF_ROUND or out_dtype not in (torch.float32, _BF16):
            raise TypeError(f"ivf_gather: product of {prod}, output of {out_dtype}; fp32, bf16 and fp16 products, fp32 and bf16 outputs")
        x = expert_repr.detach().reshape(-1, d).to(torch.float32)
        if x.stride(1) != 1 or x.stride(0) < d:
            x = x.contiguous()
        w = None if weights is None else weights.detach().to(prod).to(torch.float32).contiguous()
        assert w is None or w.numel() == x.shape[0] * K
        n = int(slot.shape[0])
        out_ld = d if out_ld is None else int(out_ld)
        out = torch.empty((n, out_ld), dtype=out_dtype, device=x.device)
        assert slot.dtype == torch.int32 and slot.is_contiguous() and (perm is None or (perm.dtype == torch.int64 and perm.is_contiguous()
                                                                                        and perm.shape[0] == n))
        self._lib.check(self.lib.dprhot_ivf_gather(_ptr(x), x.stride(0), x.shape[0], _ptr(w), _ptr(slot), _ptr(perm), n, d, int(K),
                                                   _IVF_ROUND[prod], int(bool(entry_fp16)), _IVF_ROUND[out_dtype], _ptr(out), out_ld,
                                                   self._stream()), "dprhot_ivf_gather")
        return out


_DEFAULT = None


def _load_opx():
    """csrc/opx.cpp, built next to libdprhot.so by `make -C dpr_scale_amd/csrc` / __graft_entry__.build(); DPRHOT_OPX=0 keeps the
    Python host path (A/B).  Optional: without it the operator is the same operator, ~150 us per step slower on the host."""
    if os.environ.get("DPRHOT_OPX", "1") == "0":
        return None
    try:
        from . import _lib, _opx
    except ImportError:
        return None
    _opx.init(_lib.LIB_PATH)
    return _opx


try:
    _OPX = _load_opx()
except Exception:  # pragma: no cover - a broken optional extension must not take the operator down
    _OPX = None


# the multi-rank packed step's host side in C++ (csrc/opx.cpp: packed_train_step / packed_backward); DPRHOT_OPX_PACKED=0: the Python wrappers
_OPX_PACKED = _OPX is not None and os.environ.get("DPRHOT_OPX_PACKED", "1") != "0"


def default_kernels():
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = HipKernels()
    return _DEFAULT


def _pad_cols(n):
    return (n + 7) // 8 * 8


def _mask_u8(mask):
    """The mask as bytes: a bool mask viewed in place, any other mask converted."""
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)


def _mask_bytes(mask):
    """A bool mask viewed as bytes in place, any other mask as it is (it already is one byte per element)."""
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


class ContextGather:
    """The forward collective, started as soon as the context tower has produced its rows:
    pack (bf16 rows + mask bytes) on the compute stream, then ONE all-gather with async_op=True -- it runs on RCCL's
    own stream while the query tower keeps the compute stream busy.  InBatchContrastive waits on it right before
    the sim GEMM.  Usage (what DenseRetrieverTask.training_step does):

        c  = encode_contexts(...)
        c, pending = defer_context_grad(c)            # see below: lets the reduce-scatter overlap the query-tower backward
        g  = ContextGather(c, ctx_mask, group)        # all-gather in flight ...
        q  = encode_queries(...)                      # ... under the query tower
        loss = inbatch_contrastive_loss(q, c, pos, ctx_mask, T, group, gather=g, pending=pending)
    """

    def __init__(self, c, ctx_mask, group=None, kernels=None):
        kn = kernels if kernels is not None else default_kernels()
        W, r = D.world(group)
        assert W > 1 or D.force_dist(), "ContextGather is for world size > 1"
        n_ctx, d = c.shape
        m8 = _mask_u8(ctx_mask)
        self.rows_c = kn.packed_rows(n_ctx, d)
        self.send = kn.empty((self.rows_c, d), _BF16, c)
        kn.pack_ctx(c.detach(), m8, self.send)
        self.Cb = kn.empty((W * self.rows_c, d), _BF16, c)
        self.work = D.all_gather_rows(self.send, self.Cb, group, async_op=True)
        self.shape = (n_ctx, d)

    def wait(self):
        if self.work is not None:
            self.work.wait()  # the compute stream waits for RCCL's stream; the host does not block
            self.work = None
        return self.Cb


class PendingGrad:
    """Carries the reduce-scatter started in InBatchContrastive.backward to the point where its result is consumed."""

    def __init__(self):
        self.work = None
        self.post = None  # run on the gradient after the wait (half-width wire: widen the received rows into it)


class _DeferContextGrad(torch.autograd.Function):
    """Identity on the context rows whose backward first waits for the pending reduce-scatter.  Placed right after
    the context tower and BEFORE the query tower runs, its autograd node is older than every query-tower node, so
    the engine runs the whole query-tower backward (it only needs dq) before it gets here: the collective overlaps
    it on RCCL's stream."""

    @staticmethod
    def forward(ctx, c, pending):
        ctx.pending = pending
        return c.view_as(c)

    @staticmethod
    def backward(ctx, grad):
        w, ctx.pending.work = ctx.pending.work, None
        if w is not None:
            w.wait()
        post, ctx.pending.post = ctx.pending.post, None
        if post is not None:
            out = post(grad)  # (may hand on a different tensor: the half-width wire's widened rows)
            grad = out if out is not None else grad
        return grad, None


def defer_context_grad(c):
    pending = PendingGrad()
    return _DeferContextGrad.apply(c, pending), pending


# ---- the operator's parts.  Every kernel set offers what HipKernels offers (the stand-in of the CPU tests included): nothing here asks
# what it was given.  The staged operands and the step's result travel as plain tuples and _Bwd takes attribute stores (a constructor
# call per step shows in the eager step's host time).
PRESCALED = "PRESCALED"      # gradients computed in forward by a train_step_* entry point, scaled by the predicted grad_output
#                              (opx_packed: the packed step's host side in csrc/opx.cpp)
SAVED = "SAVED"              # forward only: Qb, Cb, G saved for the backward GEMMs
FP32G_DEBUG = "FP32G_DEBUG"  # DPRHOT_FP32_G=1: the logits kept, dScores rebuilt in fp32 and sent through the GEMMs as a bf16 pair
REGEN = "REGEN"              # what PRESCALED turns into once it has given its tensors away: the backward GEMMs again


class _Bwd:
    """The one record forward leaves on ctx: kind, row_lse and that kind's fields -- PRESCALED: grads, used, site, opx_packed + REGEN's;
    REGEN: Qb, Cb, G, pos_idx, y_off, mask (None: still packed in Cb), inv_T, grad_scale;  FP32G_DEBUG: S, labels, gs
    (SAVED and FP32G_DEBUG keep Qb, Cb, G in ctx.saved_tensors).  All carry what backward needs besides: kn, group, W, n_ctx, rows_c,
    d, multi, direct_ctx_grad, in_dtypes, pending."""

    __slots__ = ("kind", "row_lse", "grads", "used", "site", "opx_packed", "Qb", "Cb", "G", "pos_idx", "y_off", "mask", "inv_T", "grad_scale",
                 "S", "labels", "gs", "kn", "group", "W", "n_ctx", "rows_c", "d", "multi", "direct_ctx_grad", "in_dtypes", "pending")


def _plain_single_rank(q, group, kernels):
    """The C++ node of inbatch_contrastive_loss asks first: own kernels, a device, one rank, no debug mode."""
    return kernels is None and q.is_cuda and (group is False or D.world(group)[0] == 1) and not _fp32_g_mode() and not (D.force_dist() and group is not False)


def _stage_single(kn, q, c, m8, Qb, q_f32):
    """One rank: columns = this rank's contexts (padded to 8 with masked zero rows).  -> (Qb, Cb, colmask, rows_c, Nc, c_direct, q_f32, packed_step)"""
    n_ctx, d = c.shape
    Nc = _pad_cols(n_ctx)
    Cb = kn.empty((Nc, d), _BF16, c)
    if Nc == n_ctx:
        colmask = m8 if m8.is_contiguous() else m8.contiguous()  # the batch's own bool mask, read in place
    else:
        colmask = kn.empty((Nc,), torch.uint8, c)
        colmask[:n_ctx].copy_(m8)
        Cb[n_ctx:].zero_()
        colmask[n_ctx:].fill_(1)
    # fp32 encoder outputs are consumed as they are by the sim kernel (it rounds to bf16 while staging and leaves the bf16 images in Qb / Cb)
    c_direct = q_f32 and c.dtype == torch.float32 and Nc == n_ctx
    if not c_direct:
        kn.prep(q, Qb, c, Cb[:n_ctx])
        q_f32 = False
    return Qb, Cb, colmask, Nc, Nc, c_direct, q_f32, False


def _stage_multi(kn, q, c, m8, Qb, q_f32, W, group, gather, wants_grad):
    """Several ranks.  ONE all-gather: context rows (bf16) + mask bytes in trailing rows of the same buffer; the trailing
    rows become always-masked extra columns (the reference issues 4 fp32 all_gathers, :169-176).  -> as _stage_single"""
    n_ctx, d = c.shape
    rows_c = kn.packed_rows(n_ctx, d)
    Nc = W * rows_c
    if gather is not None:  # started under the query tower (ContextGather): only wait here
        assert gather.shape == (n_ctx, d)
        Cb = gather.wait()
    else:
        send = kn.empty((rows_c, d), _BF16, c)
        kn.pack_ctx(c, m8, send)
        Cb = kn.empty((Nc, d), _BF16, c)
        D.all_gather_rows(send, Cb, group)
    # with a backward to follow, the one-call step reads the mask straight from the gathered buffer: no unpack launch
    packed_step = q_f32 and wants_grad
    colmask = None
    if not packed_step:
        colmask = kn.empty((Nc,), torch.uint8, c)
        kn.unpack_mask(Cb, W, n_ctx, colmask)
    if not q_f32:
        kn.cast_bf16(q, Qb)
    return Qb, Cb, colmask, rows_c, Nc, False, q_f32, packed_step


def _run_step(kn, q, c32, Qb, Cb, colmask, Nc, q_f32, packed_step, pos_idx, W, r, n_ctx, inv_T, grad_scale, y_off, multi, wants_grad, dc_dtype, kernels):
    """Choose the step's route and run it.  -> (bw, loss_sum, loss_is_mean, saved): the _Bwd with its kind, row_lse and that kind's own
    fields; the loss numerator (already the mean when loss_is_mean: the kernel multiplied it by 1 / Nq); the tensors for forward to save."""
    B, d = q.shape
    Nq = W * B
    bw = _Bwd()
    if not multi and _fp32_g_mode() and wants_grad:
        _, bw.row_lse, loss_sum, G, bw.S = (kn.inbatch_fwd_f32(q, c32, Qb, Cb, pos_idx, y_off, colmask, inv_T, grad_scale, want_logits=True) if q_f32
                                            else kn.inbatch_fwd(Qb, Cb, pos_idx, y_off, colmask, inv_T, grad_scale, want_logits=True))
        bw.kind, bw.gs = FP32G_DEBUG, grad_scale  # (forward adds the labels)
        return bw, loss_sum, False, (Qb, Cb, G)
    if not (q_f32 and wants_grad):
        _, bw.row_lse, loss_sum, G, _ = (kn.inbatch_fwd_f32(q, c32, Qb, Cb, pos_idx, y_off, colmask, inv_T, grad_scale) if q_f32
                                         else kn.inbatch_fwd(Qb, Cb, pos_idx, y_off, colmask, inv_T, grad_scale))
        bw.kind = SAVED
        return bw, loss_sum, False, (Qb, Cb, G)
    # a backward will follow: forward and backward of this rank's rows in ONE library call (two launches at the BASELINE shapes), the
    # gradients scaled by the grad_output the last backward saw; backward() only checks the grad_output it was given against that one
    bw.used = used = _ExpectedGradScale.get(q.device, (B, Nc, d))
    bw.opx_packed = False
    if packed_step:
        if _OPX_PACKED and kernels is None and q.is_contiguous() and pos_idx.dtype == torch.int64 and pos_idx.is_contiguous() \
                and dc_dtype in (torch.float32, _BF16):
            # host side in C++ (csrc/opx.cpp: packed_train_step): the allocations, the library call and its fall-back to fp32
            # partials in one function; backward's counterpart is packed_backward
            loss_sum, bw.row_lse, dQ, dC_part, Qb, G, part = _OPX.packed_train_step(q.detach(), Cb, pos_idx, W, r, n_ctx, inv_T, grad_scale,
                                                                                    1.0 / Nq, used, 0 if dc_dtype == _BF16 else 2)
            G = G if (G is not None and G.numel() > 0) else None  # (an undefined at::Tensor arrives as None)
            if part is not None and part.numel() > 0:
                dQ = (dQ, part)
            bw.opx_packed = True
        else:
            try:
                _, bw.row_lse, loss_sum, G, dQ, dC_part = kn.train_step_packed_f32(q, Cb, Qb, W, r, n_ctx, pos_idx, inv_T, grad_scale, 1.0 / Nq,
                                                                                   used, dc_dtype, defer_dq=True, want_G="auto")
            except Exception as e:  # a plan without a bf16 dC epilogue: fp32 partials, rounded to the wire format in backward
                if dc_dtype == torch.float32 or "dc_kind" not in str(e):
                    raise
                _, bw.row_lse, loss_sum, G, dQ, dC_part = kn.train_step_packed_f32(q, Cb, Qb, W, r, n_ctx, pos_idx, inv_T, grad_scale, 1.0 / Nq,
                                                                                   used, torch.float32, defer_dq=True, want_G="auto")
    else:
        _, bw.row_lse, loss_sum, G, dQ, dC_part = kn.train_step_f32(q, c32, Qb, Cb, pos_idx, y_off, colmask, inv_T, grad_scale, 1.0 / Nq, used,
                                                                    defer_dq=True, want_G="auto")
    bw.grads, bw.kind = (dQ, dC_part), PRESCALED
    # (what REGEN will need; mask None: still packed in Cb)
    bw.Qb, bw.Cb, bw.G, bw.pos_idx, bw.y_off, bw.mask, bw.inv_T, bw.grad_scale = Qb, Cb, G, pos_idx, y_off, colmask, inv_T, grad_scale
    return bw, loss_sum, True, None


def _regen_grads(kn, Qb, Cb, G, pos_idx, y_off, mask, inv_T, grad_scale, go, need_dq, need_dc, packed=None):
    """A second backward through a retained graph: the first one gave its gradient tensors away; the backward GEMMs run again on the
    operands the step left behind (exact, rare).  The dScores are recomputed first where the step never materialised them (G is None),
    the mask unpacked from the gathered buffer where the step read it there (mask None; packed = (W, n_ctx)).  -> (dQ, dC, G to keep)."""
    if G is None:
        if mask is None:
            mask = kn.empty((Cb.shape[0],), torch.uint8, Cb)
            kn.unpack_mask(Cb, packed[0], packed[1], mask)
        G = kn.inbatch_fwd(Qb, Cb, pos_idx, y_off, _mask_bytes(mask), inv_T, grad_scale)[3]
    dQ, dC = kn.inbatch_bwd(G, Qb, Cb, 1.0, go, need_dq, need_dc)
    return dQ, dC, G


def _local_grads(ctx, st, go, need_dq, need_dc):
    """This rank's gradients, grad_output applied, for every kind but the per-step one (PRESCALED: in backward itself) -> (dQ, dC_part)."""
    kn, kind = st.kn, st.kind
    if kind is REGEN:
        dQ, dC_part, st.G = _regen_grads(kn, st.Qb, st.Cb, st.G, st.pos_idx, st.y_off, st.mask, st.inv_T, st.grad_scale, go, need_dq, need_dc,
                                         (st.W, st.n_ctx))
        return dQ, dC_part
    Qb, Cb, G = ctx.saved_tensors
    if kind is FP32G_DEBUG:
        # fp32-G debug mode: G = (exp(S - lse) - onehot) * scale recomputed in fp32, split into a bf16 pair, two GEMM passes
        S = st.S
        G32 = torch.exp(S - st.row_lse[:, None])
        G32[torch.arange(S.shape[0], device=S.device), st.labels] -= 1.0
        G32 *= st.gs
        hi = G32.to(_BF16)
        lo = (G32 - hi.float()).to(_BF16)
        dQ1, dC1 = kn.inbatch_bwd(hi, Qb, Cb, 1.0, go, need_dq, need_dc)
        dQ2, dC2 = kn.inbatch_bwd(lo, Qb, Cb, 1.0, go, need_dq, need_dc)
        return (dQ1 + dQ2 if need_dq else None), (dC1 + dC2 if need_dc else None)
    return kn.inbatch_bwd(G, Qb, Cb, 1.0, go, need_dq, need_dc)


def _reduce_context_grads(st, dC_part, mine_ready):
    """Several ranks: dc = this rank's rows of the sum over ranks of the dC partials (grad_output already in them), in the dtype c came in."""
    kn, group, n_ctx, d, c_dtype = st.kn, st.group, st.n_ctx, st.d, st.in_dtypes[1]
    wire = _dc_wire_dtype(group)
    mine = mine_ready if mine_ready is not None else kn.empty((st.rows_c, d), wire, dC_part)
    if dC_part.dtype != wire:
        dC_part = dC_part.to(wire)  # half the bytes on the links (and in RCCL's reduction)
    widen = wire != c_dtype and c_dtype == torch.float32
    if st.pending is not None and st.direct_ctx_grad and (wire == c_dtype or widen):
        # reduce-scatter on RCCL's stream; whoever consumes dc (defer_context_grad, after the query-tower backward has
        # been enqueued) waits for it -- and, on a half-width wire, widens the result into the fp32 gradient there.
        # Only in the task's own flow (c IS the output of defer_context_grad: `gather` given), where autograd hands this
        # very tensor to that node.  Should anything still sit in between (another consumer of c, a hook), the tensor that
        # arrives there is a different one: the half-width wire therefore returns ZEROS here (whatever autograd adds to
        # them stays right) and post() adds the widened rows to whatever arrives instead of overwriting it.
        st.pending.work = D.reduce_scatter_rows(dC_part, mine, group, async_op=True)
        if not widen:
            return mine[:n_ctx]
        # nothing to return yet: a gradient of zeros that costs no launch (one cached zero, expanded).  post() hands
        # the widened rows on in its place, or adds them to whatever autograd made of it (zeros + somebody else's term)
        dc = _zeros_view((n_ctx, d), mine.device)

        def post(g, kn=kn, mine=mine, zptr=dc.data_ptr(), shape=(n_ctx, d)):
            if g.data_ptr() == zptr and g.stride() == (0, 0):
                return kn.widen(mine, kn.empty(shape, torch.float32, mine))
            g.add_(kn.widen(mine, kn.empty(shape, torch.float32, mine)).to(g.dtype))
            return g

        st.pending.post = post
        return dc
    D.reduce_scatter_rows(dC_part, mine, group)  # sum over ranks of the partials of MY columns
    return kn.widen(mine, kn.empty((n_ctx, d), torch.float32, mine)) if widen else mine[:n_ctx].to(c_dtype)


class InBatchContrastive(torch.autograd.Function):
    """loss = InBatchContrastive.apply(q_local, c_local, pos_idx, ctx_mask, temperature, group, kernels)

    q_local [B,d], c_local [B*K,d] (fp32 or bf16, requires_grad), pos_idx [B] int64 rank-local positive
    indices (dpr_transform.py:164-166), ctx_mask [B*K] bool (dummy-context mask, dpr_transform.py:143-157).
    Returns the scalar fp32 loss, identical on every rank (mean over the W*B global queries), exactly the
    value dpr_task.py:212 returns.  backward returns (dq_local, dc_local): the same tensors the reference's
    autograd leaves in q.grad / c.grad on this rank.
    """

    @staticmethod
    def forward(ctx, q, c, pos_idx, ctx_mask, temperature, group, kernels, gather=None, pending=None):
        wants_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        inv_T = 1.0 / float(temperature)
        kn = kernels if kernels is not None else default_kernels()
        W, r = (1, 0) if group is False else D.world(group)  # group=False: single-device strategy, never gather
        B, d = q.shape
        n_ctx = c.shape[0]  # contexts on this rank (B*K)
        Nq = W * B
        assert pos_idx.shape[0] == B and ctx_mask.shape[0] == n_ctx
        if d % 8 != 0:
            raise ValueError(f"hidden size {d} must be a multiple of 8")
        multi = W > 1 or (group is not False and D.force_dist())  # (forced: the multi-rank code path on a one-rank world, for timelines)
        m8 = _mask_u8(ctx_mask)
        q_f32 = q.dtype == torch.float32
        Qb = kn.empty((B, d), _BF16, q)
        Qb, Cb, colmask, rows_c, Nc, c_direct, q_f32, packed_step = (
            _stage_multi(kn, q, c, m8, Qb, q_f32, W, group, gather, wants_grad) if multi else _stage_single(kn, q, c, m8, Qb, q_f32))
        grad_scale = inv_T / Nq  # d loss / d S of the global mean, before grad_output
        y_off = r * rows_c       # dpr_task.py:189-190 (label offset of this rank's columns)
        dc_dtype = _dc_wire_dtype(group) if multi else torch.float32
        bw, loss_sum, loss_is_mean, saved = _run_step(kn, q, c if c_direct else None, Qb, Cb, colmask, Nc, q_f32, packed_step, pos_idx, W, r,
                                                      n_ctx, inv_T, grad_scale, y_off, multi, wants_grad, dc_dtype, kernels)
        loss_sum = loss_sum[:1]
        if multi:
            D.all_reduce_sum(loss_sum, group)  # (of the means when loss_is_mean: the sum over ranks is the global mean)
        loss = (loss_sum if loss_is_mean else loss_sum / Nq).reshape(())
        if saved is not None:
            ctx.save_for_backward(*saved)
        if bw.kind is FP32G_DEBUG:
            bw.labels = pos_idx + y_off
        ctx.state = bw
        bw.kn, bw.group, bw.W, bw.n_ctx, bw.rows_c, bw.d, bw.site, bw.multi = kn, group, W, n_ctx, rows_c, d, (B, Nc, d), multi
        # direct_ctx_grad: c came straight from defer_context_grad (the task's own flow)
        bw.direct_ctx_grad, bw.in_dtypes, bw.pending = gather is not None, (q.dtype, c.dtype), pending if multi else None
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        st = ctx.state
        need_dq, need_dc = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        go = grad_out.detach().reshape(1).float().contiguous()  # device scalar: AMP loss scale, no host sync
        mine_ready = None  # (the reduce-scatter's receive buffer, where csrc/opx.cpp has made it already)
        if st.kind is PRESCALED:
            # computed in forward for grad_output = *st.used; ONE launch compares and only rescales when the scale really changed.
            # The tensors are handed to autograd and FORGOTTEN here: AccumulateGrad takes a gradient nobody else references as
            # .grad itself, and clones it otherwise (one copy launch per step, 50 MB of traffic at cfg3 per rank).
            dQs, dC_part = st.grads
            dQ, part = dQs if isinstance(dQs, tuple) else (dQs, None)  # (dQ buffer, split-K slabs: the rescale adds them up into the buffer)
            if st.opx_packed:
                # csrc/opx.cpp: the rescale launch, dC_part in the wire format (one cast launch where the step wrote fp32 for a bf16 wire)
                # and the reduce-scatter's receive buffer, in one C++ call
                nxt, dC_part, mine_ready = _OPX.packed_backward(dQ, part, dC_part, go, st.used, 0 if _dc_wire_dtype(st.group) == _BF16 else 2,
                                                                st.rows_c, need_dq, need_dc)
            else:
                nxt = st.kn.rescale_grads(dQs if need_dq else None, dC_part if need_dc else None, go, st.used)[1:2]
            st.kind, st.grads, st.used = REGEN, None, None
            _ExpectedGradScale.publish(go.device, nxt, st.site)
        else:
            dQ, dC_part = _local_grads(ctx, st, go, need_dq, need_dc)
        dq = dc = None
        if need_dq:
            dq = dQ.to(st.in_dtypes[0])
        if need_dc and st.multi:
            dc = _reduce_context_grads(st, dC_part, mine_ready)
        elif need_dc:
            dc = dC_part[:st.n_ctx].to(st.in_dtypes[1])
        return dq, dc, None, None, None, None, None, None, None


def _pad_hidden(q, c):
    """Hidden sizes that are not a multiple of 8 (16-byte bf16 rows) get zero columns appended: dot products are
    unchanged and autograd slices the gradients back (e.g. 30522-wide router vectors, citadel_task.py:249-262)."""
    pad = (-q.shape[1]) % 8
    if pad == 0:
        return q, c
    return torch.nn.functional.pad(q, (0, pad)), torch.nn.functional.pad(c, (0, pad))


def _opx_regen(Qb, Cb, G, pos_idx, mask, inv_T, grad_scale, go, need_dq, need_dc):
    """Second backward through a retained graph of the C++ node (csrc/opx.cpp: InBatchFn::backward): see _regen_grads."""
    return _regen_grads(default_kernels(), Qb, Cb, G, pos_idx, 0, mask, inv_T, grad_scale, go.reshape(1), need_dq, need_dc)


_OPX_NODE = _OPX is not None and os.environ.get("DPRHOT_OPX_NODE", "1") != "0"
if _OPX_NODE:
    _OPX.set_regen(_opx_regen)


def inbatch_contrastive_loss(q, c, pos_idx, ctx_mask, temperature=1.0, group=None, kernels=None, gather=None, pending=None):
    if gather is None:
        if _OPX_NODE and _plain_single_rank(q, group, kernels):
            # the plain single-rank fp32 step: a C++ autograd node (csrc/opx.cpp), no Python frame in forward or backward
            # (DPRHOT_OPX_NODE=0: InBatchContrastive on HipKernels' wrappers, the same two library calls from Python)
            loss = _OPX.inbatch_loss(q, c, pos_idx, ctx_mask, 1.0 / float(temperature), default_kernels()._lib.options_epoch())
            if loss is not None:
                return loss
        q, c = _pad_hidden(q, c)
    return InBatchContrastive.apply(q, c, pos_idx, ctx_mask, temperature, group, kernels, gather, pending)


class WindowedContrastive(torch.autograd.Function):
    """in_batch_negatives=False (dpr_task.py:198-207): query i is scored only against its own K contexts
    [pos_i, pos_i + K) (dummy ones masked).  No gather in the reference on this branch either."""

    @staticmethod
    def forward(ctx, q, c, pos_idx, ctx_mask, temperature, kernels):
        kn = kernels if kernels is not None else default_kernels()
        B, d = q.shape
        n_ctx = c.shape[0]
        K = n_ctx // B
        Nc_pad = _pad_cols(n_ctx)
        Qb = kn.empty((B, d), _BF16, q)
        Cb = kn.empty((Nc_pad, d), _BF16, c)
        kn.prep(q, Qb, c, Cb[:n_ctx])
        m8 = torch.ones(Nc_pad, dtype=torch.uint8, device=c.device)
        m8[:n_ctx].copy_(_mask_bytes(ctx_mask))
        if Nc_pad != n_ctx:
            Cb[n_ctx:].zero_()
        inv_T = 1.0 / float(temperature)
        S = kn.sim(Qb, Cb, m8, inv_T)
        row_loss, _, G = kn.softmax_ce(S, pos_idx, 0, inv_T / B, want_G=True, row_win_start=pos_idx, win_len=K)
        loss = kn.reduce_sum(row_loss, 1.0 / B).reshape(())
        ctx.kn, ctx.n_ctx, ctx.in_dtypes = kn, n_ctx, (q.dtype, c.dtype)
        ctx.save_for_backward(Qb, Cb, G)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        Qb, Cb, G = ctx.saved_tensors
        go = grad_out.detach().reshape(1).float().contiguous()
        dQ, dC = ctx.kn.inbatch_bwd(G, Qb, Cb, 1.0, go, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        dq = dQ.to(ctx.in_dtypes[0]) if dQ is not None else None
        dc = dC[:ctx.n_ctx].to(ctx.in_dtypes[1]) if dC is not None else None
        return dq, dc, None, None, None, None


def windowed_contrastive_loss(q, c, pos_idx, ctx_mask, temperature=1.0, kernels=None):
    q, c = _pad_hidden(q, c)
    return WindowedContrastive.apply(q, c, pos_idx, ctx_mask, temperature, kernels)


# ---- scoring helpers used by the task's eval path and by subclasses that train through sim_score ----------------
def _sim_fwd(kn, q, c, colmask, inv_T):
    """(S, Qb, Cb, Nc) -- fp32 logits [Nq, Nc_pad] and the bf16 operand images (the backward of SimScore re-uses them)."""
    Nc = c.shape[0]
    Nc_pad = _pad_cols(Nc)
    Qb = kn.empty(tuple(q.shape), _BF16, q)
    kn.cast_bf16(q, Qb)
    Cb = kn.empty((Nc_pad, c.shape[1]), _BF16, c)
    kn.cast_bf16(c, Cb[:Nc])
    m8 = None
    if colmask is not None or Nc_pad != Nc:
        m8 = torch.zeros(Nc_pad, dtype=torch.uint8, device=c.device)
        if colmask is not None:
            m8[:Nc].copy_(_mask_bytes(colmask))
        if Nc_pad != Nc:
            Cb[Nc:].zero_()
            m8[Nc:] = 1
    return kn.sim(Qb, Cb, m8, inv_T), Qb, Cb, Nc


class SimScore(torch.autograd.Function):
    """scores = sim_score(q, c, colmask) * inv_T with gradients (dpr_task.py:98-105 is a differentiable torch.matmul):
    backward dq = inv_T * dS x C, dc = inv_T * dS^T x Q on the HIP backward GEMMs.  The incoming dS is rounded to bf16 for the
    MFMA operands, exactly like the dScores of the fused training step; masked columns receive no gradient (the reference's
    index-put leaves them out of the graph as well)."""

    @staticmethod
    def forward(ctx, q, c, colmask, inv_T, kernels):
        kn = kernels if kernels is not None else default_kernels()
        S, Qb, Cb, Nc = _sim_fwd(kn, q.detach(), c.detach(), colmask, inv_T)
        ctx.kn, ctx.Nc, ctx.inv_T, ctx.in_dtypes = kn, Nc, float(inv_T), (q.dtype, c.dtype)
        ctx.save_for_backward(Qb, Cb, colmask)
        return S if S.shape[1] == Nc else S[:, :Nc]

    @staticmethod
    def backward(ctx, dS):
        Qb, Cb, colmask = ctx.saved_tensors
        kn, Nc = ctx.kn, ctx.Nc
        G = kn.empty((dS.shape[0], Cb.shape[0]), _BF16, dS)
        if Cb.shape[0] != Nc:
            G[:, Nc:].zero_()
        g = dS.detach().float()
        if colmask is not None:
            g = g.masked_fill(colmask.bool()[None, :], 0.0)
        G[:, :Nc].copy_(g)
        dq = dc = None
        if ctx.needs_input_grad[0]:
            dq = kn.dq(G, Cb, ctx.inv_T).to(ctx.in_dtypes[0])
        if ctx.needs_input_grad[1]:
            dc = kn.dc(G, Qb, ctx.inv_T)[:Nc].to(ctx.in_dtypes[1])
        return dq, dc, None, None, None


def sim_score(q, c, colmask=None, inv_T=1.0, kernels=None):
    """dpr_task.py:98-105 on the device: fp32 logits [Nq, Nc] from fp32/bf16 embeddings; colmask is the [Nc]
    dummy-context mask (the row the reference broadcasts at :197).  Differentiable when an input requires grad."""
    kn = kernels if kernels is not None else default_kernels()
    q, c = _pad_hidden(q, c)
    if torch.is_grad_enabled() and (q.requires_grad or c.requires_grad):
        if not hasattr(kn, "dq"):
            raise RuntimeError(f"sim_score: an input requires grad but the kernels object {getattr(kn, 'name', kn)!r} has no backward "
                               "GEMMs (dq / dc); scores without a grad_fn would silently train nothing")
        return SimScore.apply(q, c, colmask, inv_T, kn)
    S, _, _, Nc = _sim_fwd(kn, q.detach(), c.detach(), colmask, inv_T)
    return S if S.shape[1] == Nc else S[:, :Nc]


class PairwiseScore(torch.autograd.Function):
    """citadel_task.py:137-146 `sim_score(q, c, mask, pairwise=True)`: scores[b][j] = <q[b], c[b*M + j]>, -inf at masked
    pairs; differentiable (HBM-streaming HIP kernels, fp32)."""

    @staticmethod
    def forward(ctx, q, c, mask, kernels):
        kn = kernels if kernels is not None else default_kernels()
        qf, cf = q.detach().float().contiguous(), c.detach().float().contiguous()
        m8 = None if mask is None else _mask_u8(mask).contiguous().view(-1)
        ctx.kn, ctx.in_dtypes = kn, (q.dtype, c.dtype)
        ctx.save_for_backward(qf, cf, m8)
        return kn.pairwise_fwd(qf, cf, m8)

    @staticmethod
    def backward(ctx, dS):
        qf, cf, m8 = ctx.saved_tensors
        g = dS.detach().float()
        if m8 is not None:
            g = g.masked_fill(m8.view_as(g).bool(), 0.0)  # -inf entries were index-put: no gradient flows through them
        dq, dc = ctx.kn.pairwise_bwd(g.contiguous(), qf, cf, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (dq.to(ctx.in_dtypes[0]) if dq is not None else None, dc.to(ctx.in_dtypes[1]) if dc is not None else None, None, None)


def pairwise_score(q, c, mask=None, kernels=None):
    """[B, M] scores of every query against its own M = c.shape[0] // B contexts (mask: [B*M] or [B, M] bool)."""
    return PairwiseScore.apply(q, c, mask, kernels)


def cross_entropy_mean(S, labels, kernels=None):
    """nn.CrossEntropyLoss()(S, labels) for existing fp32 logits (eval: dpr_task.py:224,299)."""
    kn = kernels if kernels is not None else default_kernels()
    S = S.contiguous()
    if S.shape[1] % 8 != 0:
        pad = _pad_cols(S.shape[1]) - S.shape[1]
        S = torch.nn.functional.pad(S, (0, pad), value=float("-inf"))
    row_loss, _, _ = kn.softmax_ce(S, labels)
    return kn.reduce_sum(row_loss, 1.0 / S.shape[0]).reshape(())


def rank_of_gold(S, labels, kernels=None):
    kn = kernels if kernels is not None else default_kernels()
    S = S.contiguous()
    if S.shape[1] % 4 != 0:
        S = torch.nn.functional.pad(S, (0, 4 - S.shape[1] % 4), value=float("-inf"))
    return kn.rank_of_gold(S, labels)


def rank_and_loss(q, c, labels, colmask=None, inv_T=1.0, kernels=None):
    """(ranks [Nq] int64, mean cross-entropy) of scores = q x c^T * inv_T with masked columns at -inf -- what
    compute_rank_metrics + self.loss (dpr_task.py:235-246,:299) derive from the score matrix, here without ever storing it
    when the problem is large (validation over a whole epoch's embeddings: 8192 x 65536 logits would be 2 GiB)."""
    kn = kernels if kernels is not None else default_kernels()
    q, c = _pad_hidden(q.detach(), c.detach())  # hidden sizes that are not a multiple of 8 (tiny encoders, projection heads)
    Nc = c.shape[0]
    Nc_pad = _pad_cols(Nc)
    Qb = kn.empty(tuple(q.shape), _BF16, q)
    kn.cast_bf16(q, Qb)
    Cb = kn.empty((Nc_pad, c.shape[1]), _BF16, c)
    kn.cast_bf16(c, Cb[:Nc])
    m8 = torch.zeros(Nc_pad, dtype=torch.uint8, device=c.device)
    if colmask is not None:
        m8[:Nc].copy_(_mask_bytes(colmask))
    if Nc_pad != Nc:
        Cb[Nc:].zero_()
        m8[Nc:] = 1
    y = torch.as_tensor(labels, dtype=torch.long, device=q.device)
    ranks, loss_sum = kn.sim_rank_loss(Qb, Cb, y, m8, inv_T)  # ONE pass of the Nq x Nc GEMM: count and softmax statistics in the same epilogue
    return ranks, (loss_sum / q.shape[0]).reshape(())


def topk(S, k, kernels=None):
    kn = kernels if kernels is not None else default_kernels()
    return kn.topk(S.contiguous(), k)


class CorpusSearch:
    """search_index of run_retrieval_pytorch.py:141-166 plus its shard loop (:196-243) and re-merge (:272-277):

        s = CorpusSearch(query_embs, topk)      # [nq, d] fp32/bf16 on the GPU
        for shard, first_id in shards:          # each [n, d] corpus shard resident on the GPU, any n
            s.add(shard, first_id)
        scores, ids = s.result()                # [nq, topk] fp32 / int64, best first, ties by lower id

    The [nq, n] score matrix never exists: each `chunk` of passages is scored on the bf16 MFMA path and folded
    into the running top-k on the device (dprhot_search)."""

    KMAX = 1024   # largest k of dprhot_search (GEMM with the filter epilogue); run_retrieval_pytorch.py:149 accepts any --topk
    KWIDE = TOPK_KWIDE

    def __init__(self, query_embs, k, chunk=None, kernels=None):
        self.kn = kernels if kernels is not None else default_kernels()
        nq, d = query_embs.shape
        self.Qb = self.kn.empty((nq, d), _BF16, query_embs)
        self.kn.cast_bf16(query_embs, self.Qb)
        self.k = int(k)
        self.wide_k = self.k > self.KMAX
        if chunk is None:  # filtered chunks of up to 262144 passages (2 GiB of candidate workspace at 1024 queries); the library starts
            chunk = max(1024, min(262144, (1 << 28) // max(nq, 1) // 8 * 8))  # an empty state from a 65536-passage head on its own
        self.chunk = int(chunk) // 8 * 8
        self.values = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=query_embs.device)
        self.indices = torch.full((nq, k), -1, dtype=torch.int64, device=query_embs.device)
        self.ws = None if self.wide_k else self.kn.search_workspace(nq, self.chunk, query_embs)
        self.wide_ws = None
        self.first = True

    def _add_chunks(self, Cb, first_id, fold):
        """k beyond 1024: the scores of a chunk come from the MFMA path (dprhot_sim_fwd) and fold(S, cols, col_offset) takes them into
        the running top-k -- no torch sort, no host sync per chunk.  Chunks of 65536 passages: a chunk's score matrix is nq x 256 KiB."""
        n, d = Cb.shape
        step = min(self.chunk, 65536)
        for j0 in range(0, n, step):
            cols = min(step, n - j0)
            pad = (-cols) % 8
            blk = Cb[j0:j0 + cols]
            if pad:
                blk = torch.cat([blk, torch.zeros((pad, d), dtype=_BF16, device=Cb.device)], 0)
            fold(self.kn.sim(self.Qb, blk.contiguous(), None, 1.0), cols, first_id + j0)
            self.first = False

    def _fold_native(self, S, cols, col_offset):
        """1024 < k <= 4096: the streaming kernel's wide instantiation (dprhot_topk_update: radix select from an empty state, then a
        threshold filter + bitonic merges in LDS)."""
        self.kn.topk_update(S, cols, col_offset, self.values, self.indices, self.first)

    def _fold_wide(self, S, cols, col_offset):
        """k beyond 4096: the library's HBM-resident selection (dprhot_topk_update_wide, csrc/wideselect.h: exact radix select over
        state + chunk, ties at the k-th score resolved by passage id, then only the k winners are sorted)."""
        if self.wide_ws is None:
            self.wide_ws = self.kn.topk_wide_workspace(self.values.shape[0], self.k, S)
        self.kn.topk_update_wide(S, cols, col_offset, self.values, self.indices, self.first, self.wide_ws)

    def add(self, corpus_embs, first_id=0):
        n, d = corpus_embs.shape
        if corpus_embs.dtype == _BF16 and corpus_embs.is_contiguous():
            Cb = corpus_embs
        else:
            Cb = self.kn.empty((n, d), _BF16, corpus_embs)
            self.kn.cast_bf16(corpus_embs, Cb)
        if self.wide_k:
            return self._add_chunks(Cb, first_id, self._fold_native if self.k <= self.KWIDE else self._fold_wide)
        n8 = n // 8 * 8
        if n8:
            self.kn.search(self.Qb, Cb[:n8], first_id, self.values, self.indices, self.first, self.chunk, self.ws)
            self.first = False
        if n8 != n:  # ragged tail: 8 padded rows, only the real columns are scanned
            tail = torch.zeros((8, d), dtype=_BF16, device=Cb.device)
            tail[: n - n8].copy_(Cb[n8:])
            S = self.kn.sim(self.Qb, tail, None, 1.0)
            self.kn.topk_update(S, n - n8, first_id + n8, self.values, self.indices, self.first)
            self.first = False

    def result(self):
        if self.wide_ws is not None:
            err = self.kn.topk_wide_errors(self.wide_ws, self.values.shape[0])
            if bool(err.any()):  # (one sync, where the caller is about to read the result anyway; no condition sets the word today)
                raise RuntimeError("dprhot_topk_update_wide reported rows it could not update: " + str(torch.nonzero(err).flatten().tolist()[:8]))
        return self.values, self.indices


# ---- late-interaction expert scoring (citadel_task.py:155-238) ------------------------------------------------------------------
_POOL = {"sum": 0, "max": 1}
MAXSIM_MAX_SLOTS = 8


class MaxSimScore(torch.autograd.Function):
    """MultiVecRetrieverTask.expert_sim_score (citadel_task.py:215-238) without the token-level score tensor: the token GEMM with a
    running max / argmax per query slot (HIP, bf16 MFMA, fp32 accumulation), pooled to [Nq, Nc] (or [B, M] pairwise); the backward
    works from the argmax tables alone.  Gradients flow to both token tensors and, when they require it, to both weight tensors."""

    @staticmethod
    def forward(ctx, q, c, qw, cw, qids, cids, m8, KQ, KD, pool, M, kernels):
        kn = kernels if kernels is not None else default_kernels()
        d = q.shape[-1]
        pad = (-d) % 32
        Qb = torch.nn.functional.pad(q.detach(), (0, pad)).to(_BF16).contiguous()
        Cb = torch.nn.functional.pad(c.detach(), (0, pad)).to(_BF16).contiguous()
        qwf = None if qw is None else qw.detach().float().contiguous()
        cwf = None if cw is None else cw.detach().float().contiguous()
        S, state = kn.maxsim_fwd(Qb, Cb, qids, cids, qwf, cwf, KQ, KD, pool, M, m8)
        ctx.kn, ctx.meta = kn, (d, KQ, KD, pool, M, q.dtype, c.dtype, None if qw is None else (qw.shape, qw.dtype),
                                None if cw is None else (cw.shape, cw.dtype))
        ctx.save_for_backward(Qb, Cb, qwf, cwf, qids, cids, m8, state)
        return S

    @staticmethod
    def backward(ctx, dS):
        Qb, Cb, qwf, cwf, qids, cids, m8, state = ctx.saved_tensors
        d, KQ, KD, pool, M, qdt, cdt, qws, cws = ctx.meta
        need_dw = qwf is not None and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
        dq, dc, dwq, dwc = ctx.kn.maxsim_bwd(dS.detach().float().contiguous(), Qb, Cb, qids, cids, qwf, cwf, KQ, KD, pool, M, m8, state,
                                             ctx.needs_input_grad[0], ctx.needs_input_grad[1], need_dw)
        gq = dq[..., :d].to(qdt) if dq is not None else None
        gc = dc[..., :d].to(cdt) if dc is not None else None
        gqw = dwq.reshape(qws[0]).to(qws[1]) if dwq is not None and ctx.needs_input_grad[2] else None
        gcw = dwc.reshape(cws[0]).to(cws[1]) if dwc is not None and ctx.needs_input_grad[3] else None
        return gq, gc, gqw, gcw, None, None, None, None, None, None, None, None


def _slots(ids, name):
    k = 1 if ids.dim() == 2 else ids.shape[2]
    if not 1 <= k <= MAXSIM_MAX_SLOTS:
        raise ValueError(f"{name}: {k} expert slots per token; the fused expert score supports 1..{MAXSIM_MAX_SLOTS}")
    return k


def expert_sim_score(query_repr, context_repr, mask=None, pairwise=False, query_pool="sum", kernels=None):
    """citadel_task.py:215-238 on the repr dicts of ColBERT (expert_repr), COIL (+ expert_ids [B, L], expert_weights [B, L]) and CITADEL
    (+ expert_ids [B, L, K], expert_weights [B, L, K]).  Returns [Nq, Nc] (or [B, M] with pairwise=True), -inf at masked contexts."""
    if query_pool not in _POOL:
        raise NotImplementedError("Invalid query pooling! Available: [max, sum]")
    q, c = query_repr["expert_repr"], context_repr["expert_repr"]
    B, Nc = q.shape[0], c.shape[0]
    M = Nc // B if pairwise else 0
    if pairwise and M * B != Nc:
        raise ValueError(f"pairwise expert score: {Nc} contexts is not a multiple of {B} queries")
    qids = cids = qw = cw = None
    KQ = KD = 1
    if "expert_ids" in query_repr:
        KQ, KD = _slots(query_repr["expert_ids"], "query expert_ids"), _slots(context_repr["expert_ids"], "context expert_ids")
        qids = query_repr["expert_ids"].to(torch.int32).contiguous()  # int64 -> int32 once
        cids = context_repr["expert_ids"].to(torch.int32).contiguous()
        if "expert_weights" in query_repr:
            qw, cw = query_repr["expert_weights"], context_repr["expert_weights"]
            if not qw.is_floating_point():  # COIL: the integer attention mask, no gradient
                qw, cw = qw.float(), cw.float()
    m8 = None
    if mask is not None:
        m8 = mask.reshape(-1).to(torch.uint8).contiguous()
        if m8.numel() != Nc:
            raise ValueError(f"expert score: mask of {m8.numel()} entries for {Nc} contexts")
    return MaxSimScore.apply(q, c, qw, cw, qids, cids, m8, KQ, KD, _POOL[query_pool], M, kernels)


def expert_score_only(query_repr, context_repr, mask=None, query_pool="sum", kernels=None):
    """expert_sim_score(..., pairwise=True) for inference: the same repr dicts, the same operands (features padded to 32 in bf16,
    int32 ids, fp32 weights) and the same bits, [B, M] with M = Nc // B, from one launch that keeps no tables (dprhot_maxsim_score).
    The result has no grad_fn and nothing is saved."""
    if query_pool not in _POOL:
        raise NotImplementedError("Invalid query pooling! Available: [max, sum]")
    kn = kernels if kernels is not None else default_kernels()
    q, c = query_repr["expert_repr"].detach(), context_repr["expert_repr"].detach()
    B, Nc = q.shape[0], c.shape[0]
    M = Nc // B
    if M * B != Nc:
        raise ValueError(f"pairwise expert score: {Nc} contexts is not a multiple of {B} queries")
    qids = cids = qw = cw = None
    KQ = KD = 1
    if "expert_ids" in query_repr:
        KQ, KD = _slots(query_repr["expert_ids"], "query expert_ids"), _slots(context_repr["expert_ids"], "context expert_ids")
        qids = query_repr["expert_ids"].to(torch.int32).contiguous()
        cids = context_repr["expert_ids"].to(torch.int32).contiguous()
        if "expert_weights" in query_repr:  # (COIL: the integer attention mask)
            qw = query_repr["expert_weights"].detach().float().contiguous()
            cw = context_repr["expert_weights"].detach().float().contiguous()
    m8 = None
    if mask is not None:
        m8 = mask.reshape(-1).to(torch.uint8).contiguous()
        if m8.numel() != Nc:
            raise ValueError(f"expert score: mask of {m8.numel()} entries for {Nc} contexts")
    return kn.maxsim_score(_bf16_rows(q), _bf16_rows(c), qids, cids, qw, cw, KQ, KD, _POOL[query_pool], M, m8)


def _bf16_rows(x):
    """The bf16 image of token rows, zero-padded to a multiple of 32 features, without a padded copy in the source dtype."""
    d = x.shape[-1]
    pad = (-d) % 32
    if not pad:
        return x.to(_BF16).contiguous()
    out = torch.zeros(x.shape[:-1] + (d + pad,), dtype=_BF16, device=x.device)
    out[..., :d].copy_(x)
    return out


def rerank_score(query_repr, context_repr, query_pool="sum", kernels=None):
    """RerankMultiVecRetrieverTask's score of B aligned (query, passage) pairs (citadel_eval_task.py:238-265, :281-283): [B], the
    expert score of pair b plus <q_cls[b], c_cls[b]> when the passages carry `cls_repr`."""
    B, Nc = query_repr["expert_repr"].shape[0], context_repr["expert_repr"].shape[0]
    if Nc != B:
        raise ValueError(f"rerank score: {Nc} passages for {B} queries; a rerank batch is aligned pairs")
    scores = expert_score_only(query_repr, context_repr, None, query_pool, kernels)[:, 0]
    if "cls_repr" in context_repr:
        with torch.no_grad():
            scores = scores + pairwise_score(query_repr["cls_repr"], context_repr["cls_repr"], None, kernels)[:, 0]
    return scores


# ---- the CITADEL / SPLADE encoder head (citadel_model.py:46-82, splade_model.py:26-32) ---------------------------------------------
ROUTER_HEAD_MAX_TOPK = 8


class RouterHead(torch.autograd.Function):
    """Everything CITADELEncoder.forward derives from the MLM logits, without a [B, T, V] temporary: the logits are streamed by the HIP
    kernels of csrc/router_head.h forward and backward; what is kept for the backward is [B, V] / [B, T, k] / [B, T] small."""

    @staticmethod
    def forward(ctx, logits, m8, k, skip, want_softmax, kernels):
        kn = kernels if kernels is not None else default_kernels()
        x = logits.detach()
        repr_, arg, w, ids, rmask, ssum, state = kn.router_head_fwd(x, m8, k, skip, want_softmax)
        ctx.kn, ctx.meta = kn, (k, skip)
        ctx.save_for_backward(x, m8, arg, ids, state)
        ctx.set_materialize_grads(False)
        outs = (repr_, w, ssum, ids, rmask)
        ctx.mark_non_differentiable(*[o for o in (ids, rmask) if o is not None])
        return outs

    @staticmethod
    def backward(ctx, g_repr, g_w, g_soft, _g_ids, _g_mask):
        x, m8, arg, ids, state = ctx.saved_tensors
        k, skip = ctx.meta
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        g = [None if t is None else t.detach().float().contiguous() for t in (g_repr, g_w, g_soft)]
        dx = ctx.kn.router_head_bwd(x, m8, k, skip, arg, ids, state, g[0], g[1] if k else None, g[2])
        return dx, None, None, None, None, None


def router_head(logits, attention_mask, topk=1, skip_first=1, want_softmax=True, kernels=None):
    """The head of CITADELEncoder.forward (citadel_model.py:50-82) / SPLADEEncoder.forward (splade_model.py:29-32, topk = 0) from the MLM
    logits [B, T1, V] (fp32, bf16 or fp16 on a HIP device; a view with unit column stride is read in place) and attention_mask [B, T1]
    (non-zero = a real token); the first `skip_first` token rows take no part.  Returns a dict with the reference's keys -- router_repr
    [B, V], expert_ids int64 [B, T, k], expert_weights [B, T, k], router_mask [B, V], router_softmax_repr [B, V], avg_cond_num_experts
    and avg_marg_num_experts [1, 1] -- float values in the logits' dtype; topk = 0 leaves the routing keys out, want_softmax = False
    router_softmax_repr.  router_repr, expert_weights and router_softmax_repr are differentiable.  Ties: top-k by value descending then
    vocabulary index ascending, zeros included; the max over tokens keeps the lowest token."""
    if logits.dim() != 3 or attention_mask.dim() != 2 or attention_mask.shape != logits.shape[:2]:
        raise ValueError(f"router_head: logits {tuple(logits.shape)} / attention_mask {tuple(attention_mask.shape)}: want [B, T1, V] and [B, T1]")
    HipKernels._require_gpu(logits, attention_mask)
    if logits.dtype not in _RH_DTYPE:
        raise TypeError(f"router_head: logits of {logits.dtype}; fp32, bf16 and fp16 are supported")
    k, skip = int(topk), int(skip_first)
    if not 0 <= k <= ROUTER_HEAD_MAX_TOPK:
        raise ValueError(f"router_head: topk={k}; the fused head supports 0..{ROUTER_HEAD_MAX_TOPK}")
    if logits.stride(2) != 1 or logits.stride(1) < logits.shape[2]:
        logits = logits.contiguous()
    m8 = (attention_mask != 0).to(torch.uint8).contiguous()
    repr_, w, ssum, ids, rmask = RouterHead.apply(logits, m8, k, skip, bool(want_softmax), kernels)
    ret = {"router_repr": repr_}
    if k:
        ret["expert_ids"] = ids.long()
        ret["expert_weights"] = w
        ret["router_mask"] = rmask
        ret["avg_cond_num_experts"] = rmask.sum(1, keepdim=True).mean(0, keepdim=True)         # citadel_model.py:66
        ret["avg_marg_num_experts"] = rmask.max(0, keepdim=True).values.sum(1, keepdim=True)   # :68
    if want_softmax:
        ret["router_softmax_repr"] = ssum
    return ret
