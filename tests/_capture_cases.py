"""The capture / side-stream conformance table: one or more rows per entry point of include/dprhot.h that takes a `void* stream`.

A row (`Case`) names the C symbols it exercises and a builder.  The builder returns a `Built`:
    A, B    two input sets of the same shapes and dtypes (device tensors).  B differs from A in the device-resident STRUCTURE, not only in
            values -- other labels and masks, other candidate lists (an empty one, one that grows), other block offsets, other expert
            offsets and centroid ids, NaN cells in other places -- so that a loop bound read from device memory shows when a replay
            does not read it again.
    fn(x)   the call or calls, on the CURRENT torch stream, reading the static input buffers `x` (the harness copies A or B into them
            in place).  Returns the outputs it allocated itself (HipKernels methods do); None entries are dropped.
    outs    caller-owned outputs, sentinel-filled before every run.
    ws      caller-owned workspaces, or a callable returning the cached ones (HipKernels._workspace, per stream).
    after   optional check on the buffers after a replay (the wide selection's error record).

Entry points are driven the way the product drives them: through the HipKernels method where one exists, through ctypes where the
method reads results back to the host (ivf_compact) or where there is none.  Every library call goes through ONE recording proxy around
_lib.lib, so that the symbols a row declares can be held against the symbols its fn() really called.

Inputs come from the builders the conformance suites already have (_search_cases, _ivf_fixture, _ivf_cases, _spar_oracle, _fp8_oracle,
_rowwise_cases, _topk_oracle, _multivec_oracle, _router_head_oracle, _ivf_pack_inputs and the `corpus` / `lists` helpers of the ColBERT
GPU tests); index tensors are CLONED before anything is copied into them: the shared fixtures stay as they are.  No oracle is needed
here: the reference of a replay is the eager call on the default stream, which those suites hold to their oracles."""
import ctypes
import types
from typing import Callable, NamedTuple

import numpy as np
import torch

DEV = "cuda:0"
BF16 = torch.bfloat16
SENTINEL, SCRIBBLE = 0xA5, 0x3C

# The six RCCL collectives: no capture next to a live communicator (a captured collective replays on every rank or hangs all of them),
# and a one-process test has no peer to run them with.  Everything else that takes a stream is covered by a row below.
EXCLUDED = {
    "dprhot_allgather_ctx": "RCCL collective: no capture next to a live communicator",
    "dprhot_reducescatter_dc": "RCCL collective: no capture next to a live communicator",
    "dprhot_reducescatter_rows": "RCCL collective: no capture next to a live communicator",
    "dprhot_allreduce_sum": "RCCL collective: no capture next to a live communicator",
    "dprhot_allgather_allpairs": "RCCL collective: no capture next to a live communicator",
    "dprhot_reducescatter_allpairs": "RCCL collective: no capture next to a live communicator",
}

# shapes of tests/test_step_refusals.py, and the smallest one-pass and no-logits shapes of tests/test_bounds_cpu.py's PLAN_TABLE
SMALL, FEW, GEN = (8, 16, 64), (32, 1032, 128), (64, 512, 64)
ONEPASS = (160, 2048, 768)   # dprhot_fwd_one_pass == 2 ("sk_plan rows", outside)
NOLOG = (1024, 8192, 768)    # dprhot_fwd_no_logits == 1 ("nl_ok tiles", inside)
P_SMALL, P_FEW = (8, 2, 8, 64), (32, 2, 512, 128)  # (B, W, n_ctx, d) of the packed step
INV_T = 2.0


class Case(NamedTuple):
    name: str
    symbols: tuple
    build: Callable


class Built:
    def __init__(self, A, B, fn, outs=(), ws=(), after=None):
        assert len(A) == len(B) and all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(A, B)), "A and B: the same shapes"
        self.A, self.B, self.fn, self.outs, self.ws, self.after = list(A), list(B), fn, list(outs), ws, after


CASES = []


def case(name, *symbols):
    def reg(build):
        assert all(s.startswith("dprhot_") for s in symbols) and name not in [c.name for c in CASES]
        CASES.append(Case(name, tuple(symbols), build))
        return build
    return reg


# ---- the recording proxy and the one kernel set ------------------------------------------------------------------------------------
class Recorder:
    """_lib.lib with a note of every dprhot_* symbol called through it."""

    def __init__(self, lib):
        self._lib, self.called = lib, set()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dprhot_"):
            return fn

        def call(*args):
            self.called.add(name)
            return fn(*args)
        return call


_KN = None


def kernels():
    """(HipKernels whose library handle is the recording proxy, the proxy, _lib)."""
    global _KN
    if _KN is None:
        from dpr_scale_amd import _lib
        from dpr_scale_amd.hotpath import HipKernels

        kn = HipKernels()
        kn.lib = Recorder(_lib.lib)
        _KN = (kn, kn.lib, _lib)
    return _KN


def _call(name, *args):
    """One entry point through ctypes (and the proxy): tensors go as their addresses, None as NULL, the stream is the current one."""
    kn, L, _lib = kernels()
    argv = [ctypes.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args]
    _lib.check(getattr(L, name)(*argv, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def dv(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    t = t.to(DEV)
    return (t if dtype is None else t.to(dtype)).contiguous()


def empty(shape, dtype):
    return torch.empty(shape, dtype=dtype, device=DEV)


def step_ws(x):
    """The cached step workspace of the current stream (what the HipKernels methods of the training step hand to the library)."""
    return lambda: [kernels()[0]._workspace(x[0].device, 1)]


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _shift_offsets(off):
    """Other non-decreasing offsets with the same ends: every inner boundary one further (the first range grows, the last shrinks)."""
    out = off.clone()
    out[1:-1] = torch.clamp(off[1:-1] + 1, max=int(off[-1]))
    return out


# ---- the training step family --------------------------------------------------------------------------------------------------------
def _step_data(shape, seed):
    """(q, c fp32, y int64 distinct gold columns, mask uint8 over an eighth of the other columns) of a (B, Nc, d) step."""
    B, Nc, d = shape
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, d, generator=g) * d ** -0.25
    c = torch.randn(Nc, d, generator=g) * d ** -0.25
    perm = torch.randperm(Nc, generator=g)
    y = perm[:B].clone()
    mask = torch.zeros(Nc, dtype=torch.uint8)
    mask[perm[B:B + max(1, (Nc - B) // 8)]] = 1
    return dv(q), dv(c), dv(y), dv(mask)


def _tag(shape):
    return "x".join(str(s) for s in shape)


def _gs(shape):
    return INV_T / shape[0]


for _shape in (SMALL, FEW, GEN, ONEPASS, NOLOG):
    def _fwd(shape=_shape):
        kn = kernels()[0]
        (qa, ca, ya, ma), (qb, cb, yb, mb) = _step_data(shape, 11), _step_data(shape, 12)
        A, B = [qa.to(BF16), ca.to(BF16), ya, ma], [qb.to(BF16), cb.to(BF16), yb, mb]
        x0 = A
        return Built(A, B, lambda x: kn.inbatch_fwd(x[0], x[1], x[2], 0, x[3], INV_T, _gs(shape)), ws=step_ws(x0))

    case(f"inbatch_fwd-{_tag(_shape)}", "dprhot_inbatch_fwd")(_fwd)

    def _fwd32(shape=_shape):
        kn = kernels()[0]
        A, B = list(_step_data(shape, 13)), list(_step_data(shape, 14))
        Qb, Cb = empty((shape[0], shape[2]), BF16), empty((shape[1], shape[2]), BF16)
        return Built(A, B, lambda x: kn.inbatch_fwd_f32(x[0], x[1], Qb, Cb, x[2], 0, x[3], INV_T, _gs(shape)), outs=[Qb, Cb], ws=step_ws(A))

    case(f"inbatch_fwd_f32-{_tag(_shape)}", "dprhot_inbatch_fwd_f32")(_fwd32)

    def _train(shape=_shape, double=False):
        """The operator's two calls: dprhot_train_step_f32 with the slabs deferred, then dprhot_rescale_grads.  `double`: the engine
        delivers twice the scale the step expected (the rescale pass runs); else the same scale (its workgroups read two floats)."""
        kn = kernels()[0]
        f = 2.0 if double else 1.0
        A = list(_step_data(shape, 15)) + [dv(torch.tensor([1.0])), dv(torch.tensor([1.0 * f]))]
        B = list(_step_data(shape, 16)) + [dv(torch.tensor([4.0])), dv(torch.tensor([4.0 * f]))]
        Qb, Cb = empty((shape[0], shape[2]), BF16), empty((shape[1], shape[2]), BF16)

        def fn(x):
            _, lse, loss, G, dQs, dC = kn.train_step_f32(x[0], x[1], Qb, Cb, x[2], 0, x[3], INV_T, _gs(shape), 1.0 / shape[0], x[4], defer_dq=True,
                                                         want_G="auto")
            out2 = kn.rescale_grads(dQs, dC, x[5], x[4])
            return (lse, loss[:1], G, dC, out2) + (dQs if isinstance(dQs, tuple) else (dQs,))  # (loss_out[0] is the loss)

        return Built(A, B, fn, outs=[Qb, Cb], ws=step_ws(A))

    case(f"train_step_f32-{_tag(_shape)}", "dprhot_train_step_f32", "dprhot_rescale_grads")(_train)
    if _shape == FEW:
        case(f"train_step_f32-{_tag(_shape)}-go2x", "dprhot_train_step_f32", "dprhot_rescale_grads")(
            lambda shape=_shape, build=_train: build(shape, True))

for _shape in (SMALL, FEW, GEN, ONEPASS):
    def _step(shape=_shape):
        kn = kernels()[0]
        A, B = list(_step_data(shape, 17)), list(_step_data(shape, 18))
        Qb, Cb = empty((shape[0], shape[2]), BF16), empty((shape[1], shape[2]), BF16)
        return Built(A, B, lambda x: kn.inbatch_step_f32(x[0], x[1], Qb, Cb, x[2], 0, x[3], INV_T, _gs(shape)), outs=[Qb, Cb], ws=step_ws(A))

    case(f"inbatch_step_f32-{_tag(_shape)}", "dprhot_inbatch_step_f32")(_step)

for _shape in (SMALL, FEW, GEN):
    def _bwd(shape=_shape):
        """The three backward entry points from given dScores and a device scale."""
        kn = kernels()[0]
        B_, Nc, d = shape

        def data(seed, scale):
            q, c, _, _ = _step_data(shape, seed)
            G = torch.randn(B_, Nc, generator=torch.Generator().manual_seed(seed)) / Nc
            return [dv(G, BF16), q.to(BF16), c.to(BF16), dv(torch.tensor([scale]))]

        A, B = data(19, 1.0), data(20, -0.5)

        def fn(x):
            dQ, dC = kn.inbatch_bwd(x[0], x[1], x[2], 1.0, x[3])
            return dQ, dC, kn.dq(x[0], x[2], 1.0, x[3]), kn.dc(x[0], x[1], 1.0, x[3])

        return Built(A, B, fn, ws=step_ws(A))

    case(f"inbatch_bwd-{_tag(_shape)}", "dprhot_inbatch_bwd", "dprhot_dq", "dprhot_dc")(_bwd)

for _shape, _f32 in ((SMALL, False), (FEW, False), (GEN, False), (NOLOG, False), (SMALL, True), (FEW, True), (GEN, True)):
    def _launches(shape=_shape, f32=_f32):
        """The forward's launches one by one: dprhot_sim_stats (or _f32), dprhot_softmax_finish and, where the logits are never stored,
        dprhot_dscores -- all through ctypes on a caller-owned workspace."""
        _, _, _lib = kernels()
        B_, Nc, d = shape
        nl = _lib.fwd_no_logits(*shape)
        A, B = list(_step_data(shape, 21)), list(_step_data(shape, 22))
        if not f32:
            A, B = [A[0].to(BF16), A[1].to(BF16)] + A[2:], [B[0].to(BF16), B[1].to(BF16)] + B[2:]
        wsb = _lib.workspace_bytes(*shape)
        ws = empty(wsb, torch.uint8)
        row_loss, row_lse, loss = empty(B_, torch.float32), empty(B_, torch.float32), empty(1, torch.float32)
        G = empty((B_, Nc), BF16)
        Qb, Cb = empty((B_, d), BF16), empty((Nc, d), BF16)
        gs = _gs(shape)

        def fn(x):
            if f32:
                _call("dprhot_sim_stats_f32", x[0], x[1], Qb, Cb, B_, Nc, d, x[2], 0, x[3], INV_T, None, ws, wsb)
            else:
                _call("dprhot_sim_stats", x[0], B_, x[1], Nc, d, x[2], 0, x[3], INV_T, None, ws, wsb)
            _call("dprhot_softmax_finish", None, B_, Nc, d, x[2], 0, gs, row_loss, row_lse, loss, None if nl else G, ws, wsb)
            if nl:
                _call("dprhot_dscores", x[0], B_, x[1], Nc, d, x[2], 0, x[3], INV_T, gs, None, G, ws, wsb)
            return ()

        return Built(A, B, fn, outs=[row_loss, row_lse, loss, G] + ([Qb, Cb] if f32 else []), ws=[ws])

    _syms = ("dprhot_sim_stats_f32" if _f32 else "dprhot_sim_stats", "dprhot_softmax_finish") + (("dprhot_dscores",) if _shape == NOLOG else ())
    case(f"{'sim_stats_f32' if _f32 else 'sim_stats'}-{_tag(_shape)}", *_syms)(_launches)

for _shape in (GEN, NOLOG):
    def _rank(shape=_shape):
        kn = kernels()[0]
        (qa, ca, ya, ma), (qb, cb, yb, mb) = _step_data(shape, 23), _step_data(shape, 24)
        A, B = [qa.to(BF16), ca.to(BF16), ya, ma], [qb.to(BF16), cb.to(BF16), yb, mb]

        def fn(x):
            S = kn.sim(x[0], x[1], x[3], INV_T)
            return (S, kn.rank_of_gold(S, x[2]), kn.sim_rank(x[0], x[1], x[2], x[3], INV_T)) + kn.sim_rank_loss(x[0], x[1], x[2], x[3], INV_T)

        return Built(A, B, fn, ws=step_ws(A))

    case(f"sim_rank-{_tag(_shape)}", "dprhot_sim_fwd", "dprhot_rank_of_gold", "dprhot_sim_rank", "dprhot_sim_rank_loss")(_rank)


def _packed_data(shape, seed):
    """(q [B, d], c [W, n_ctx, d] fp32, m8 [W, n_ctx] with dummies on both ranks, y [B] among rank 1's real contexts) of a packed step."""
    B_, W, n_ctx, d = shape
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B_, d, generator=g) * d ** -0.25
    c = torch.randn(W, n_ctx, d, generator=g) * d ** -0.25
    m8 = torch.zeros(W, n_ctx, dtype=torch.uint8)
    real = []
    for r in range(W):
        perm = torch.randperm(n_ctx, generator=g)
        m8[r, perm[: n_ctx // 8]] = 1
        real.append(perm[n_ctx // 8:])
    y = real[1][torch.randint(0, real[1].numel(), (B_,), generator=g)].clone()
    return [dv(q), dv(c), dv(m8), dv(y)]


for _shape, _train_step in ((P_SMALL, False), (P_FEW, False), (P_SMALL, True), (P_FEW, True)):
    def _packed(shape=_shape, train=_train_step):
        """What a rank does between the all-gather and the reduce-scatter, the gather replaced by dprhot_pack_ctx of every rank's rows
        into its slot: pack, unpack_mask (the column mask the unfused callers build), the packed step as rank 1; the operator's form
        with dprhot_rescale_grads behind it, its dC partials in bf16 where the plan has that epilogue (the few-rows shape)."""
        kn, _, _lib = kernels()
        B_, W, n_ctx, d = shape
        rows_c = _lib.packed_rows(n_ctx, d)
        A, B = _packed_data(shape, 25), _packed_data(shape, 26)
        if train:
            A, B = A + [dv(torch.tensor([1.0])), dv(torch.tensor([1.0]))], B + [dv(torch.tensor([2.0])), dv(torch.tensor([0.5]))]
        gathered, colmask, Qb = empty((W * rows_c, d), BF16), empty(W * rows_c, torch.uint8), empty((B_, d), BF16)
        gs = INV_T / (W * B_)
        dc_dtype = BF16 if shape == P_FEW else torch.float32

        def fn(x):
            for r in range(W):
                kn.pack_ctx(x[1][r], x[2][r], gathered[r * rows_c:(r + 1) * rows_c])
            kn.unpack_mask(gathered, W, n_ctx, colmask)
            if not train:
                return kn.inbatch_step_packed_f32(x[0], gathered, Qb, W, 1, n_ctx, x[3], INV_T, gs)
            _, lse, loss, G, dQs, dC = kn.train_step_packed_f32(x[0], gathered, Qb, W, 1, n_ctx, x[3], INV_T, gs, 1.0 / (W * B_), x[4], dc_dtype,
                                                                defer_dq=True, want_G="auto")
            out2 = kn.rescale_grads(dQs, dC, x[5], x[4])
            return (lse, loss[:1], G, dC, out2) + (dQs if isinstance(dQs, tuple) else (dQs,))  # (loss_out[0] is the loss)

        return Built(A, B, fn, outs=[gathered, colmask, Qb], ws=step_ws(A))

    _syms = ("dprhot_pack_ctx", "dprhot_unpack_mask") + (("dprhot_train_step_packed_f32", "dprhot_rescale_grads") if _train_step
                                                         else ("dprhot_inbatch_step_packed_f32",))
    case(f"{'train_step' if _train_step else 'inbatch_step'}_packed_f32-{_tag(_shape)}", *_syms)(_packed)


# ---- row kernels, casts, the gradient legs ------------------------------------------------------------------------------------------
@case("casts", "dprhot_cast_bf16", "dprhot_prep", "dprhot_reduce_sum")
def _casts():
    kn = kernels()[0]
    g = torch.Generator().manual_seed(31)
    A = [dv(torch.randn(33, 72, generator=g)), dv(torch.randn(129, 72, generator=g))]
    B = [dv(torch.randn(33, 72, generator=g) * 1e-3), dv(torch.randn(129, 72, generator=g) * 1e3)]
    B[0][5, 7] = float("nan")
    one, Qb, Cb = empty((33, 72), BF16), empty((33, 72), BF16), empty((129, 72), BF16)

    def fn(x):
        kn.cast_bf16(x[0], one)
        kn.prep(x[0], Qb, x[1], Cb)
        return (kn.reduce_sum(x[1].view(-1)[:5000], 0.25),)

    return Built(A, B, fn, outs=[one, Qb, Cb])


def _rowwise(name_a, name_b):
    """Two cases of the row-kernel conformance table at one shape; B's rows, labels and windows are A's partner's, rolled by one row."""
    import _rowwise_cases as RW

    kn = kernels()[0]
    a, b = RW.TABLE[name_a](), RW.TABLE[name_b]()
    assert a.S.shape == b.S.shape and (a.y_offset, a.win_len, a.want_G) == (b.y_offset, b.win_len, b.want_G) and (a.win_start is None) == (b.win_start is None)
    roll = lambda v: np.roll(v, 1, axis=0)
    A = [dv(a.S), dv(a.y)] + ([dv(a.win_start)] if a.win_start is not None else [])
    B = [dv(roll(b.S)), dv(roll(b.y))] + ([dv(roll(b.win_start))] if b.win_start is not None else [])

    def fn(x):
        row_loss, row_lse, G = kn.softmax_ce(x[0], x[1], a.y_offset, a.gs, a.want_G, x[2] if len(x) > 2 else None, a.win_len)
        return row_loss, row_lse, G, kn.reduce_sum(row_loss, 1.0 / row_loss.numel())

    return Built(A, B, fn)


# NaN cells in other places (64 threads per row); a window per row with other starts and labels; 256 threads per row
case("softmax_ce-nan-1032", "dprhot_softmax_ce_fwd_bwd", "dprhot_reduce_sum")(lambda: _rowwise("N-nan_among_finite-1032", "N-nan_alone_after_finite-1032"))
case("softmax_ce-window-264", "dprhot_softmax_ce_fwd_bwd")(lambda: _rowwise("W-len13-264", "W-len13-off0-planted-264"))
case("softmax_ce-nan-8200", "dprhot_softmax_ce_fwd_bwd")(lambda: _rowwise("N-nan_among_finite-8200", "N-nan_in_empty_row-8200"))

for _wire, _dt in ((0, BF16), (1, torch.float16), (2, torch.float32)):
    def _legs(wire=_wire, dt=_dt):
        """The three local legs of the gradient hook for one bucket of n = 4096 * 33 + 5 values on W = 4 ranks: pack, the sum of the W
        received shards (here: the packed bucket's own four shards), unpack."""
        n, W = 4096 * 33 + 5, 4
        shard = (-(-n // W) + 7) // 8 * 8
        g = torch.Generator().manual_seed(40 + wire)
        A, B = [dv(torch.randn(n, generator=g))], [dv(torch.randn(n, generator=g) * 300.0)]
        B[0][17] = float("inf")
        send, out, back = empty(W * shard, dt), empty(shard, dt), empty(n, torch.float32)
        out32 = empty(shard, torch.float32)

        def fn(x):
            _call("dprhot_grad_pack", x[0], n, 0.5, wire, send, W * shard)
            _call("dprhot_grad_sum_shards", send, W, shard, wire, wire, out)
            _call("dprhot_grad_sum_shards", send, W, shard, wire, 2, out32)
            _call("dprhot_grad_unpack", send, wire, back, n)
            return ()

        return Built(A, B, fn, outs=[send, out, out32, back])

    case(f"grad_legs-wire{_wire}", "dprhot_grad_pack", "dprhot_grad_sum_shards", "dprhot_grad_unpack")(_legs)


# ---- pairwise, MaxSim, the router head ------------------------------------------------------------------------------------------------
@case("pairwise", "dprhot_pairwise_fwd", "dprhot_pairwise_bwd")
def _pairwise():
    kn = kernels()[0]
    Bq, M, d = 3, 4, 30522

    def data(seed):
        g = torch.Generator().manual_seed(seed)
        m8 = torch.zeros(Bq * M, dtype=torch.uint8)
        m8[torch.randperm(Bq * M, generator=g)[:3]] = 1
        gS = torch.randn(Bq, M, generator=g) * (1 - m8.view(Bq, M).float())
        return [dv(torch.randn(Bq, d, generator=g)), dv(torch.randn(Bq * M, d, generator=g)), dv(m8), dv(gS)]

    def fn(x):
        return (kn.pairwise_fwd(x[0], x[1], x[2]),) + kn.pairwise_bwd(x[3], x[0], x[1])

    return Built(data(51), data(52), fn)


@case("maxsim", "dprhot_maxsim_fwd", "dprhot_maxsim_bwd", "dprhot_maxsim_score")
def _maxsim():
    import _multivec_oracle as MV

    kn = kernels()[0]
    Nq, LQ, Nc, LD, d, KQ, KD = 3, 20, 12, 33, 96, 2, 3

    def data(seed, masked):
        qr, cr, mask = MV.make_inputs(seed, "citadel", Nq, LQ, Nc, LD, d, KQ=KQ, KD=KD, masked=masked)
        g = torch.Generator().manual_seed(seed)
        return [dv(qr["expert_repr"], BF16), dv(cr["expert_repr"], BF16), dv(qr["expert_ids"], torch.int32), dv(cr["expert_ids"], torch.int32),
                dv(qr["expert_weights"]), dv(cr["expert_weights"]), dv(mask, torch.uint8), dv(torch.randn(Nq, Nc, generator=g)),
                dv(torch.randn(Nq, Nc // Nq, generator=g))]

    def fn(x):
        outs = []
        for M, dS in ((0, x[7]), (Nc // Nq, x[8])):  # in-batch, then pairwise
            S, state = kn.maxsim_fwd(x[0], x[1], x[2], x[3], x[4], x[5], KQ, KD, 0, M, x[6])
            outs += [S, *kn.maxsim_bwd(dS, x[0], x[1], x[2], x[3], x[4], x[5], KQ, KD, 0, M, x[6], state, need_dw=True)]
        return outs + [kn.maxsim_score(x[0], x[1], x[2], x[3], x[4], x[5], KQ, KD, 1, Nc // Nq, x[6])]

    return Built(data(53, (2,)), data(54, (0, 7, 11)), fn)


for _rh in ((3, 6, 509, 3), (2, 4, 30522, 8)):
    def _router(rh=_rh):
        import _router_head_oracle as RO

        kn = kernels()[0]
        Bq, T1, V, k = rh

        def data(seed):
            rng = np.random.default_rng(seed)
            g = torch.Generator().manual_seed(seed)
            logits = RO.grid_logits(rng, Bq, T1, V)
            logits[0, 1, 5] = np.nan
            return [dv(logits), dv(RO.masks(rng, Bq, T1), torch.uint8), dv(torch.randn(Bq, V, generator=g)),
                    dv(torch.randn(Bq, T1 - 1, k, generator=g)), dv(torch.randn(Bq, V, generator=g))]

        def fn(x):
            repr_, arg, w, ids, rmask, ssum, state = kn.router_head_fwd(x[0], x[1], k, 1, True)
            return repr_, arg, w, ids, rmask, ssum, kn.router_head_bwd(x[0], x[1], k, 1, arg, ids, state, x[2], x[3], x[4])

        return Built(data(55), data(56), fn)

    case(f"router_head-{_tag(_rh)}", "dprhot_router_head_fwd", "dprhot_router_head_bwd")(_router)


# ---- the streaming top-k and the dense search -------------------------------------------------------------------------------------------
@case("topk", "dprhot_topk", "dprhot_topk_update")
def _topk():
    import _topk_oracle as TO

    kn = kernels()[0]
    rows, cols, k = 6, 1000, 100
    A, B = [dv(TO.adversarial(rows, cols, 61, "specials"))], [dv(TO.adversarial(rows, cols, 62, "nan_rows", k))]
    values, indices = empty((rows, k), torch.float32), empty((rows, k), torch.int64)

    def fn(x):
        kn.topk_update(x[0], 504, 0, values, indices, True)
        kn.topk_update(x[0][:, 504:], cols - 504, 504, values, indices, False)
        return kn.topk(x[0], k)

    return Built(A, B, fn, outs=[values, indices])


def _wide_clean(ws, rows):
    def check():
        assert not bool(kernels()[0].topk_wide_errors(ws, rows).any()), "the wide selection's error record is not clean"
    return check


@case("topk_update_wide-k5000", "dprhot_topk_update_wide")
def _topk_wide():
    import _topk_oracle as TO

    kn = kernels()[0]
    rows, cols, k = 6, 6000, 5000
    A, B = [dv(TO.adversarial(rows, cols, 63, "nan_rows", k))], [dv(TO.adversarial(rows, cols, 64, "specials"))]
    values, indices = empty((rows, k), torch.float32), empty((rows, k), torch.int64)
    ws = kn.topk_wide_workspace(rows, k, values)

    def fn(x):
        kn.topk_update_wide(x[0], 3000, 0, values, indices, True, ws)
        kn.topk_update_wide(x[0][:, 3000:], cols - 3000, 3000, values, indices, False, ws)
        return ()

    return Built(A, B, fn, outs=[values, indices], ws=[ws], after=_wide_clean(ws, rows))


@case("search", "dprhot_search")
def _search():
    """Two cases of the dense-search table with the same shapes: shard A (two chunks) from an empty state, shard B (two chunks) folded in."""
    import _search_cases as SC

    kn = kernels()[0]
    a, b = SC.load("N-nan-corpus-rows").case, SC.load("N-nan-query-row").case
    assert (a.k, a.chunk) == (b.k, b.chunk) and [s[0] for s in a.shards] == [s[0] for s in b.shards] and not a.options and not b.options
    A = [dv(a.Q, BF16)] + [dv(C, BF16) for _, C in a.shards]
    B = [dv(b.Q, BF16)] + [dv(C, BF16) for _, C in b.shards]
    values, indices = empty((a.nq, a.k), torch.float32), empty((a.nq, a.k), torch.int64)
    ws = kn.search_workspace(a.nq, a.chunk, values)
    offs = [s[0] for s in a.shards]

    def fn(x):
        kn.search(x[0], x[1], offs[0], values, indices, True, a.chunk, ws)
        kn.search(x[0], x[2], offs[1], values, indices, False, a.chunk, ws)
        return ()

    return Built(A, B, fn, outs=[values, indices], ws=[ws])


# ---- inverted-index retrieval ---------------------------------------------------------------------------------------------------------
def _reverse_experts(post_doc, rows, off, corpus_len, queries):
    """The same postings and entries under the expert ids V - 1 - e: other exp_off, another posting order, the same counts."""
    V = len(off) - 1
    ex = np.repeat(np.arange(V), np.diff(off))
    order = np.argsort((V - 1 - ex) * corpus_len + post_doc.astype(np.int64), kind="stable")
    off2 = np.concatenate([[0], np.cumsum(np.bincount(V - 1 - ex, minlength=V))]).astype(np.int64)
    return post_doc[order], rows[order], off2, [{(V - 1 - e if e < V else e): v for e, v in q.items()} for q in queries]


def _ivf_batch_tensors(qb):
    return [qb.ent_vec, qb.ent_q, qb.bexp, qb.boff] + ([qb.cls] if qb.cls is not None else [])


def _ivf_batch_of(t, nq, has_cls):
    return _ns(ent_vec=t[0], ent_q=t[1], bexp=t[2], boff=t[3], cls=t[4] if has_cls else None, nq=nq, n_entries=int(t[1].shape[0]))


@case("ivf", "dprhot_ivf_score", "dprhot_ivf_search")
def _ivf():
    """A golden CITADEL fixture with CLS vectors: 20 passages in chunks of 8, ids [0, 8) from an empty state and [8, 20) folded in."""
    import _ivf_fixture as IF
    from dpr_scale_amd import ivf

    kn = kernels()[0]
    meta, z = IF.load("ivf_citadel23_cls")
    n, nq, k, chunk = int(meta["corpus_len"]), int(meta["nq"]), 8, 8
    cls_q, emb, _ = IF.queries(meta, z)
    index = ivf.IVFIndex(torch.from_numpy(z["post_expert"]), torch.from_numpy(z["post_doc"]), torch.from_numpy(z["post_vec"]),
                         torch.from_numpy(z["cls_doc"]), n, "cpu")
    post_doc2, vec2, off2, emb2 = _reverse_experts(index.post_doc.numpy(), index.post_vec.float().numpy(), index.exp_off.numpy(), n, emb)
    qa, qb = ivf.pack_queries(cls_q, emb), ivf.pack_queries(cls_q.flip(0), emb2)
    A = [dv(index.post_vec), dv(index.post_doc), dv(index.exp_off), dv(index.cls)] + [dv(t) for t in _ivf_batch_tensors(qa)]
    B = [dv(vec2, BF16), dv(post_doc2), dv(off2), dv(index.cls.flip(1))] + [dv(t) for t in _ivf_batch_tensors(qb)]
    S = empty((nq, 24), torch.float32)
    values, indices = empty((nq, k), torch.float32), empty((nq, k), torch.int64)
    ws = kn.ivf_workspace(nq, qa.n_entries, chunk, True, k, values)

    def fn(x):
        I = _ns(post_vec=x[0], post_doc=x[1], exp_off=x[2], cls=x[3], n_postings=int(x[1].shape[0]), n_experts=int(x[2].shape[0]) - 1,
                dp=int(x[0].shape[1]), dc=int(x[3].shape[1]), corpus_len=n)
        q = _ivf_batch_of(x[4:], nq, True)
        S.zero_()
        kn.ivf_score(I, q, 0, n, S)
        kn.ivf_search(I, q, 0, 8, values, indices, True, chunk, ws)
        kn.ivf_search(I, q, 8, n, values, indices, False, chunk, ws)
        return ()

    return Built(A, B, fn, outs=[S, values, indices], ws=[ws])


@case("ivf_pq", "dprhot_pq_encode", "dprhot_ivf_pq_score", "dprhot_ivf_pq_search")
def _ivf_pq():
    """The Zipf case of the IVF conformance table in its product-quantised form (2003 passages, CLS vectors, dp = 64, dsub = 4): chunks
    of 512, ids [0, 512) from an empty state and the other three chunks folded in; the codes of the packed rows re-encoded."""
    import _ivf_cases as IC
    from dpr_scale_amd import ivf

    kn = kernels()[0]
    case_ = IC.load("G-zipf").case
    dsub, codebook, codes, post_doc, off = IC.pq_form("G-zipf")
    rows = IC.packed(case_)[1]
    cls_q, cls_doc = IC.cls_of("G-zipf")
    n, nq, k, chunk = case_.corpus_len, len(case_.queries), 10, 512
    post_doc2, codes2, off2, queries2 = _reverse_experts(post_doc, codes, off, n, case_.queries)
    rows2 = _reverse_experts(post_doc, rows, off, n, case_.queries)[1]
    qa, qb = ivf.pack_queries(torch.from_numpy(cls_q), case_.queries), ivf.pack_queries(torch.from_numpy(cls_q).flip(0), queries2)
    cls = torch.cat([ivf._pad_cols(torch.from_numpy(cls_doc).float(), 8).to(BF16), torch.zeros((8, (cls_doc.shape[1] + 7) // 8 * 8), dtype=BF16)], 0)
    A = [dv(codes), dv(codebook, BF16), dv(post_doc), dv(off), dv(cls), dv(rows, BF16)] + [dv(t) for t in _ivf_batch_tensors(qa)]
    B = [dv(codes2), dv(codebook, BF16).flip(1).contiguous(), dv(post_doc2), dv(off2), dv(cls.flip(1)), dv(rows2, BF16)] \
        + [dv(t) for t in _ivf_batch_tensors(qb)]
    S = empty((nq, 2008), torch.float32)
    values, indices = empty((nq, k), torch.float32), empty((nq, k), torch.int64)
    ws = kn.ivf_workspace(nq, qa.n_entries, chunk, True, k, values)

    def fn(x):
        I = _ns(post_code=x[0], codebook=x[1], dsub=dsub, post_doc=x[2], exp_off=x[3], cls=x[4], n_postings=int(x[2].shape[0]),
                n_experts=int(x[3].shape[0]) - 1, dp=int(x[5].shape[1]), dc=int(x[4].shape[1]), corpus_len=n)
        q = _ivf_batch_of(x[6:], nq, True)
        S.zero_()
        kn.ivf_pq_score(I, q, 0, n, S)
        kn.ivf_pq_search(I, q, 0, 512, values, indices, True, chunk, ws)
        kn.ivf_pq_search(I, q, 512, n, values, indices, False, chunk, ws)
        return (kn.pq_encode(x[5], x[1]),)

    return Built(A, B, fn, outs=[S, values, indices], ws=[ws])


@case("ivf-no-cls", "dprhot_ivf_search")
def _ivf_no_cls():
    """A golden COIL fixture WITHOUT CLS vectors: every chunk's score buffer then starts from zeros the call itself writes (the first
    node of the captured graph: zero_words_kernel, once a hipMemsetAsync whose zeroes were absent on replay), the expert part is added
    on top.  The search form only: 20 passages in chunks of 8, [0, 8) then [8, 20)."""
    import _ivf_fixture as IF
    from dpr_scale_amd import ivf

    kn = kernels()[0]
    meta, z = IF.load("ivf_coil")
    n, nq, k, chunk = int(meta["corpus_len"]), int(meta["nq"]), 8, 8
    _, emb, _ = IF.queries(meta, z)
    index = ivf.IVFIndex(torch.from_numpy(z["post_expert"]), torch.from_numpy(z["post_doc"]), torch.from_numpy(z["post_vec"]), None, n, "cpu")
    post_doc2, vec2, off2, emb2 = _reverse_experts(index.post_doc.numpy(), index.post_vec.float().numpy(), index.exp_off.numpy(), n, emb)
    qa, qb = ivf.pack_queries([], emb), ivf.pack_queries([], emb2)
    A = [dv(index.post_vec), dv(index.post_doc), dv(index.exp_off)] + [dv(t) for t in _ivf_batch_tensors(qa)]
    B = [dv(vec2, BF16), dv(post_doc2), dv(off2)] + [dv(t) for t in _ivf_batch_tensors(qb)]
    values, indices = empty((nq, k), torch.float32), empty((nq, k), torch.int64)
    ws = kn.ivf_workspace(nq, qa.n_entries, chunk, False, k, values)

    def fn(x):
        I = _ns(post_vec=x[0], post_doc=x[1], exp_off=x[2], cls=None, n_postings=int(x[1].shape[0]), n_experts=int(x[2].shape[0]) - 1,
                dp=int(x[0].shape[1]), dc=0, corpus_len=n)
        q = _ivf_batch_of(x[3:], nq, False)
        kn.ivf_search(I, q, 0, 8, values, indices, True, chunk, ws)
        kn.ivf_search(I, q, 8, n, values, indices, False, chunk, ws)
        return ()

    return Built(A, B, fn, outs=[values, indices], ws=[ws])


@case("ivf_pack", "dprhot_ivf_compact", "dprhot_ivf_gather")
def _ivf_pack():
    """Postings from a repr dict: dprhot_ivf_compact through ctypes (the HipKernels method reads the count back), then dprhot_ivf_gather
    over every record slot of the capacity (a slot the compaction left unwritten is outside the slots and gives a row of zeros)."""
    import _ivf_pack_inputs as IP

    kn = kernels()[0]
    Bs, Ls, K, d = 7, 19, 3, 40

    def data(seed):
        r = IP.gaussian_repr(seed, Bs, Ls, K, d)
        w = r["expert_weights"].float()
        w[1, 2, 0] = float("nan")
        return [dv(r["expert_ids"], torch.int32), dv(w), dv(r["attention_mask"] > 0, torch.uint8),
                dv(torch.randperm(1000, generator=torch.Generator().manual_seed(seed))[:Bs], torch.int32), dv(r["expert_repr"])]

    cap = Bs * Ls * K
    seq_off = empty(Bs + 1, torch.int32)
    expert, row, slot = (empty(cap, torch.int32) for _ in range(3))
    weight = empty(cap, torch.float32)

    def fn(x):
        _call("dprhot_ivf_compact", x[0], x[1], x[2], x[3], Bs, Ls, K, 1, 0.05, seq_off, expert, row, slot, weight, cap)
        return (kn.ivf_gather(x[4], x[1], slot, None, K, True, BF16, 64),)

    return Built(data(71), data(72), fn, outs=[seq_off, expert, row, slot, weight])


# ---- ColBERT: exhaustive, candidate lists, centroid interaction, residual and PQ token indexes --------------------------------------------
RAGGED_A = [[], [10], list(range(40)), list(range(1, 39, 2)), [0]]           # the RAGGED lists of tests/test_colbert_cand_gpu.py: 61 ids
RAGGED_B = [[10], [], list(range(1, 39, 2)), list(range(40)), [3]]            # a list that grows, one that empties, the long ones swapped
assert [sum(len(x) for x in r[:n]) for r in (RAGGED_A, RAGGED_B) for n in (4, 5)] == [60, 61, 60, 61]  # the same n_cand for 4 and 5 queries


def _lists(per_query, nq, n_docs):
    """cand_off / cand_doc for nq queries and a corpus of n_docs passages from the ragged pattern (ids folded into the corpus)."""
    import test_colbert_cand_gpu as CAND

    return CAND.lists([[j % n_docs for j in per_query[i % len(per_query)]] for i in range(nq)])


def _search_bufs(workspace, nq, k, chunk):
    values, indices = empty((nq, k), torch.float32), empty((nq, k), torch.int64)
    return values, indices, workspace(nq, chunk, k, values)


for _cshape in ("d24", "d128"):
    def _colbert(shape=_cshape):
        """The corpus of the candidate-list tests (40 passages, ragged block counts): exhaustive score and search (chunks of 8: ids
        [0, 16) from an empty state, [16, 40) folded in), candidate score and search over ragged lists."""
        import test_colbert_cand_gpu as CAND
        from dpr_scale_amd import colbert

        kn = kernels()[0]
        q, _, index = CAND.corpus(shape, 5)
        nq, LQ, n = q.shape[0], q.shape[1], index.corpus_len
        qb = colbert._bf16_padded(q.to(DEV), index.dp)
        A = [index.tok.clone(), index.doc_blk.clone(), qb, *_lists(RAGGED_A, nq, n)]
        B = [index.tok.roll(16, 0), _shift_offsets(index.doc_blk), qb.flip(0).contiguous(), *_lists(RAGGED_B, nq, n)]
        S, SC_ = empty((nq, n), torch.float32), empty((nq, 43), torch.float32)
        v1, i1, ws1 = _search_bufs(kn.colbert_workspace, nq, 10, 8)
        v2, i2, ws2 = _search_bufs(kn.colbert_cand_workspace, nq, 30, 8)

        def fn(x):
            I = _ns(tok=x[0], doc_blk=x[1], n_blk=index.n_blk, corpus_len=n, dp=index.dp)
            kn.colbert_score(I, x[2], 0, 0, n, S)
            kn.colbert_search(I, x[2], 0, 0, 16, v1, i1, True, 8, ws1)
            kn.colbert_search(I, x[2], 0, 16, n, v1, i1, False, 8, ws1)
            kn.colbert_cand_score(I, x[2], 1, x[3], x[4], 0, 43, SC_)
            kn.colbert_cand_search(I, x[2], 1, x[3], x[4], n, v2, i2, 8, ws2)
            return ()

        return Built(A, B, fn, outs=[S, SC_, v1, i1, v2, i2], ws=[ws1, ws2])

    case(f"colbert-{_cshape}", "dprhot_colbert_score", "dprhot_colbert_search", "dprhot_colbert_cand_score", "dprhot_colbert_cand_search")(_colbert)


@case("colbert_search-k5000", "dprhot_colbert_search")
def _colbert_wide():
    """6000 passages of one to three tokens, k = 5000: the chunk driver on the HBM-resident selection, chunks of 2048, ids [0, 2048) from
    an empty state and the other two chunks folded in.  The selection's error record behind the score buffer is read after the replay."""
    from dpr_scale_amd import colbert

    kn, _, _lib = kernels()
    n, nq, LQ, d, k, chunk = 6000, 2, 4, 32, 5000, 2048

    def data(seed):
        g = torch.Generator().manual_seed(seed)
        lens = torch.randint(1, 4, (n,), generator=g)
        index = colbert.ColBERTIndex(torch.arange(n), lens, torch.randn(int(lens.sum()), d, generator=g).to(BF16), n, DEV)
        return index, [index.tok, index.doc_blk, dv(torch.randn(nq, LQ, d, generator=g), BF16)]

    index, A = data(81)
    B = data(82)[1]
    assert B[0].shape == A[0].shape, "one block per passage: the same n_blk"
    B[1] = _shift_offsets(B[1])
    values, indices, ws = _search_bufs(kn.colbert_workspace, nq, k, chunk)
    score_bytes = _lib.colbert_workspace_bytes(nq, chunk)

    def fn(x):
        I = _ns(tok=x[0], doc_blk=x[1], n_blk=index.n_blk, corpus_len=n, dp=index.dp)
        kn.colbert_search(I, x[2], 0, 0, chunk, values, indices, True, chunk, ws)
        kn.colbert_search(I, x[2], 0, chunk, n, values, indices, False, chunk, ws)
        return ()

    return Built(A, B, fn, outs=[values, indices], ws=[ws], after=_wide_clean(ws[score_bytes:], nq))


for _cshape in ("d24", "d128"):
    def _colbert_cen(shape=_cshape):
        """Centroid interaction over the corpus of its own tests (300 grid centroids): table, score and search over ragged lists.  B's
        tokens sit under other centroids (a relabelling that keeps every passage's count) and its lists are the other ragged set."""
        import test_colbert_cen_gpu as CEN
        from dpr_scale_amd import colbert

        kn = kernels()[0]
        q, index, _ = CEN.corpus(shape, 5)
        nq, LQ, n, C = q.shape[0], q.shape[1], index.corpus_len, int(index.centroids.shape[0])
        qb = colbert._bf16_padded(q.to(DEV), index.dp)
        off_a, cen_a = index.doc_centroids()
        tc = index.tok_centroid
        tc_b = torch.where(tc >= 0, (tc * 7 + 3) % C, tc)
        off_b, cen_b = colbert._doc_centroid_lists(tc_b, index.doc_blk, C, n)
        assert off_b.shape == off_a.shape and cen_b.shape == cen_a.shape and not torch.equal(cen_a, cen_b)
        A = [index.centroids.clone(), qb, off_a.clone(), cen_a.clone(), *_lists(RAGGED_A, nq, n)]
        B = [index.centroids.flip(0).contiguous(), qb.flip(0).contiguous(), off_b, cen_b, *_lists(RAGGED_B, nq, n)]
        T = empty((nq, C, (LQ + 15) // 16 * 16), torch.float32)
        S = empty((nq, 43), torch.float32)
        values, indices, ws = _search_bufs(kn.colbert_cen_workspace, nq, 30, 8)

        def fn(x):
            I = _ns(centroids=x[0], corpus_len=n, doc_centroids=lambda: (x[2], x[3]))
            kn.colbert_cen_table(I, x[1], T)
            kn.colbert_cen_score(I, T, LQ, 0, x[4], x[5], 0, 43, S)
            kn.colbert_cen_search(I, T, LQ, 1, x[4], x[5], n, values, indices, 8, ws)
            return ()

        return Built(A, B, fn, outs=[T, S, values, indices], ws=[ws])

    case(f"colbert_cen-{_cshape}", "dprhot_colbert_cen_table", "dprhot_colbert_cen_score", "dprhot_colbert_cen_search")(_colbert_cen)


for _d, _nbits in ((24, 2), (128, 4)):  # dp = 32 and dp = 128
    def _colbert_res(d=_d, nbits=_nbits):
        """The residual index of its own tests (30 passages, 16 centroids, trained buckets): encode of the decoded rows, score and search
        over ragged lists.  B: other centroid ids (a relabelling), other codes, weights and block offsets."""
        import test_colbert_res_gpu as RES
        from dpr_scale_amd import colbert

        kn = kernels()[0]
        res, dec = RES.built(d, nbits)
        nq, LQ, n, C = RES.NQ, 17, res.corpus_len, int(res.centroids.shape[0])
        qb = colbert._bf16_padded(RES.queries(d, LQ).to(DEV), res.dp)
        tc = res.tok_centroid
        A = [res.res_code.clone(), tc.clone(), res.centroids.clone(), res.weights.clone(), res.doc_blk.clone(), qb, dec.tok.clone(), res.cutoffs.clone(),
             *_lists(RAGGED_A, nq, n)]
        B = [res.res_code.roll(5, 0), torch.where(tc >= 0, (tc * 5 + 1) % C, tc), res.centroids.flip(0).contiguous(), res.weights.flip(0).contiguous(),
             _shift_offsets(res.doc_blk), qb.flip(0).contiguous(), dec.tok.roll(3, 0), (res.cutoffs * 0.5).contiguous(), *_lists(RAGGED_B, nq, n)]
        S = empty((nq, 33), torch.float32)
        values, indices, ws = _search_bufs(kn.colbert_res_workspace, nq, 12, 8)

        def fn(x):
            I = _ns(res_code=x[0], tok_centroid=x[1], centroids=x[2], weights=x[3], nbits=nbits, doc_blk=x[4], n_blk=res.n_blk, corpus_len=n)
            kn.colbert_res_score(I, x[5], 0, x[8], x[9], 0, 33, S)
            kn.colbert_res_search(I, x[5], 1, x[8], x[9], 40, values, indices, 8, ws)
            return (kn.colbert_res_encode(x[6], x[7], nbits, x[1], x[2]),)

        return Built(A, B, fn, outs=[S, values, indices], ws=[ws])

    case(f"colbert_res-d{_d}", "dprhot_colbert_res_encode", "dprhot_colbert_res_score", "dprhot_colbert_res_search")(_colbert_res)


for _d, _dsub in ((24, 2), (128, 8)):  # dp = 32 and dp = 128
    def _colbert_pq(d=_d, dsub=_dsub):
        """The product-quantised token index of its own tests (51 passages): encode of the dense rows, score and search (chunks of 8: ids
        [0, 16) from an empty state, [16, 51) folded in).  B: other codes, row counts per block, block offsets and codebook."""
        import test_colbert_pq_gpu as PQ
        from dpr_scale_amd import colbert

        kn = kernels()[0]
        q, dense, pq, _ = PQ.case(d, dsub)
        nq, n = q.shape[0], pq.corpus_len
        qb = colbert._bf16_padded(q.to(DEV), pq.dp)
        A = [pq.tok_code.clone(), pq.blk_rows.clone(), pq.codebook.clone(), pq.doc_blk.clone(), qb, dense.tok.clone()]
        B = [pq.tok_code.roll(7, 0), pq.blk_rows.flip(0).contiguous(), pq.codebook.flip(1).contiguous(), _shift_offsets(pq.doc_blk),
             qb.flip(0).contiguous(), dense.tok.roll(16, 0)]
        S = empty((nq, 56), torch.float32)
        values, indices, ws = _search_bufs(kn.colbert_workspace, nq, 9, 8)

        def fn(x):
            I = _ns(tok_code=x[0], blk_rows=x[1], codebook=x[2], dsub=dsub, doc_blk=x[3], n_blk=pq.n_blk, corpus_len=n, dp=pq.dp)
            kn.colbert_pq_score(I, x[4], 0, 0, n, S)
            kn.colbert_pq_search(I, x[4], 1, 0, 16, values, indices, True, 8, ws)
            kn.colbert_pq_search(I, x[4], 1, 16, n, values, indices, False, 8, ws)
            return (kn.colbert_pq_encode(x[5], x[2]),)

        return Built(A, B, fn, outs=[S, values, indices], ws=[ws])

    case(f"colbert_pq-d{_d}", "dprhot_colbert_pq_encode", "dprhot_colbert_pq_score", "dprhot_colbert_pq_search")(_colbert_pq)


# ---- SPAR and the fp8 dense index -----------------------------------------------------------------------------------------------------
@case("spar", "dprhot_spar_score", "dprhot_spar_search")
def _spar():
    """Grid operands of the SPAR oracle, three weights: chunks of 64, ids [0, 64) from an empty state and [64, 200) folded in."""
    import _spar_oracle as SO

    kn = kernels()[0]
    nq, n, d1, d2, k, chunk = 5, 200, 32, 96, 10, 64
    lam = SO.grid_lams(3)

    def data(seed):
        rng = np.random.default_rng(seed)
        return [dv(SO.grid(rng, nq, d1), BF16), dv(SO.grid(rng, nq, d2), BF16), dv(SO.grid(rng, n, d1), BF16), dv(SO.grid(rng, n, d2), BF16)]

    A, B = data(91), data(92)
    B[2][[3, 70, 199]] = float("nan")
    S = empty((3 * nq, n), torch.float32)
    values, indices = empty((3 * nq, k), torch.float32), empty((3 * nq, k), torch.int64)
    ws = kn.spar_workspace(nq, 3, chunk, k, values)

    def fn(x):
        I = _ns(c1=x[2], c2=x[3], corpus_len=n)
        kn.spar_score(I, x[0], x[1], lam, 0, n, S)
        kn.spar_search(I, x[0], x[1], lam, 0, 64, values, indices, True, chunk, ws)
        kn.spar_search(I, x[0], x[1], lam, 64, n, values, indices, False, chunk, ws)
        return ()

    return Built(A, B, fn, outs=[S, values, indices], ws=[ws])


for _d in (32, 100):  # dp = 32 and dp = 128
    def _fp8(d=_d):
        """Grid rows of the fp8 oracle encoded on the device, scored and searched (chunks of 64: ids [0, 64) from an empty state, [64, 200)
        folded in).  B holds a non-finite row on either side: a NaN scale, NaN scores in other places."""
        import _fp8_oracle as FO

        kn = kernels()[0]
        nq, n, k, chunk, dp = 5, 200, 10, 64, FO.padded_width(d)

        def data(seed):
            rng = np.random.default_rng(seed)
            return [dv(FO.grid(rng, nq, d)), dv(FO.grid(rng, n, d))]

        A, B = data(93), data(94)
        A[1][7, 3] = float("nan")
        B[0][2, 0] = float("inf")
        B[1][[0, 64, 130], 5] = float("nan")
        qc, qs, cc, cs = empty((nq, dp), torch.uint8), empty(nq, torch.float32), empty((n, dp), torch.uint8), empty(n, torch.float32)
        S = empty((nq, n), torch.float32)
        values, indices, ws = _search_bufs(kn.dense_fp8_workspace, nq, k, chunk)

        def fn(x):
            kn.fp8_encode(x[0], qc, qs)
            kn.fp8_encode(x[1], cc, cs)
            I = _ns(codes=cc, scale=cs, corpus_len=n)
            kn.dense_fp8_score(I, qc, qs, 0, n, S)
            kn.dense_fp8_search(I, qc, qs, 0, 64, values, indices, True, chunk, ws)
            kn.dense_fp8_search(I, qc, qs, 64, n, values, indices, False, chunk, ws)
            return ()

        return Built(A, B, fn, outs=[qc, qs, cc, cs, S, values, indices], ws=[ws])

    case(f"dense_fp8-d{_d}", "dprhot_fp8_encode", "dprhot_dense_fp8_score", "dprhot_dense_fp8_search")(_fp8)


def covered():
    return set().union(*(c.symbols for c in CASES))
