"""Every entry point of the training-step family refuses a bad call on the host, before its first launch, with the documented status code:
one row per entry point and refusal kind.  A workspace refusal also says how many bytes dprhot_workspace_bytes asks for, and names the entry
point wherever the library has always named it.

The rows hold no made-up address: every buffer is a torch tensor of (at least) its true size, on the device when there is one, so a call
that launched by mistake would be harmless -- only the workspace_bytes ARGUMENT is understated, and a misaligned pointer is a true buffer's
address plus 4 (each buffer has that much slack).  Next to each row: why the call is refused before anything is launched."""
import ctypes

import pytest
import torch

INVALID, UNSUPPORTED, WORKSPACE = -1, -3, -4

# one smallest shape per plan family (default options; tests/test_bounds_cpu.py PLAN_TABLE pins the gates)
SMALL = (8, 16, 64)      # small step: two launches (step_small.h)
FEW = (32, 1032, 128)    # few rows x many contexts (skinny.h); under 2^19 scores, so it wants G and leaves 17 dQ slabs to a caller who asks
GEN = (64, 512, 64)      # general family, short-row forward, register-staged backward pair with 4 dQ slabs
NL = (256, 256, 128)     # with big_min = 1: a no-logits shape (one-pass forward on the 256 x 256 tile)
# the packed step's shapes are (B, W, n_ctx, d); its column count is W * dprhot_packed_rows(n_ctx, d)
P_SMALL = (8, 2, 8, 64)      # 2 x 16 columns: small step
P_FEW = (32, 2, 512, 128)    # 2 x 520 columns: few rows

SIGS = {
    "dprhot_sim_fwd": "Qb B Cb Nc d colmask one S stream",
    "dprhot_dc": "G Qb B Nc d one d_scale dC stream",
    "dprhot_dq": "G Cb B Nc d one d_scale dQ ws wsb stream",
    "dprhot_sim_stats": "Qb B Cb Nc d y zero colmask one S_out ws wsb stream",
    "dprhot_sim_stats_f32": "q c Qb Cb B Nc d y zero colmask one S_out ws wsb stream",
    "dprhot_softmax_finish": "S_out B Nc d y zero one row_loss row_lse loss_sum G ws wsb stream",
    "dprhot_dscores": "Qb B Cb Nc d y zero colmask one one lse_in G ws wsb stream",
    "dprhot_inbatch_fwd": "Qb B Cb Nc d y zero colmask one one S_out row_loss row_lse loss_sum G ws wsb stream",
    "dprhot_inbatch_fwd_f32": "q c Qb Cb B Nc d y zero colmask one one S_out row_loss row_lse loss_sum G ws wsb stream",
    "dprhot_inbatch_bwd": "G Qb Cb B Nc d one d_scale dQ dC ws wsb stream",
    "dprhot_inbatch_step_f32": "q c Qb Cb B Nc d y zero colmask one one one d_scale S_out row_loss row_lse loss_sum G dQ dC ws wsb stream",
    "dprhot_inbatch_step_packed_f32": "q Cb Qb B W rank n_ctx d y one one one d_scale row_loss row_lse loss_sum G dQ dC ws wsb stream",
    "dprhot_train_step_f32": "q c Qb Cb B Nc d y zero colmask one one one d_scale row_loss row_lse loss_sum G dQ dq_part dC dc_kind ws wsb stream",
    "dprhot_train_step_packed_f32": "q Cb Qb B W rank n_ctx d y one one one d_scale row_loss row_lse loss_sum G dQ dq_part dC dc_kind ws wsb stream",
}
POINTERS = {"q", "c", "Qb", "Cb", "y", "S", "row_loss", "row_lse", "loss_sum", "G", "dQ", "dC", "slabs", "ws"}

# (entry point, shape, what is wrong, code, who a workspace error names, why the call is refused before the first launch -- each row was
# read against the library as it stood before the checks were separated from the launching bodies, which refused it at the same point)
#   null X / misalign X: that argument NULL / its buffer's address + 4;   set {...}: arguments replaced;   ws-1: workspace_bytes one short
ROWS = [
    # --- NULL required pointer
    ("dprhot_sim_fwd", GEN, ("null", "S"), INVALID, None, "REQUIRE(Q && C && S) is the first statement"),
    ("dprhot_dc", GEN, ("null", "dC"), INVALID, None, "REQUIRE(G && Q && dC_part) is the first statement"),
    ("dprhot_dq", GEN, ("null", "dQ"), INVALID, None, "REQUIRE(G && C && dQ) is the first statement"),
    ("dprhot_sim_stats", GEN, ("null", "y"), INVALID, None, "REQUIRE(Q && C && y) is the first statement"),
    ("dprhot_sim_stats_f32", GEN, ("null", "Qb"), INVALID, None, "REQUIRE(q && Qb && Cb && y) is the first statement"),
    ("dprhot_softmax_finish", GEN, ("null", "loss_sum"), INVALID, None, "REQUIRE(y && loss_sum) is the first statement"),
    ("dprhot_dscores", GEN, ("null", "G"), INVALID, None, "REQUIRE(Q && C && y && G) is the first statement"),
    ("dprhot_inbatch_fwd", GEN, ("null", "y"), INVALID, None, "not a no-logits shape: straight into dprhot_sim_stats, whose REQUIRE is first"),
    ("dprhot_inbatch_fwd_f32", GEN, ("null", "Qb"), INVALID, None, "B <= 128: straight into dprhot_sim_stats_f32, whose REQUIRE is first"),
    ("dprhot_inbatch_bwd", GEN, ("null", "G"), INVALID, None, "REQUIRE(G && Q && C) is the first statement"),
    ("dprhot_inbatch_step_f32", SMALL, ("null", "dQ"), INVALID, None, "REQUIRE(loss_sum && dQ && dC_part) is the first statement"),
    ("dprhot_inbatch_step_packed_f32", P_SMALL, ("null", "Cb"), INVALID, None, "REQUIRE(q && gathered && ...) is the first statement"),
    ("dprhot_train_step_f32", GEN, ("null", "loss_sum"), INVALID, None, "shape, dc_kind and dq_part pass; the step's first REQUIRE refuses"),
    ("dprhot_train_step_packed_f32", P_SMALL, ("null", "q"), INVALID, None, "dc_kind and dq_part pass; the packed step's first REQUIRE refuses"),
    # --- bad shape
    ("dprhot_sim_fwd", GEN, ("set", {"Nc": 508}), INVALID, None, "check_shape (Nc % 8) follows the NULL check"),
    ("dprhot_dc", GEN, ("set", {"d": 60}), INVALID, None, "check_shape (d % 8) follows the NULL check"),
    ("dprhot_dq", GEN, ("set", {"B": 0}), INVALID, None, "check_shape (B > 0) follows the NULL check"),
    ("dprhot_sim_stats", GEN, ("set", {"Nc": 508}), INVALID, None, "check_shape follows the NULL check"),
    ("dprhot_sim_stats_f32", GEN, ("set", {"d": 60}), INVALID, None, "check_shape follows the NULL check"),
    ("dprhot_softmax_finish", GEN, ("set", {"Nc": 508}), INVALID, None, "check_shape follows the NULL check"),
    ("dprhot_dscores", GEN, ("set", {"Nc": 508}), INVALID, None, "check_shape follows the NULL check"),
    ("dprhot_inbatch_fwd", GEN, ("set", {"Nc": 508}), INVALID, None, "64 rows: no one-pass forward whatever Nc; dprhot_sim_stats' check_shape"),
    ("dprhot_inbatch_fwd_f32", GEN, ("set", {"d": 60}), INVALID, None, "B <= 128: dprhot_sim_stats_f32's check_shape"),
    ("dprhot_inbatch_bwd", GEN, ("set", {"Nc": 508}), INVALID, None, "check_shape follows the NULL check"),
    ("dprhot_inbatch_step_f32", SMALL, ("set", {"Nc": 12}), INVALID, None, "check_shape follows the pointer checks"),
    ("dprhot_inbatch_step_packed_f32", P_SMALL, ("set", {"rank": 2}), INVALID, None, "REQUIRE(rank < W) is the second statement"),
    ("dprhot_train_step_f32", GEN, ("set", {"Nc": 508}), INVALID, None, "check_shape is the first statement"),
    ("dprhot_train_step_packed_f32", P_SMALL, ("set", {"W": 0}), INVALID, None, "REQUIRE(W > 0 ...) is the first statement"),
    # --- misaligned pointer
    ("dprhot_sim_fwd", GEN, ("misalign", "S"), INVALID, None, "the alignment REQUIRE follows check_shape"),
    ("dprhot_dc", GEN, ("misalign", "dC"), INVALID, None, "the alignment REQUIRE follows check_shape"),
    ("dprhot_dq", GEN, ("misalign", "dQ"), INVALID, None, "the alignment REQUIRE follows check_shape"),
    ("dprhot_sim_stats", GEN, ("misalign", "Qb"), INVALID, None, "the alignment REQUIRE follows check_shape"),
    ("dprhot_sim_stats", GEN, ("misalign", "ws"), INVALID, None, "the workspace's alignment is checked right behind its size"),
    ("dprhot_sim_stats_f32", GEN, ("misalign", "q"), INVALID, None, "the alignment REQUIRE follows check_shape"),
    ("dprhot_softmax_finish", GEN, ("misalign", "G"), INVALID, None, "the alignment REQUIRE follows check_shape"),
    ("dprhot_dscores", GEN, ("misalign", "G"), INVALID, None, "the alignment REQUIRE follows check_shape (in front of the no-logits test)"),
    ("dprhot_inbatch_fwd", GEN, ("misalign", "Qb"), INVALID, None, "dprhot_sim_stats checks Q in front of its launch (G only behind it)"),
    ("dprhot_inbatch_fwd_f32", GEN, ("misalign", "q"), INVALID, None, "B <= 128: dprhot_sim_stats_f32 checks q in front of its launch"),
    ("dprhot_inbatch_bwd", GEN, ("misalign", "dQ"), INVALID, None, "dQ and dC_part given, default options: the REQUIRE over all five pointers"),
    ("dprhot_inbatch_step_f32", GEN, ("misalign", "dQ"), INVALID, None, "REQUIRE(aligned16(G) && aligned16(dQ) ...) is the second statement"),
    ("dprhot_inbatch_step_f32", SMALL, ("misalign", "ws"), INVALID, None, "dprhot_sim_stats_f32 checks the workspace in front of its launch"),
    ("dprhot_inbatch_step_packed_f32", P_SMALL, ("misalign", "dC"), INVALID, None, "the step's second statement"),
    ("dprhot_train_step_f32", FEW, ("misalign", "dQ"), INVALID, None, "the step's second statement"),
    ("dprhot_train_step_packed_f32", P_FEW, ("misalign", "dQ"), INVALID, None, "the step's second statement"),
    # --- workspace understated by one byte
    ("dprhot_dq", GEN, ("ws-1",), WORKSPACE, b"dq", "4 slabs: the size check follows the pointer checks"),
    ("dprhot_sim_stats", GEN, ("ws-1",), WORKSPACE, b"sim_stats", "the size check follows the pointer checks"),
    ("dprhot_sim_stats_f32", GEN, ("ws-1",), WORKSPACE, b"sim_stats", "the size check follows the pointer checks"),
    ("dprhot_softmax_finish", GEN, ("ws-1",), WORKSPACE, b"softmax_finish", "the size check follows the pointer checks"),
    ("dprhot_dscores", NL, ("ws-1",), WORKSPACE, b"dscores", "no-logits shape, row_lse == NULL: the size check follows"),
    ("dprhot_inbatch_fwd", NL, ("ws-1",), WORKSPACE, b"inbatch_fwd", "one-pass forward: pointer checks, then the size check"),
    # (no name asserted where the message used to name the launch group the call had reached, "sim_stats", and now names the entry point)
    ("dprhot_inbatch_fwd_f32", GEN, ("ws-1",), WORKSPACE, None, "B <= 128: dprhot_sim_stats_f32's size check, in front of its launch"),
    ("dprhot_inbatch_bwd", GEN, ("ws-1",), WORKSPACE, b"inbatch_bwd", "the register-staged pair with 4 dQ slabs: size check, then the launch"),
    ("dprhot_inbatch_step_f32", FEW, ("ws-1",), WORKSPACE, b"inbatch_step", "few-rows branch: pointer checks, size check, then the cast launch"),
    ("dprhot_inbatch_step_f32", SMALL, ("ws-1",), WORKSPACE, None, "dprhot_sim_stats_f32's size check, in front of its launch"),
    ("dprhot_inbatch_step_f32", GEN, ("ws-1",), WORKSPACE, None, "B <= 128: dprhot_sim_stats_f32's size check, in front of its launch"),
    ("dprhot_inbatch_step_packed_f32", P_FEW, ("ws-1",), WORKSPACE, b"inbatch_step", "few-rows branch of the step"),
    ("dprhot_train_step_f32", FEW, ("ws-1",), WORKSPACE, b"inbatch_step", "few-rows branch of the step"),
    ("dprhot_train_step_packed_f32", P_FEW, ("ws-1",), WORKSPACE, b"inbatch_step", "few-rows branch of the step"),
    # --- G == NULL where dprhot_step_wants_g is 1
    ("dprhot_inbatch_step_f32", SMALL, ("null", "G"), INVALID, None, "the dprhot_step_wants_g test follows check_shape"),
    ("dprhot_inbatch_step_f32", FEW, ("null", "G"), INVALID, None, "the dprhot_step_wants_g test follows check_shape"),
    ("dprhot_inbatch_step_f32", GEN, ("null", "G"), INVALID, None, "the dprhot_step_wants_g test follows check_shape"),
    ("dprhot_inbatch_step_packed_f32", P_FEW, ("null", "G"), INVALID, None, "the step's dprhot_step_wants_g test"),
    ("dprhot_train_step_f32", GEN, ("null", "G"), INVALID, None, "the step's dprhot_step_wants_g test"),
    ("dprhot_train_step_packed_f32", P_SMALL, ("null", "G"), INVALID, None, "the step's dprhot_step_wants_g test"),
    # --- dC_part as bf16 at a shape outside the few-rows plan
    ("dprhot_train_step_f32", SMALL, ("set", {"dc_kind": 0}), UNSUPPORTED, None, "the dc_kind test follows check_shape (step_admit)"),
    ("dprhot_train_step_f32", GEN, ("set", {"dc_kind": 0}), UNSUPPORTED, None, "the dc_kind test follows check_shape (step_admit)"),
    ("dprhot_train_step_packed_f32", P_SMALL, ("set", {"dc_kind": 0}), UNSUPPORTED, None, "the dc_kind test follows dprhot_packed_rows"),
    # --- dq_part where dprhot_train_dq_slabs is 0
    ("dprhot_train_step_f32", SMALL, ("set", {"dq_part": "slabs"}), INVALID, None, "the dq_part test follows the dc_kind test (step_admit)"),
    ("dprhot_train_step_f32", GEN, ("set", {"dq_part": "slabs"}), INVALID, None, "the dq_part test follows the dc_kind test (step_admit)"),
    ("dprhot_train_step_packed_f32", P_SMALL, ("set", {"dq_part": "slabs"}), INVALID, None, "the dq_part test follows the dc_kind test (step_admit)"),
]

_BUFFERS = {}


def _good_args(shape):
    """Buffers and scalars of a correct call at `shape`; the tensors stay alive in _BUFFERS."""
    from dpr_scale_amd import _lib

    if len(shape) == 4:
        B, W, n_ctx, d = shape
        Nc = W * _lib.packed_rows(n_ctx, d)
    else:
        (B, Nc, d), W, n_ctx = shape, 1, 0
    key = (B, Nc, d, _lib.options_epoch())
    if key not in _BUFFERS:
        dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        slack = 8  # elements: room for the 4 bytes a misaligned pointer is moved by

        def buf(n, dtype):
            return torch.zeros(n + slack, dtype=dtype, device=dev)

        f32, bf16 = torch.float32, torch.bfloat16
        wsb = _lib.workspace_bytes(B, Nc, d)
        _BUFFERS[key] = dict(q=buf(B * d, f32), c=buf(Nc * d, f32), Qb=buf(B * d, bf16), Cb=buf(Nc * d, bf16), y=buf(B, torch.int64),
                             S=buf(B * Nc, f32), row_loss=buf(B, f32), row_lse=buf(B, f32), loss_sum=buf(1, f32), G=buf(B * Nc, bf16),
                             dQ=buf(B * d, f32), dC=buf(Nc * d, f32), slabs=buf(64 * B * d, f32), ws=buf(wsb, torch.uint8), wsb=wsb)
    t = _BUFFERS[key]
    args = {k: v.data_ptr() for k, v in t.items() if k in POINTERS}
    assert all(p % 16 == 0 for p in args.values())
    args.update(B=B, Nc=Nc, d=d, W=W, rank=0, n_ctx=n_ctx, wsb=t["wsb"], one=1.0, zero=0, dc_kind=2, colmask=None, d_scale=None, S_out=None,
                lse_in=None, dq_part=None, stream=None)
    return args


def test_shapes_are_in_the_families_they_stand_for():
    from dpr_scale_amd import _lib

    assert _lib.step_wants_g(*SMALL) and _lib.step_wants_g(*FEW) and _lib.step_wants_g(*GEN)
    assert (_lib.train_dq_slabs(*SMALL), _lib.train_dq_slabs(*FEW), _lib.train_dq_slabs(*GEN)) == (0, 17, 0)
    assert (_lib.packed_rows(8, 64), _lib.packed_rows(512, 128)) == (16, 520)
    assert _lib.train_dq_slabs(8, 32, 64) == 0 and _lib.train_dq_slabs(32, 1040, 128) > 1 and _lib.step_wants_g(32, 1040, 128)
    assert not _lib.fwd_no_logits(*NL) and all(_lib.fwd_one_pass(*s) == 0 for s in (SMALL, FEW, GEN, NL))


@pytest.mark.parametrize("entry,shape,wrong,code,who,why", ROWS, ids=[f"{r[0][7:]}-{'x'.join(map(str, r[1]))}-{'-'.join(map(str, r[2][:2]))}" for r in ROWS])
def test_refused_on_the_host(entry, shape, wrong, code, who, why):
    from dpr_scale_amd import _lib

    lowered = shape == NL
    if lowered:
        _lib.set_option("big_min", 1)
    try:
        if lowered:
            assert _lib.fwd_no_logits(*NL) and _lib.fwd_one_pass(*NL) == 1
        args = _good_args(shape)
        kind = wrong[0]
        if kind == "null":
            args[wrong[1]] = None
        elif kind == "misalign":
            args[wrong[1]] += 4
        elif kind == "ws-1":
            args["wsb"] -= 1
        else:
            args.update({k: (args[v] if isinstance(v, str) else v) for k, v in wrong[1].items()})
        rc = getattr(_lib.lib, entry)(*[args[name] for name in SIGS[entry].split()])
        err = _lib.lib.dprhot_last_error()
        assert rc == code, (entry, shape, wrong, rc, err, why)
        if code == WORKSPACE:
            assert b"needs %d workspace bytes, got %d" % (args["wsb"] + 1, args["wsb"]) in err, err
            if who is not None:
                assert err.startswith(who + b" needs "), err
    finally:
        if lowered:
            _lib.set_option("big_min", 256)
