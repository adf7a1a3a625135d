"""Row-kernel conformance on the MI355X: the stand-alone kernels of csrc/rowwise.h behind their C-ABI calls, element by element.

  softmax-CE  softmax_ce_kernel<64> / <256> (dprhot_softmax_ce_fwd_bwd) on the case table of tests/_rowwise_cases.py against its fp64
              oracle: row_lse, row_loss and G inside the bounds derived in that module's docstring (the worst err / bound per output is
              printed; above 1 the kernel or the derivation is wrong), finite / non-finite patterns equal, and -- with no tolerance --
              row_loss == row_lse - S[row, y + y_offset] as fp32 words, G exactly 0 at -inf and out-of-window columns, the same words
              without G, on a second run, for a row alone and with the batch reversed.  The CPU half
              (tests/test_rowwise_conformance.py) shows that the table tells the kernel's plan from ten defective ones.
  wrapper     HotCrossEntropyLoss against fp64 cross_entropy where it pads with -inf, through (3 * loss).backward().
  casts       dprhot_cast_bf16 / dprhot_prep against tensor.to(torch.bfloat16), word for word (NaNs as NaN-ness).
  packing     dprhot_pack_ctx / dprhot_unpack_mask word for word against the layout comment of rowwise.h restated in numpy.
  reduce      dprhot_reduce_sum within (gamma(ceil(n / 256) + 9) sum|x| + u |sum|) |scale| of the fp64 sum.
  rank        dprhot_rank_of_gold equal to the oracle's count with y_offset != 0, non-finite cells and ties.
Outputs of the bare ABI calls sit between two 4096-byte guard bands, as in the other conformance suites.

MEASURED on an MI355X (`test_worst_ratios_of_the_table`'s printout; worst err / bound over the 123 cases): lse 0.385 and loss 0.384
(V-down-8200), G 0.49 (V-peaky-8200); the wrapper's mean loss at most 0.049 of its bound, dprhot_reduce_sum at most 0.033.  Before the
NaN rule of DESIGN.md section 7 was put into pass 1, the eleven cases N-nan_alone_before_finite-*, N-nan_alone_first_then_finite-* and
N-nan_in_empty_row-* failed (a finite lse / loss where the oracle has NaN) and every other test of this file passed."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _bounds as Bd  # noqa: E402
import _rowwise_cases as C  # noqa: E402
from oracle import inbatch_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5
BF16, F32 = torch.bfloat16, torch.float32
WORST = {}  # output -> (ratio, case): filled by the per-case test, printed by test_worst_ratios_of_the_table


@pytest.fixture(scope="module")
def kn():
    from dpr_scale_amd.hotpath import HipKernels

    assert torch.cuda.is_available(), "needs a HIP device"
    return HipKernels()


class Bands:
    """Device tensors that are the interior of a byte buffer filled with PATTERN; `check` after the calls."""

    def __init__(self):
        self.regions = []

    def empty(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.regions.append((raw, n))
        return raw[GUARD:GUARD + n].view(dtype).view(shape)

    def check(self):
        torch.cuda.synchronize()
        for raw, n in self.regions:
            assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[GUARD + n:] == PATTERN).all()), f"guard band of a {n}-byte buffer overwritten"


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _words(t):
    """The words of a tensor with every NaN mapped to one pattern (NaNs compare as NaN-ness, not payload)."""
    t = t.detach().cpu().contiguous()
    w = t.view(torch.int16 if t.element_size() == 2 else torch.int32).clone()
    w[torch.isnan(t)] = -1
    return w


# ---- softmax-CE ------------------------------------------------------------------------------------------------------------------------
def _inputs(case, rows=None):
    rows = slice(None) if rows is None else rows
    S = torch.from_numpy(case.S[rows]).contiguous().to(DEV)
    y = torch.from_numpy(case.y[rows].copy()).to(DEV)
    ws = None if case.win_start is None else torch.from_numpy(case.win_start[rows].copy()).to(DEV)
    return S, y, ws


def _ce(kn, case, rows=None, want_G=None):
    """Through HipKernels.softmax_ce -> (row_loss, row_lse, G) on the CPU."""
    S, y, ws = _inputs(case, rows)
    want_G = case.want_G if want_G is None else want_G
    loss, lse, G = kn.softmax_ce(S, y, case.y_offset, case.gs, want_G=want_G, row_win_start=ws, win_len=case.win_len)
    torch.cuda.synchronize()
    return loss.cpu(), lse.cpu(), None if G is None else G.cpu()


def _ce_abi(kn, case):
    """Through the bare ABI with every output between guard bands."""
    S, y, ws = _inputs(case)
    B, Nc = S.shape
    bands = Bands()
    loss, lse = bands.empty((B,), F32), bands.empty((B,), F32)
    G = bands.empty((B, Nc), BF16) if case.want_G else None
    kn._lib.check(kn.lib.dprhot_softmax_ce_fwd_bwd(_p(S), B, Nc, _p(y), case.y_offset, case.gs, _p(ws), case.win_len, _p(loss), _p(lse), _p(G),
                                                   _stream()), "dprhot_softmax_ce_fwd_bwd")
    bands.check()
    return loss.cpu(), lse.cpu(), None if G is None else G.cpu()


def _same_words(a, b):
    return all((x is None and y is None) or torch.equal(_words(x), _words(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", C.NAMES)
def test_softmax_ce_case_is_within_the_derived_bounds(kn, name):
    L = C.load(name)
    case, ref = L.case, L.ref
    loss, lse, G = _ce_abi(kn, case)
    sc = C.check(case, ref, loss, lse, G)
    print(f"{name}: " + " ".join(f"{k}={v:.3g}" for k, v in sc.items()))
    for k, v in sc.items():
        if k != "words" and v >= WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (v, name)
    # finite and non-finite patterns, then the bounds
    assert Bd.finite_match(lse, ref["lse"]) and Bd.finite_match(loss, ref["loss"]), (name, case.note, lse, ref["lse"], loss, ref["loss"])
    if G is not None:
        assert Bd.finite_match(G, ref["G"]), (name, case.note, "rows whose G differs in its finite pattern",
                                              torch.nonzero((torch.isfinite(G) != torch.isfinite(ref["G"])).any(1)).flatten().tolist())
        # exactly 0 outside the window, and at -inf columns of a row that has a logsumexp; the gold excepted
        S = torch.from_numpy(case.S)
        zero = ref["outside"] | ((S == -math.inf) & torch.isfinite(ref["lse"])[:, None])
        zero[torch.arange(len(case.y)), ref["yg"]] = False
        assert bool((G[zero] == 0).all()), (name, case.note)
    assert sc["words"] == 0, (name, "row_loss is not fp32(row_lse - S[row, y + y_offset])")
    assert C.worst(sc) <= 1.0, (name, case.note, sc)


@pytest.mark.parametrize("name", C.NAMES)
def test_softmax_ce_words_do_not_depend_on_the_call(kn, name):
    """No tolerance: the wrapper and the bare ABI, a second run, a run without G, every row alone and the batch reversed give the
    same words."""
    case = C.load(name).case
    B = len(case.y)
    first = _ce_abi(kn, case)
    assert _same_words(_ce(kn, case), first), (name, "HipKernels.softmax_ce differs from the bare ABI / a second run")
    assert _same_words(_ce(kn, case, want_G=False)[:2], first[:2]), (name, "row_loss / row_lse differ without G")
    rev = np.arange(B)[::-1].copy()
    back = _ce(kn, case, rows=rev)
    assert _same_words([None if t is None else t[torch.from_numpy(rev)] for t in back], first), (name, "rows depend on their order")
    for i in range(B):
        alone = _ce(kn, case, rows=np.array([i]))
        assert _same_words(alone, [None if t is None else t[i:i + 1] for t in first]), (name, f"row {i} depends on its neighbours")


def test_worst_ratios_of_the_table():
    """The measurement: worst err / bound per output over the whole table (run after the per-case test)."""
    assert set(WORST) == {"lse", "loss", "G"}, "run together with test_softmax_ce_case_is_within_the_derived_bounds"
    print("worst err / bound over the table: " + ", ".join(f"{k} {v:.3g} ({n})" for k, (v, n) in WORST.items()))
    assert all(v <= 1.0 for v, _ in WORST.values()), WORST


# ---- the loss wrapper -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Nc", [5, 8, 13])
def test_loss_wrapper_equals_fp64_cross_entropy(kn, Nc, dtype):
    from dpr_scale_amd.task.dpr_task import HotCrossEntropyLoss

    g = np.random.default_rng(40 + Nc)
    B = 6
    scores = torch.from_numpy(g.standard_normal((B, Nc)).astype(np.float32)).to(dtype)
    y = g.integers(0, Nc, size=B)
    y[0], y[1] = 0, Nc - 1
    pad = -Nc % 8
    padded = np.concatenate([scores.float().numpy(), np.full((B, pad), -np.inf, np.float32)], 1)
    case = C._case(padded, y, f"the loss wrapper's Nc={Nc}")
    ref = C.oracle(case)
    x64 = scores.double().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(x64, torch.from_numpy(y))
    (3 * want).backward()
    assert torch.allclose(ref["loss"].mean(), want.detach(), rtol=1e-13, atol=0)
    assert torch.allclose(ref["G"][:, :Nc] * 3, x64.grad, rtol=2.0 ** -24, atol=0)  # (the oracle's gs is the fp32 of 1 / B)

    loss_fn = HotCrossEntropyLoss(kernels=kn)
    x = scores.to(DEV).requires_grad_(True)
    loss = loss_fn(x, torch.from_numpy(y).to(DEV))
    (3 * loss).backward()
    assert loss.shape == () and x.grad.shape == (B, Nc) and x.grad.dtype == dtype
    # the mean: every row inside its bound, then dprhot_reduce_sum's (below) with scale 1 / B
    l = ref["loss"]
    # (2u: the multiply, and 1 / B as the fp32 the kernel is given)
    bound = (float(ref["e_loss"].sum()) + Bd.gamma(1 + 9, Bd.U) * float(l.abs().sum()) + 2 * Bd.U * float(l.sum().abs())) / B
    err = abs(float(loss) - float(want))
    print(f"Nc={Nc} {dtype}: loss err / bound = {err / bound:.3g}")
    assert err <= bound, (float(loss), float(want), bound)
    # the gradient: the kernel's bf16 G (scale 1 / B, judged like the table's), times go = 3 in fp32, rounded to the input dtype
    _, _, G = _ce(kn, case)
    assert float(Bd.g_scores(G, ref)[0].max()) <= 1.0
    assert torch.equal(_words(x.grad), _words((G[:, :Nc].float() * 3).to(dtype)))
    # the path without a gradient: the same loss bits
    again = loss_fn(scores.to(DEV), torch.from_numpy(y).to(DEV))
    assert torch.equal(_words(again.reshape(1)), _words(loss.detach().reshape(1)))


# ---- casts -----------------------------------------------------------------------------------------------------------------------------
# bf16 ties up and down (the kept bit odd / even) of both signs, subnormals, +-0, +-inf, the largest finite fp32 and the tie below it
# (both round to inf), the largest value that stays finite, a quiet and a signalling NaN
SPECIAL_BITS = (0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x00000001, 0x007FFFFF, 0x80000001, 0x00008000,
                0x00018000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7FFFFF, 0x7FC00000,
                0x7F800001, 0xFFC12345)


def _cast_source(n, seed):
    """n fp32 words: a third special patterns, a third random bit patterns, a third Gaussian."""
    g = np.random.default_rng(seed)
    w = g.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    pick = g.integers(0, 3 * len(SPECIAL_BITS), size=n)
    for j, b in enumerate(SPECIAL_BITS):
        w[pick == j] = np.uint32(b)
    gauss = g.standard_normal(n).astype(np.float32).view(np.uint32)
    w = np.where(pick >= 2 * len(SPECIAL_BITS), gauss, w)
    w[: len(SPECIAL_BITS)] = np.array(SPECIAL_BITS, dtype=np.uint32)[:n]
    return torch.from_numpy(w.view(np.int32).copy()).view(F32)


def _check_cast(got, src, what):
    want = src.to(BF16)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, "NaN-ness")
    bad = torch.nonzero(_words(got) != _words(want)).flatten()
    assert not len(bad), (what, len(bad), [(hex(int(src.view(torch.int32)[i]) & 0xFFFFFFFF), hex(int(got.view(torch.int16)[i]) & 0xFFFF),
                                            hex(int(want.view(torch.int16)[i]) & 0xFFFF)) for i in bad[:5].tolist()])


@pytest.mark.parametrize("n", [8, 2040, 2048, 2056, 4096 + 8])
def test_cast_bf16_word_for_word(kn, n):
    src = _cast_source(n, n)
    bands = Bands()
    dst, src_d = bands.empty((n,), BF16), src.to(DEV)
    kn._lib.check(kn.lib.dprhot_cast_bf16(_p(src_d), _p(dst), n, _stream()), "dprhot_cast_bf16")
    bands.check()
    _check_cast(dst.cpu(), src, f"cast_bf16 n={n}")
    # and through the wrapper
    out = torch.empty(n, dtype=BF16, device=DEV)
    kn.cast_bf16(src_d, out)
    assert torch.equal(_words(out), _words(dst))


# the last pair: more than 2048 * 256 groups of 8 in all, so the grid is capped and every thread strides
@pytest.mark.parametrize("nq,nc", [(8, 8), (8, 2056), (2040, 16), (2048, 4096 + 8), (4096 + 8, 2040), (8 * (2048 * 256 + 5), 2056)])
def test_prep_word_for_word(kn, nq, nc):
    q, c = _cast_source(nq, nq + 1), _cast_source(nc, nc + 2)
    bands = Bands()
    Qb, Cb, q_d, c_d = bands.empty((nq,), BF16), bands.empty((nc,), BF16), q.to(DEV), c.to(DEV)
    kn._lib.check(kn.lib.dprhot_prep(_p(q_d), nq, _p(Qb), _p(c_d), nc, _p(Cb), _stream()), "dprhot_prep")
    bands.check()
    _check_cast(Qb.cpu(), q, f"prep q nq={nq} nc={nc}")
    _check_cast(Cb.cpu(), c, f"prep c nq={nq} nc={nc}")


# ---- packing ---------------------------------------------------------------------------------------------------------------------------
PACK_SHAPES = [(1, 8), (7, 8), (16, 8), (17, 8), (33, 64), (129, 64), (2047, 8), (2048, 8)]


def _packed_rows(n_ctx, d):
    """dprhot_packed_rows restated: the context rows, ceil(n_ctx / 2d) rows for n_ctx mask bytes, rounded up to 8 rows (64 from 2048
    contexts on)."""
    align = 64 if n_ctx >= 2048 else 8
    return -(-(n_ctx + -(-n_ctx // (2 * d))) // align) * align


def _pack_ref(c, mask, rows_c):
    """The send buffer as bytes (rowwise.h: rows [0, n_ctx) = contexts; rows [n_ctx, rows_c) = mask bytes, then zeros)."""
    n_ctx, d = c.shape
    out = np.zeros(rows_c * d * 2, dtype=np.uint8)
    out[: n_ctx * d * 2] = c.to(BF16).view(torch.int16).numpy().view(np.uint8).reshape(-1)
    if mask is not None:
        out[n_ctx * d * 2: n_ctx * d * 2 + n_ctx] = mask != 0
    return out


def _pack(kn, c, mask, rows_c):
    n_ctx, d = c.shape
    bands = Bands()
    send = bands.empty((rows_c, d), BF16)
    m, c_d = None if mask is None else torch.from_numpy(mask).to(DEV), c.to(DEV)
    kn._lib.check(kn.lib.dprhot_pack_ctx(_p(c_d), _p(m), n_ctx, d, _p(send), _stream()), "dprhot_pack_ctx")
    bands.check()
    return send


def _pack_inputs(n_ctx, d, seed):
    g = np.random.default_rng(seed)
    c = torch.from_numpy(g.standard_normal((n_ctx, d)).astype(np.float32))
    mask = g.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=n_ctx)
    return c, mask


@pytest.mark.parametrize("n_ctx,d", PACK_SHAPES)
def test_pack_ctx_word_for_word(kn, n_ctx, d):
    rows_c = _packed_rows(n_ctx, d)
    assert rows_c == kn.packed_rows(n_ctx, d) and rows_c % 8 == 0 and (rows_c - n_ctx) * d * 2 >= n_ctx
    c, mask = _pack_inputs(n_ctx, d, 50 + n_ctx)
    for mk in (mask, None, np.zeros(n_ctx, np.uint8), np.full(n_ctx, 255, np.uint8)):
        send = _pack(kn, c, mk, rows_c)
        got = send.cpu().view(torch.int16).numpy().view(np.uint8).reshape(-1)
        want = _pack_ref(c, mk, rows_c)
        assert np.array_equal(got[: n_ctx * d * 2], want[: n_ctx * d * 2]), "context rows"
        assert np.array_equal(got[n_ctx * d * 2: n_ctx * d * 2 + n_ctx], want[n_ctx * d * 2: n_ctx * d * 2 + n_ctx]), "mask bytes"
        assert not got[n_ctx * d * 2 + n_ctx:].any(), "bytes behind the mask"
    # and through the wrapper
    out = torch.empty((rows_c, d), dtype=BF16, device=DEV)
    kn.pack_ctx(c.to(DEV), torch.from_numpy(mask).to(DEV), out)
    assert torch.equal(out.cpu().view(torch.int16), _pack(kn, c, mask, rows_c).cpu().view(torch.int16))


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("n_ctx,d", PACK_SHAPES)
def test_unpack_mask_word_for_word(kn, n_ctx, d, W):
    rows_c = _packed_rows(n_ctx, d)
    sends, want = [], []
    for r in range(W):
        c, mask = _pack_inputs(n_ctx, d, 60 + 10 * r + n_ctx)
        if r == 1:
            mask = None  # a rank without a mask
        sends.append(_pack(kn, c, mask, rows_c))
        want.append(np.concatenate([np.zeros(n_ctx, np.uint8) if mask is None else (mask != 0).astype(np.uint8),
                                    np.ones(rows_c - n_ctx, np.uint8)]))  # header rows: always masked
    gathered = torch.cat(sends, 0).contiguous()
    bands = Bands()
    colmask = bands.empty((W * rows_c,), torch.uint8)
    kn._lib.check(kn.lib.dprhot_unpack_mask(_p(gathered), W, n_ctx, d, _p(colmask), _stream()), "dprhot_unpack_mask")
    bands.check()
    assert np.array_equal(colmask.cpu().numpy(), np.concatenate(want))
    out = torch.empty(W * rows_c, dtype=torch.uint8, device=DEV)
    kn.unpack_mask(gathered, W, n_ctx, out)
    assert torch.equal(out, colmask)


# ---- reduce ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2047, 2048, 2049, 8192 + 3])
def test_reduce_sum_within_its_bound(kn, n):
    """A thread adds ceil(n / 256) values in index order, then 6 wave steps and 3 additions across the waves: gamma(ceil(n / 256) + 9)
    on sum|x|; the multiply by scale: u |sum|."""
    g = np.random.default_rng(70 + n)
    x = (g.standard_normal(n) * np.exp(g.uniform(-3, 3, size=n))).astype(np.float32)  # mixed signs and magnitudes
    for scale in (1.0, -0.375, 1.0 / 7):
        sc = float(np.float32(scale))
        want = float(x.astype(np.float64).sum())
        bound = (Bd.gamma(-(-n // 256) + 9, Bd.U) * float(np.abs(x.astype(np.float64)).sum()) + Bd.U * abs(want)) * abs(sc)
        bands = Bands()
        out = bands.empty((1,), F32)
        xd = torch.from_numpy(x).to(DEV)
        kn._lib.check(kn.lib.dprhot_reduce_sum(_p(xd), n, sc, _p(out), _stream()), "dprhot_reduce_sum")
        bands.check()
        err = abs(float(out) - want * sc)
        print(f"n={n} scale={scale:.3g}: err / bound = {err / bound:.3g}")
        assert err <= bound, (n, scale, float(out), want * sc, bound)
        assert torch.equal(kn.reduce_sum(xd, sc).cpu().view(torch.int32), out.cpu().view(torch.int32)), "two runs differ"
    x[n // 2] = np.nan
    assert math.isnan(float(kn.reduce_sum(torch.from_numpy(x).to(DEV), 0.5)))


# ---- rank ------------------------------------------------------------------------------------------------------------------------------
def _rank_case(cols, y_offset, seed):
    """S fp32 [9, cols] on a coarse grid (ties on both sides of a gold), rank-local y.  Rows 2, 3, 4: -inf, +inf, NaN non-gold cells;
    row 5: all three; row 6: every cell ties with the gold; row 7: a -inf gold among -inf cells; row 8: a +inf gold."""
    g = np.random.default_rng(seed)
    rows = 9
    S = (g.integers(-6, 7, size=(rows, cols)) / 2.0).astype(np.float32)
    y = g.integers(0, cols - y_offset, size=rows)
    y[0], y[1], y[6] = 0, cols - y_offset - 1, (cols - y_offset) // 2
    gold = y + y_offset
    for i, v in enumerate((-np.inf, np.inf, np.nan)):
        pick = g.choice(cols, size=max(2, cols // 5), replace=False)
        S[2 + i, pick[pick != gold[2 + i]]] = v
        S[5, pick[pick != gold[5]][i::3]] = v
    S[6, :] = 1.5
    S[7, g.choice(cols, size=cols // 2, replace=False)] = -np.inf
    S[7, gold[7]] = -np.inf
    S[8, gold[8]] = np.inf
    return S, y


@pytest.mark.parametrize("y_offset", [0, 4, 7])
@pytest.mark.parametrize("cols", [8, 260, 1028, 2052])
def test_rank_of_gold_with_offset_ties_and_non_finite_cells(kn, cols, y_offset):
    """1 + #{S > gold} + #{S == gold, j < y + y_offset}: a NaN cell is never counted, -inf ties with a -inf gold."""
    S, y = _rank_case(cols, y_offset, 80 + cols + y_offset)
    want = O.rank_of_gold(S, y + y_offset)
    got = kn.rank_of_gold(torch.from_numpy(S).to(DEV), torch.from_numpy(y).to(DEV), y_offset).cpu().numpy()
    assert np.array_equal(got, want), (got, want)
