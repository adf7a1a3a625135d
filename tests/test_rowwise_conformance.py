"""The row softmax-CE conformance table on the CPU (tests/_rowwise_cases.py; the GPU half is tests/test_rowwise_conformance_gpu.py).

  1. The fp64 oracle is pinned against torch.nn.functional.cross_entropy(reduction='none') and its autograd in fp64, on the columns of
     each row's window: values, the non-finite rules (an all -inf row, a -inf gold, NaN and +inf inside, NaN and +inf outside a
     window) and the -inf padding HotCrossEntropyLoss appends.
  2. The table is shown to discriminate.  `emulate` restates the PLAN of softmax_ce_kernel (csrc/rowwise.h) in numpy fp32 -- thread t of
     a row strides 4 TPR columns, online max / sum with a rescale only when the maximum moves, the xor-butterfly combine and the
     4-wave LDS combine of TPR 256, pass 2 in groups of 8 with the window test per column -- with a `defect=` switch.  The faithful
     stand-in must pass the checker on every case; every defect of DEFECTS must fail at least one case, and the test prints which
     (as test_injected_bug_is_far_outside_the_bounds does for the training step)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _bounds as Bd  # noqa: E402
import _rowwise_cases as C  # noqa: E402

DEFECTS = {
    "win_end_inclusive": "the window's end taken inclusively",
    "win_begin_rounded": "the window's begin rounded down to a multiple of 4",
    "win_without_y_offset": "y_offset not applied to the window",
    "onehot_at_y": "the onehot at y instead of y + y_offset",
    "last_trip_dropped": "the last, partial trip of pass 1 dropped",
    "no_rescale": "the running sum not rescaled when the maximum moves",
    "three_waves": "the fourth wave left out of the TPR 256 combine",
    "pass2_no_window": "out-of-window columns not zeroed in pass 2",
    "gs_before_onehot": "grad_scale applied before the onehot is subtracted",
    "nan_dropped": "a NaN alone among -inf, met before any finite value, dropped from the sum (the kernel before this suite)",
}
F32 = np.float32
NINF = F32(-np.inf)


def _combine(m, s, m2, s2):
    """ms_combine on arrays: (max, sum relative to it) pairs; a -inf maximum carries sum 0."""
    M = np.fmax(m, m2)  # fmaxf: drops a NaN
    with np.errstate(invalid="ignore", over="ignore"):
        out = (s * np.exp(m - M) + s2 * np.exp(m2 - M)).astype(F32)
    return M, np.where(M == NINF, F32(0), out)


def emulate(case, defect=None):
    """(row_loss fp32 [B], row_lse fp32 [B], G bf16 [B, Nc] or None) after softmax_ce_kernel's plan in fp32."""
    assert defect is None or defect in DEFECTS
    S, (B, Nc) = case.S, case.S.shape
    tpr = C.tpr_of(Nc)
    windowed = case.win_start is not None
    loss, lse_out, G = np.empty(B, F32), np.empty(B, F32), np.zeros((B, Nc), F32)
    col = np.arange(Nc)
    for i in range(B):
        lo, hi = 0, Nc
        if windowed:
            lo = int(case.win_start[i]) + (0 if defect == "win_without_y_offset" else case.y_offset)
            hi = lo + case.win_len
        lo1 = lo & ~3 if defect == "win_begin_rounded" else lo
        hi1 = hi + 1 if defect == "win_end_inclusive" else hi
        out1 = (col < lo1) | (col >= hi1) if windowed else np.zeros(Nc, bool)
        # pass 1: thread t reads the float4 at 4 t + 4 tpr k in trip k
        m, s = np.full(tpr, NINF), np.zeros(tpr, F32)
        trips = -(-Nc // (4 * tpr))
        for k in range(trips):
            if defect == "last_trip_dropped" and (k + 1) * 4 * tpr > Nc:
                break
            j0 = k * 4 * tpr
            n = min(tpr, (Nc - j0) // 4)  # threads with a float4 in this trip
            v = np.where(out1[j0:j0 + 4 * n], NINF, S[i, j0:j0 + 4 * n]).reshape(n, 4)
            lm = np.fmax(np.fmax(v[:, 0], v[:, 1]), np.fmax(v[:, 2], v[:, 3]))
            mt, st = m[:n].copy(), s[:n].copy()
            with np.errstate(invalid="ignore", over="ignore"):
                up = lm > mt
                if defect != "no_rescale":
                    st = np.where(up, (st * np.exp(mt - lm)).astype(F32), st)  # m == -inf: 0 * 0
                mt = np.where(up, lm, mt)
                if defect != "nan_dropped":  # a group of NaN beside -inf: no maximum, but its NaN reaches the sum
                    mt = np.where((mt == NINF) & (((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])) != NINF), F32(0), mt)
                e = np.exp(v - mt[:, None]).astype(F32)
                add = (st + (((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3])).astype(F32)
            m[:n], s[:n] = mt, np.where(mt != NINF, add, st)
        # combine: the xor butterfly inside each wave of 64, then the waves through LDS
        lane = np.arange(tpr)
        for o in (32, 16, 8, 4, 2, 1):
            m, s = _combine(m, s, m[lane ^ o], s[lane ^ o])
        M, T = m[0], s[0]
        for w in range(1, tpr // 64):
            if defect == "three_waves" and w == 3:
                break
            M, T = _combine(M, T, m[64 * w], s[64 * w])
        with np.errstate(invalid="ignore", divide="ignore"):
            lse = F32(M + np.log(F32(T)))
            yi = int(case.y[i]) + case.y_offset
            lse_out[i], loss[i] = lse, lse - S[i, yi]
            # pass 2
            out2 = (col < lo) | (col >= hi) if windowed and defect != "pass2_no_window" else np.zeros(Nc, bool)
            pr = np.where(out2, F32(0), np.exp(S[i] - lse).astype(F32))
            hot = int(case.y[i]) if defect == "onehot_at_y" else yi
            if defect == "gs_before_onehot":
                g = (pr * F32(case.gs)).astype(F32)
                g[hot] -= F32(1)
            else:
                pr[hot] -= F32(1)
                g = (pr * F32(case.gs)).astype(F32)
        G[i] = g
    G = torch.from_numpy(G).to(torch.bfloat16) if case.want_G else None
    return torch.from_numpy(loss), torch.from_numpy(lse_out), G


# ---- 1. the oracle against torch.nn.functional.cross_entropy ---------------------------------------------------------------------------
def _torch_ce(S, yg, gs):
    """fp64 cross_entropy(reduction='none') of one row's window and the gradient of gs * loss."""
    x = S.clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(x[None, :], torch.tensor([yg]), reduction="none")[0]
    (g,) = torch.autograd.grad(loss * gs, x)
    return loss.detach(), g


def _same(a, b, tol):
    a, b = a.to(torch.float64), b.to(torch.float64)
    if not Bd.finite_match(a, b):
        return False
    f = torch.isfinite(b)
    return bool(((a[f] - b[f]).abs() <= tol * (1 + b[f].abs())).all())


@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_equals_fp64_cross_entropy_on_every_window(name):
    L = C.load(name)
    case, ref = L.case, L.ref
    S = torch.from_numpy(case.S).to(torch.float64)
    for i in range(S.shape[0]):
        lo, hi = 0, S.shape[1]
        if case.win_start is not None:
            lo = int(case.win_start[i]) + case.y_offset
            hi = lo + case.win_len
        yg = int(case.y[i]) + case.y_offset
        loss, g = _torch_ce(S[i, lo:hi], yg - lo, case.gs)
        assert _same(ref["loss"][i], loss, 1e-12), (name, i, float(ref["loss"][i]), float(loss))
        assert _same(ref["G"][i, lo:hi], g, 1e-12), (name, i)
        assert bool((ref["G"][i, :lo] == 0).all()) and bool((ref["G"][i, hi:] == 0).all()), (name, i)
        if torch.isfinite(ref["lse"][i]):
            assert _same(ref["lse"][i], torch.logsumexp(S[i, lo:hi], 0), 1e-12), (name, i)


def test_non_finite_rules_are_those_of_cross_entropy():
    """The rules of the oracle's docstring, each on a row of its own, straight from torch in fp64."""
    inf, nan = np.inf, np.nan
    x = lambda *v: torch.tensor(v, dtype=torch.float64)
    loss, g = _torch_ce(x(-inf, -inf, -inf, -inf), 1, 0.5)          # an all -inf row
    assert torch.isnan(loss) and torch.isnan(g).all()
    loss, g = _torch_ce(x(1.0, -inf, 2.0, 0.5), 1, 0.5)             # a -inf gold
    assert loss == inf and torch.isfinite(g).all() and g[1] == -0.5
    for bad in (nan, inf):                                          # NaN or +inf inside: everything NaN
        loss, g = _torch_ce(x(1.0, bad, 2.0, 0.5), 0, 0.5)
        assert torch.isnan(loss) and torch.isnan(g).all()
    loss, g = _torch_ce(x(1.0, 2.0, 3.0, 4.0, nan, -inf, -inf, -inf), 0, 1.0)  # Nc = 5 with a NaN in column 4, as the loss wrapper pads it
    assert torch.isnan(loss) and torch.isnan(g).all()
    # and the oracle says the same of the case built that way
    L = C.load("N-nan_alone_before_finite-8")
    assert torch.isnan(L.ref["loss"][1]) and torch.isnan(L.ref["lse"][1]) and torch.isnan(L.ref["G"][1]).all()
    assert torch.isfinite(L.ref["loss"][[0, 2, 3]]).all() and torch.isfinite(L.ref["G"][[0, 2, 3]]).all()


@pytest.mark.parametrize("Nc", [5, 8, 13])
def test_padding_of_the_loss_wrapper_changes_nothing(Nc):
    """HotCrossEntropyLoss pads the columns to a multiple of 8 with -inf: loss and gradient of the first Nc columns stay, G of the pad
    is 0 -- in cross_entropy and in the oracle."""
    g = np.random.default_rng(Nc)
    B = 4
    S = g.standard_normal((B, Nc)).astype(np.float32)
    y = g.integers(0, Nc, size=B)
    pad = -Nc % 8
    Sp = np.concatenate([S, np.full((B, pad), -np.inf, np.float32)], 1)
    ref = C.oracle(C._case(Sp, y, "padded"))
    for i in range(B):
        loss, grad = _torch_ce(torch.from_numpy(S[i]).double(), int(y[i]), 1.0 / B)
        lossp, gradp = _torch_ce(torch.from_numpy(Sp[i]).double(), int(y[i]), 1.0 / B)
        assert _same(lossp, loss, 1e-15) and _same(gradp[:Nc], grad, 1e-15) and bool((gradp[Nc:] == 0).all())
        assert _same(ref["loss"][i], loss, 1e-12) and _same(ref["G"][i, :Nc], grad, 1e-12) and bool((ref["G"][i, Nc:] == 0).all())


# ---- 2. the table discriminates ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def faithful():
    return {n: emulate(C.load(n).case) for n in C.NAMES}


@pytest.mark.parametrize("name", C.NAMES)
def test_faithful_standin_passes_every_case(faithful, name):
    L = C.load(name)
    sc = C.check(L.case, L.ref, *faithful[name])
    print(f"{name}: " + " ".join(f"{k}={v:.3g}" for k, v in sc.items()))
    assert C.worst(sc) <= 1.0, (name, L.case.note, sc)


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_every_defect_fails_some_case(defect):
    caught = {}
    for n in C.NAMES:
        L = C.load(n)
        w = C.worst(C.check(L.case, L.ref, *emulate(L.case, defect)))
        if w > 1.0:
            caught[n] = w
    print(f"{defect} ({DEFECTS[defect]}): caught by {len(caught)} of {len(C.NAMES)} cases: "
          + ", ".join(f"{n} ({w:.3g})" for n, w in list(caught.items())[:6]))
    assert caught, f"no case notices: {DEFECTS[defect]}"


def test_the_dropped_nan_is_caught_by_the_cases_built_for_it():
    """The suspected behaviour of the kernel before this suite shows exactly where the issue said: a NaN alone among -inf that its
    thread meets before any finite value.  After a finite value the NaN arrives by itself, defect or not."""
    caught = {n for n in C.NAMES if C.worst(C.check(C.load(n).case, C.load(n).ref, *emulate(C.load(n).case, "nan_dropped"))) > 1.0}
    assert caught == {n for n in C.NAMES if n.startswith(("N-nan_alone_before_finite", "N-nan_alone_first_then_finite", "N-nan_in_empty_row"))}

