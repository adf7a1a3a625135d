"""TEST-ONLY case table, fp64 oracle and derived bound of softmax_ce_kernel<64> / <256> (csrc/rowwise.h, dprhot_softmax_ce_fwd_bwd),
importable without a GPU (helper module like _ivf_cases.py; not a conftest).

ORACLE.  Plain float64 torch on the CPU (`oracle`, on top of _bounds.from_scores): lse, row_loss = lse - S[y + y_offset],
G = (softmax - onehot) * gs.  With a window [lo, hi) = [row_win_start + y_offset, + win_len) the columns outside it count as -inf and
their G is exactly 0, whatever they hold (NaN and +inf included).  Non-finite rows follow torch.nn.functional.cross_entropy
(reduction='none') in fp64 and its autograd on the columns of the window (tests/test_rowwise_conformance.py pins this):
  an all -inf row        lse -inf, loss NaN, G NaN
  a -inf gold            lse finite, loss +inf, G finite with -gs at the gold
  a NaN or +inf inside   lse, loss NaN and the whole G row NaN
A -inf column (and an out-of-window one) has G exactly 0, the gold excepted.

BOUND (u = 2^-24, first order in u like _bounds.py; the logits are given, so eS = 0).  TPR threads share a row, thread t takes the
float4 at columns 4 t + 4 TPR k of trip k, so trips = ceil(Nc / (4 TPR)); the TPR pairs (max, sum) are then combined in
steps = 6 xor-shuffle rounds (TPR 64) plus 3 LDS combines (TPR 256: 9).
  a term      e_j = __expf(S_j - m) relative to the thread's running maximum m at its trip, then one RESCALE every time the maximum it is
              relative to moves: inside the thread at most trips - 1 times (`s *= __expf(m - lm)`, only when the maximum moves), and
              once per combine step (ms_combine rescales both sides, by __expf(0) = 1 where the maximum stays).  R = trips - 1 + steps.
              Each of the 1 + R stages is one __expf, 2u (1 + |x|) relative (_bounds.py, "exp"), and -- but for the first -- one
              multiply, u: at most 3u per stage and 2u |x|.  All the x of one term's path are <= 0 and add up to
              S_j - (final maximum) >= S_j - lse = -gap_j.  So a term is off by at most 3u (1 + R) + 2u gap_j, relative.
  the sum     a term passes at most 4 additions per trip (`s += e0 + e1 + e2 + e3`) and one per combine step:
              gamma(4 trips + steps) relative on a sum of positive terms (gamma with u: plain fp32 additions round to nearest).
  underflow   __expf flushes below 2^-126 and a rescaled sum may: at most (Nc + steps) 2^-126 absolute on s >= 1.
  log, add    lse = m + logf(s): 3u |log s| for logf and u (|m| + |lse|) for the addition.
  e_lse_i  =  sum_j P_ij (3u (1 + R) + 2u gap_ij) + gamma(4 trips + steps) + (Nc + steps) 2^-126 + 3u |log s_i| + u (|m_i| + |lse_i|)
  e_loss_i =  e_lse_i + u |loss_i|                                         (one subtraction of an exact input)
  G           P_ij = __expf(S_ij - lse_i): relative e_lse_i + 2u (1 + gap_ij) + 2u (exp_u = 2 of from_scores); the subtraction of the
              onehot and the scale 2u |G|; P below 2^-126 is flushed (2^-126 |gs|) and so may the product P gs be (2^-126).  The bf16
              value the kernel stores is judged by _bounds.g_scores: the distance the fp64 G would have to move to round (RNE) to it,
              over that bound -- no list of excluded cells.
A measured ratio above 1 means the kernel or this derivation is wrong; no constant multiplies the bound.

CASES (`TABLE`, name -> Case; `load(name)` adds the oracle).  Rows B in {1, 4, 5} (a block holds 4 rows at TPR 64), Nc in NC64 (one
trip = 256 columns; 4096 is the last of TPR 64) and NC256 (one trip = 1024 columns).  Families:
  V  values x every Nc: gauss (sigma 1), peaky (sigma 30: gaps in the hundreds, terms underflow), const, onefinite, up (strictly
     increasing: the maximum moves at every trip of every thread), down.  Gold at column 0, at Nc - 1, in the last partial trip.
  O  y_offset in {8, 5} with rank-local y
  I  -inf columns: scattered, the trailing 1 .. 7 (the loss wrapper's padding), whole aligned groups of 4 and of 8, a -inf gold, a
     whole row
  W  windows: win_len in {1, 3, 8, 13}, lo = 0, hi = Nc, lo not a multiple of 4, with y_offset, with NaN and +inf planted outside
  S  grad_scale in {1 / B, 1.0, -2.5, 2^-20}, with and without G
  N  NaN among finite values; NaN alone in an aligned 4-group of -inf BEFORE and AFTER its thread has seen a finite value; NaN in
     an otherwise all -inf row; +inf.  The poisoned row sits between clean ones."""
import functools
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

import _bounds as Bd

U, TINY = Bd.U, Bd.TINY
NC64 = (8, 16, 248, 256, 264, 1032, 4096)
NC256 = (4104, 5128, 8200)
INF, NAN = math.inf, math.nan


def tpr_of(Nc):
    return 64 if Nc <= 4096 else 256  # dprhot_softmax_ce_fwd_bwd's switch (csrc/dprhot.hip)


def geometry(Nc):
    """(TPR, trips, steps, R) of the module docstring."""
    tpr = tpr_of(Nc)
    trips = -(-Nc // (4 * tpr))
    steps = 6 if tpr == 64 else 9
    return tpr, trips, steps, trips - 1 + steps


class Case(NamedTuple):
    S: np.ndarray                    # fp32 [B, Nc]
    y: np.ndarray                    # int64 [B], rank-local: the gold column is y + y_offset
    y_offset: int
    gs: float
    win_start: Optional[np.ndarray]  # int64 [B], rank-local: the window is [win_start + y_offset, + win_len); None: the whole row
    win_len: int
    want_G: bool
    note: str


# ---- the oracle and the bound ----------------------------------------------------------------------------------------------------------
def e_lse_rowwise(Nc):
    _, trips, steps, R = geometry(Nc)

    def e_lse(P, gap, eS, lse, m, s):
        z = lambda x: x.abs().nan_to_num(0.0, 0.0, 0.0)
        return ((P * (eS + 3 * U * (1 + R) + 2 * U * gap)).sum(1) + Bd.gamma(4 * trips + steps, U) + (Nc + steps) * TINY
                + 3 * U * z(torch.log(s)) + U * (z(m) + z(lse)))

    return e_lse


def window_mask(case):
    """bool [B, Nc]: True outside the row's window."""
    B, Nc = case.S.shape
    if case.win_start is None:
        return np.zeros((B, Nc), dtype=bool)
    lo = (case.win_start + case.y_offset)[:, None]
    col = np.arange(Nc)[None, :]
    return (col < lo) | (col >= lo + case.win_len)


def oracle(case):
    """_bounds.from_scores on the case (mask: outside the window, or -inf) with the non-finite rules of the module docstring laid over
    it.  Adds `outside` [B, Nc], True outside the row's window."""
    S = torch.from_numpy(case.S).to(torch.float64)
    outside = torch.from_numpy(window_mask(case))
    inside = ~outside
    poisoned = ((torch.isnan(S) | (S == INF)) & inside).any(1)
    empty = ((S == -INF) | outside).all(1)
    clean = torch.where((poisoned | empty)[:, None] & inside, torch.zeros_like(S), S)  # (their rows are overwritten below)
    ref = Bd.from_scores(clean, torch.from_numpy(case.y), case.gs, case.y_offset, outside | (S == -INF), e_lse=e_lse_rowwise(S.shape[1]),
                         exp_u=2, g_tiny=TINY)
    nan_g = torch.where(inside, torch.full_like(S, NAN), torch.zeros_like(S))
    bad = poisoned | empty
    ref["lse"] = torch.where(poisoned, NAN, torch.where(empty, -INF, ref["lse"]))
    ref["loss"] = torch.where(bad, NAN, ref["loss"])
    ref["G"] = torch.where(bad[:, None], nan_g, ref["G"])
    ref["outside"] = outside
    return ref


def _rows(ref, keep):
    return {k: (v[keep] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == keep.shape[0] else v) for k, v in ref.items()}


def check(case, ref, row_loss, row_lse, G=None):
    """Scores of one run's outputs (torch tensors on the CPU) against the oracle: worst err / bound of lse, loss and G (inf where a
    finite / non-finite pattern differs), and `words`: 0 when row_loss equals fp32(row_lse - S[row, y + y_offset]) word for word."""
    sc = {"lse": Bd.score_rows(row_lse, ref["lse"], ref["e_lse"]), "loss": Bd.score_rows(row_loss, ref["loss"], ref["e_loss"])}
    gold = case.S[np.arange(len(case.y)), case.y + case.y_offset]
    with np.errstate(invalid="ignore"):
        want = row_lse.numpy().astype(np.float32) - gold
    got = row_loss.numpy()
    same = (want.view(np.uint32) == got.view(np.uint32)) | (np.isnan(want) & np.isnan(got))
    sc["words"] = 0.0 if same.all() else INF
    if G is not None:
        if not Bd.finite_match(G, ref["G"]):
            sc["G"] = INF
        else:
            keep = torch.isfinite(ref["G"]).all(1)
            sc["G"] = float(Bd.g_scores(G[keep], _rows(ref, keep))[0].max()) if keep.any() else 0.0
    return sc


def worst(sc):
    return max(sc.values())


# ---- values ------------------------------------------------------------------------------------------------------------------------------
def _values(kind, B, Nc, g):
    if kind == "gauss":
        return g.standard_normal((B, Nc)).astype(np.float32)
    if kind == "peaky":
        return (30.0 * g.standard_normal((B, Nc))).astype(np.float32)
    if kind == "const":
        return np.repeat((g.integers(-40, 41, size=(B, 1)) / 8.0).astype(np.float32), Nc, axis=1)
    if kind == "up":
        return np.repeat((np.arange(Nc, dtype=np.float32) / 16.0 - 3.0)[None, :], B, axis=0) + np.arange(B, dtype=np.float32)[:, None]
    if kind == "down":
        return _values("up", B, Nc, g)[:, ::-1].copy()
    assert kind == "onefinite"
    return np.full((B, Nc), -INF, dtype=np.float32)


def _golds(B, Nc, g, width=None):
    """Gold at column 0, at the last column, in the last partial trip, then random: one per row."""
    width = Nc if width is None else width
    tpr = tpr_of(Nc)
    last_trip = (width - 1) // (4 * tpr) * (4 * tpr)
    picks = [0, width - 1, min(width - 1, last_trip + (width - last_trip) // 2)]
    y = [picks[i] if i < 3 else int(g.integers(0, width)) for i in range(B)]
    return np.array(y if B > 1 else [picks[2]], dtype=np.int64)


def _case(S, y, note, y_offset=0, gs=None, win_start=None, win_len=0, want_G=True):
    S = np.ascontiguousarray(S, dtype=np.float32)
    B, Nc = S.shape
    gs = float(np.float32(1.0 / B if gs is None else gs))  # the fp32 the kernel is given
    y = np.asarray(y, dtype=np.int64)
    ws = None if win_start is None else np.asarray(win_start, dtype=np.int64)
    assert Nc % 8 == 0 and y.shape == (B,) and ((y + y_offset >= 0) & (y + y_offset < Nc)).all()
    if ws is not None:  # valid inputs only: the window inside the row, the gold inside the window
        lo = ws + y_offset
        assert win_len > 0 and (lo >= 0).all() and (lo + win_len <= Nc).all() and ((y >= ws) & (y < ws + win_len)).all()
    return Case(S, y, int(y_offset), float(gs), ws, int(win_len), bool(want_G), note)


def shape_v(kind, Nc, B, seed):
    g = np.random.default_rng(seed)
    S = _values(kind, B, Nc, g)
    y = _golds(B, Nc, g)
    if kind == "onefinite":  # rows in turn: the gold is the finite column (loss 0) / another one is (a -inf gold: loss +inf)
        for i in range(B):
            S[i, y[i] if i % 2 == 0 else (y[i] + 1 + Nc // 2) % Nc] = np.float32(2.5 - i)
    return _case(S, y, f"{kind} values, B={B} Nc={Nc}")


def shape_o(Nc, y_offset, seed):
    g = np.random.default_rng(seed)
    B = 5
    S = _values("gauss", B, Nc, g)
    return _case(S, _golds(B, Nc, g, Nc - y_offset), f"y_offset={y_offset}, rank-local y, Nc={Nc}", y_offset=y_offset)


def shape_i(kind, Nc, seed, k=0):
    g = np.random.default_rng(seed)
    B = 4
    S = _values("gauss", B, Nc, g)
    y = _golds(B, Nc, g)
    if kind == "scattered":
        S[g.random((B, Nc)) < 0.3] = -INF
        S[np.arange(B), y] = g.standard_normal(B).astype(np.float32)
    elif kind == "trailing":  # what HotCrossEntropyLoss appends when the column count is no multiple of 8
        S[:, Nc - k:] = -INF
        y = _golds(B, Nc, g, Nc - k)
    elif kind == "group4":
        S[:, 4:8] = -INF
        S[1:, Nc - 4:] = -INF
        y = np.array([0, 1, 2, 3], dtype=np.int64)
    elif kind == "group8":
        S[:, 8:16] = -INF
        S[1:, Nc - 8:] = -INF
        y = np.array([0, 1, 2, 3], dtype=np.int64)
    elif kind == "gold":
        S[1, y[1]] = -INF
        S[3, y[3]] = -INF
    else:
        assert kind == "row"
        S[2, :] = -INF
    return _case(S, y, f"-inf columns: {kind}{k or ''}, Nc={Nc}")


def shape_w(Nc, win_len, y_offset, plant, seed):
    g = np.random.default_rng(seed)
    B = 5
    S = _values("gauss", B, Nc, g)
    top = Nc - y_offset - win_len  # largest rank-local start: hi == Nc
    odd = lambda x: min(top, x | 1)  # lo = start + y_offset no multiple of 4 (for y_offset in {0, 8}: an odd lo)
    ws = np.array([0, top, odd(5), odd(top // 2), odd(max(0, top - 6))], dtype=np.int64)
    y = ws + np.array([0, win_len - 1, win_len // 2, 0, win_len - 1], dtype=np.int64)
    if plant:  # NaN and +inf outside the windows change nothing
        out = window_mask(_case(S, y, "", y_offset, None, ws, win_len))
        r, c = np.nonzero(out)
        pick = g.choice(len(r), size=min(len(r), 6 * B), replace=False)
        S[r[pick], c[pick]] = np.where(np.arange(len(pick)) % 2 == 0, NAN, INF).astype(np.float32)
        for i in range(B):  # and right beside the window, inside its float4 / its group of 8
            lo = ws[i] + y_offset
            if lo > 0:
                S[i, lo - 1] = NAN
            if lo + win_len < Nc:
                S[i, lo + win_len] = INF
    return _case(S, y, f"window of {win_len}, y_offset={y_offset}, Nc={Nc}" + (", NaN / +inf outside" if plant else ""), y_offset, None, ws,
                 win_len)


def shape_s(Nc, gs, want_G, seed):
    g = np.random.default_rng(seed)
    B = 5
    S = _values("gauss", B, Nc, g)
    return _case(S, _golds(B, Nc, g), f"grad_scale={gs!r}, G {'wanted' if want_G else 'not wanted'}, Nc={Nc}", gs=gs, want_G=want_G)


N_KINDS = ("nan_among_finite", "nan_alone_before_finite", "nan_alone_after_finite", "nan_alone_first_then_finite", "nan_in_empty_row",
           "pos_inf")


def shape_n(kind, Nc, seed):
    """Row 1 of 4 is poisoned.  `trip` columns are one trip of the row's threads: thread 0 reads columns 0 .. 3 and trip .. trip + 3."""
    g = np.random.default_rng(seed)
    B = 4
    S = _values("gauss", B, Nc, g)
    y = np.array([0, 1, 2, 3], dtype=np.int64)
    trip = 4 * tpr_of(Nc)
    if kind == "nan_among_finite":
        S[1, Nc // 2 + 1] = NAN
    elif kind == "pos_inf":
        S[1, Nc // 2 + 1] = INF
    elif kind == "nan_alone_before_finite":  # thread 1's first float4 is [NaN, -inf, -inf, -inf]: the loss wrapper's Nc = 5
        S[1, 4:8] = [NAN, -INF, -INF, -INF]
    elif kind == "nan_alone_after_finite":   # thread 0 has seen columns 0 .. 3 when it reads this group in its second trip
        assert Nc >= trip + 8
        S[1, trip:trip + 4] = [-INF, -INF, NAN, -INF]
    elif kind == "nan_alone_first_then_finite":  # thread 1: the group first, finite values in its second trip
        assert Nc >= trip + 8
        S[1, 4:8] = [-INF, NAN, -INF, -INF]
    else:
        assert kind == "nan_in_empty_row"
        S[1, :] = -INF
        S[1, 5] = NAN
    return _case(S, y, f"{kind.replace('_', ' ')}, Nc={Nc}")


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
TABLE = {}
_B = (5, 4, 1)
for _i, _nc in enumerate(NC64 + NC256):
    TABLE[f"V-gauss-{_nc}"] = functools.partial(shape_v, "gauss", _nc, _B[_i % 3], 100 + _nc)
for _j, _kind in enumerate(("peaky", "const", "onefinite", "up", "down")):
    for _i, _nc in enumerate((8, 264, 1032, 4096, 4104, 8200)):
        TABLE[f"V-{_kind}-{_nc}"] = functools.partial(shape_v, _kind, _nc, _B[(_i + _j) % 3], 200 + 7 * _j + _nc)
for _nc in (16, 264, 4104):
    for _off in (8, 5):
        TABLE[f"O-off{_off}-{_nc}"] = functools.partial(shape_o, _nc, _off, 300 + _nc + _off)
for _k in range(1, 8):
    TABLE[f"I-trailing{_k}-8"] = functools.partial(shape_i, "trailing", 8, 400 + _k, _k)
TABLE["I-trailing3-264"] = functools.partial(shape_i, "trailing", 264, 411, 3)
TABLE["I-trailing5-4104"] = functools.partial(shape_i, "trailing", 4104, 412, 5)
for _kind in ("scattered", "group4", "group8", "gold", "row"):
    for _nc in (16, 264, 4104):
        TABLE[f"I-{_kind}-{_nc}"] = functools.partial(shape_i, _kind, _nc, 420 + _nc + len(_kind))
for _nc in (16, 264, 4104):
    for _wl in (1, 3, 8, 13):
        TABLE[f"W-len{_wl}-{_nc}"] = functools.partial(shape_w, _nc, _wl, 0, False, 500 + _nc + _wl)
for _nc, _wl, _off in ((264, 3, 8), (264, 13, 5), (4104, 8, 5), (16, 1, 8)):
    TABLE[f"W-len{_wl}-off{_off}-{_nc}"] = functools.partial(shape_w, _nc, _wl, _off, False, 540 + _nc + _wl)
for _nc, _wl, _off in ((16, 3, 0), (264, 13, 0), (264, 8, 5), (4104, 13, 8), (8200, 1, 0)):
    TABLE[f"W-len{_wl}-off{_off}-planted-{_nc}"] = functools.partial(shape_w, _nc, _wl, _off, True, 560 + _nc + _wl)
for _nc in (264, 4104):
    for _gs, _tag in ((None, "1/B"), (1.0, "1"), (-2.5, "-2.5"), (2.0 ** -20, "2^-20")):
        TABLE[f"S-gs{_tag}-{_nc}"] = functools.partial(shape_s, _nc, _gs, True, 600 + _nc)
    TABLE[f"S-noG-{_nc}"] = functools.partial(shape_s, _nc, -2.5, False, 600 + _nc)
for _kind in N_KINDS:
    for _nc in (8, 264, 1032, 8200):
        if _nc == 8 and "finite" in _kind and _kind != "nan_among_finite" and _kind != "nan_alone_before_finite":
            continue  # (these need a second trip)
        TABLE[f"N-{_kind}-{_nc}"] = functools.partial(shape_n, _kind, _nc, 700 + _nc)
NAMES = tuple(TABLE)


class Loaded(NamedTuple):
    name: str
    case: Case
    ref: dict


@functools.lru_cache(maxsize=None)
def load(name):
    """The case with its oracle, computed once and shared (nobody writes into either)."""
    case = TABLE[name]()
    return Loaded(name, case, oracle(case))

