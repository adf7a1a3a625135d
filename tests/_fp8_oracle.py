"""The fp8 dense index by its definition (include/dprhot.h), numpy only: the 256 values of OCP e4m3fn, the row
encode rule and the float64 score.  Nothing here shares code with csrc/dense_fp8.h: the kernel rounds with integer arithmetic on the
float's bits, this file looks the nearest table value up.

e4m3fn: 1 sign bit, 4 exponent bits (bias 7), 3 significand bits; exponent field 0 is the subnormal grid m / 8 * 2^-6; exponent field 15
is an ordinary binade except for significand 7, which is NaN (0x7F, 0xFF); there is no infinity; the largest magnitude is 0x7E = 448."""
import numpy as np


def _value(code):
    s, e, m = code >> 7, (code >> 3) & 15, code & 7
    if e == 15 and m == 7:
        return float("nan")
    mag = m / 8.0 * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
    return -mag if s else mag


TABLE = np.array([_value(c) for c in range(256)], dtype=np.float64)  # value(code); exact in fp32 and bf16 as well
_MAG = TABLE[:127]                                                    # 0 .. 448, ascending
_MID = (_MAG[:-1] + _MAG[1:]) / 2.0                                   # the 126 rounding midpoints (exact in float64)
E_MIN, E_MAX, FMAX = -64, 64, 448.0
NAN_CODES = (0x7F, 0xFF)


def padded_width(d):
    return (int(d) + 31) // 32 * 32


def e4m3fn(y):
    """uint8 codes of the finite float array y: nearest value, ties to the even code, saturating at +-448; -0 keeps its sign."""
    y = np.asarray(y, dtype=np.float64)
    a = np.abs(y)
    idx = np.searchsorted(_MID, a, side="left")  # midpoints strictly below a: the lower neighbour on a tie
    tie = (idx < 126) & (a == _MID[np.minimum(idx, 125)]) & (idx % 2 == 1)
    code = (idx + tie).astype(np.uint8)
    return code | (np.signbit(y).astype(np.uint8) << 7)


def row_scale(x):
    """fp32 [n]: 2^e with e = p - 8 + (f > 1.75), amax = f * 2^p, clamped to [-64, 64]; 1 for a zero row; NaN for a non-finite row."""
    x = np.asarray(x, dtype=np.float32)
    amax = np.abs(np.where(np.isfinite(x), x, 0)).max(axis=1).astype(np.float32)
    bits = amax.view(np.uint32).astype(np.int64)
    e = (bits >> 23) - 127 - 8 + ((bits & 0x7FFFFF) > 0x600000)  # from the bits, not through log2 (a subnormal amax is clamped anyway)
    e = np.where(amax == 0, 0, np.clip(e, E_MIN, E_MAX))
    scale = np.ldexp(np.float32(1), e.astype(np.int32)).astype(np.float32)
    scale[~np.isfinite(x).all(axis=1)] = np.float32("nan")
    return scale


def encode(x):
    """(codes uint8 [n, dp], scale fp32 [n]) of the rows x [n, d] (fp32; bf16 rows are passed widened, which is exact)."""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    scale = row_scale(x)
    ok = np.isfinite(scale)
    codes = np.zeros((n, padded_width(d)), dtype=np.uint8)
    y = x[ok].astype(np.float64) / scale[ok].astype(np.float64)[:, None]  # a power of two: exact
    codes[ok, :d] = e4m3fn(y)
    return codes, scale


def decode(codes, scale):
    """float64 [n, dp]: value(code) * scale."""
    return TABLE[np.asarray(codes)] * np.asarray(scale, dtype=np.float64)[:, None]


def score(qc, qs, cc, cs):
    """float64 [nq, n]: (sum_t value(qc) value(cc)) * qs * cs.  NaN wherever a NaN takes part."""
    with np.errstate(invalid="ignore"):
        acc = TABLE[np.asarray(qc)] @ TABLE[np.asarray(cc)].T
        return acc * np.asarray(qs, dtype=np.float64)[:, None] * np.asarray(cs, dtype=np.float64)[None, :]


def bound(qc, qs, cc, cs):
    """DESIGN.md section 13's bound for one dot product of dp exact products summed in fp32 in any order, rounding to nearest or
    truncating, then scaled by powers of two: 2^-23 (dp + 1) sum_t |q_t c_t| on the decoded operands."""
    dq, dc = np.abs(decode(qc, qs)), np.abs(decode(cc, cs))
    return 2.0 ** -23 * (np.asarray(qc).shape[1] + 1) * (dq @ dc.T)


def grid(rng, n, d):
    """fp32 [n, d] of integers and halves in [-4, 4]: e4m3 with a row scale holds them without loss, every sum of products is exact in
    fp32."""
    return (rng.integers(-8, 9, size=(n, d)) / 2.0).astype(np.float32)


def edge_rows(d):
    """fp32 [m, d] rows for the edges of the rule (d >= 32): f == 1.75 exactly and the next float above it, rounding midpoints of the
    normal and the subnormal grid, +-0, a zero row, a NaN row, an inf row, both ends of the exponent clamp."""
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    rows = []

    def row(*vals):
        r = np.zeros(d, dtype=np.float32)
        r[:len(vals)] = np.array(vals, dtype=np.float32)
        r[len(vals):] = np.resize(np.array(vals, dtype=np.float32), d - len(vals)) * np.float32(0.25)
        rows.append(r)

    row(1.75, -1.0, 0.5, -0.0, 0.0)                                  # f == 1.75: e = p - 8, amax / scale == 448
    row(up(1.75), -1.75, 1.0, 0.3)                                   # the next float: e = p - 7
    row(3.5, up(3.5) * np.float32(0.5), -3.5)
    row(448.0, 25.0, 27.0, 29.0, 31.0, -25.0, -27.0, 416.0 + 16.0)   # scale 1: midpoints (ties to even: 24, 28, 28, 32; 432 -> 448)
    row(256.0, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, -(2.0 ** -10), 2.0 ** -11, 2.0 ** -9, 15 * 2.0 ** -10)  # subnormal midpoints
    row(1.0, -0.0, 0.0, -1.0)
    rows.append(np.zeros(d, dtype=np.float32))                       # amax == 0: scale 1
    rows.append(np.full(d, -0.0, dtype=np.float32))
    nan_row = np.ones(d, dtype=np.float32); nan_row[d // 2] = np.nan
    inf_row = np.ones(d, dtype=np.float32); inf_row[-1] = -np.inf
    rows += [nan_row, inf_row]
    row(2.0 ** 100, 2.0 ** 72, 2.0 ** 73 * 1.5, -(2.0 ** 90), 2.0 ** 60)  # e clamped to 64: saturates at +-448
    row(3.0e38, -3.3e38, 1.0)
    row(2.0 ** -80, 2.0 ** -70, -(2.0 ** -60) * 1.25, 2.0 ** -75)         # e clamped to -64: tiny values in the subnormal grid or 0
    row(1.0e-45, -1.0e-40, 0.0)                                            # fp32 subnormals
    return np.stack(rows)
