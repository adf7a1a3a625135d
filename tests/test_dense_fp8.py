"""The fp8 dense index without a GPU: the oracle of tests/_fp8_oracle.py against torch's float8_e4m3fn cast, the Python layer
(dpr_scale_amd/dense_fp8.py, retrieval.search_shards(quantizer="fp8")) on the CPU stand-in of tests/_dense_fp8_standin.py, the C ABI's
host-side validation and the compiler's resource report for the new kernels."""
import ctypes
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _fp8_oracle as FO  # noqa: E402
import _topk_oracle as TO  # noqa: E402
from _dense_fp8_standin import DenseFP8Kernels  # noqa: E402
from dpr_scale_amd import dense_fp8, retrieval  # noqa: E402

F8 = torch.float8_e4m3fn


# ---------------------------------------------------------------- the oracle against torch ------------------------------------------------
def test_the_value_table_is_torchs_on_every_byte():
    want = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(F8).float().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(want), np.isnan(FO.TABLE)) and [c for c in range(256) if np.isnan(FO.TABLE[c])] == list(FO.NAN_CODES)
    ok = ~np.isnan(want)
    assert np.array_equal(want[ok], FO.TABLE[ok]) and np.array_equal(np.signbit(want[ok]), np.signbit(FO.TABLE[ok]))
    assert FO.TABLE[0x7E] == 448.0 and FO.TABLE[0x01] == 2.0 ** -9 and FO.TABLE[0x08] == 2.0 ** -6 and np.signbit(FO.TABLE[0x80])
    assert np.array_equal(FO.TABLE.astype(np.float32).astype(np.float64)[ok], FO.TABLE[ok])
    assert torch.equal(torch.from_numpy(FO.TABLE[ok]).to(torch.bfloat16).double(), torch.from_numpy(FO.TABLE[ok]))  # exact in bf16


def test_rounding_is_torchs_cast_on_every_value_midpoint_and_neighbour():
    mag = FO.TABLE[:127]
    mids = (mag[:-1] + mag[1:]) / 2
    pts = np.concatenate([mag, mids, np.nextafter(mids.astype(np.float32), np.float32(np.inf)), np.nextafter(mids.astype(np.float32), np.float32(0)),
                          np.random.default_rng(0).uniform(0, 448, 20000)]).astype(np.float32)
    pts = np.concatenate([pts, -pts])
    pts = pts[np.abs(pts) <= 448]
    got = FO.e4m3fn(pts)
    want = torch.from_numpy(pts).to(F8).view(torch.uint8).numpy()
    assert np.array_equal(got, want)
    assert FO.e4m3fn(np.array([25.0, 27.0, 432.0, 2.0 ** -10, 3 * 2.0 ** -10])).tolist() == [0x5C, 0x5E, 0x7E, 0x00, 0x02]  # ties go to the even code
    assert FO.e4m3fn(np.array([449.0, 464.0, 1e9, -1e30])).tolist() == [0x7E, 0x7E, 0x7E, 0xFE]                # saturation, never NaN
    assert FO.e4m3fn(np.array([-0.0, 0.0])).tolist() == [0x80, 0x00]


@pytest.mark.parametrize("d", [32, 100, 768])
def test_encode_on_the_edges_of_the_rule(d):
    x = FO.edge_rows(d)
    codes, scale = FO.encode(x)
    dp = FO.padded_width(d)
    assert codes.shape == (len(x), dp) and codes.dtype == np.uint8 and scale.dtype == np.float32 and not codes[:, d:].any()
    finite = np.isfinite(x).all(axis=1)
    assert np.isnan(scale[~finite]).all() and not codes[~finite].any() and int((~finite).sum()) == 2
    amax = np.abs(x[finite]).max(axis=1).astype(np.float64)
    s = scale[finite].astype(np.float64)
    assert np.array_equal(np.log2(s), np.round(np.log2(s)))                      # powers of two
    free = (np.log2(s) > FO.E_MIN) & (np.log2(s) < FO.E_MAX) & (amax > 0)
    assert bool((amax[free] <= 448 * s[free]).all() and (amax[free] > 448 * s[free] / 2).all())  # the smallest that holds amax
    assert scale[finite][amax == 0].tolist() == [1.0, 1.0]
    assert scale[0] == 2.0 ** -8 and codes[0, 0] == 0x7E and scale[1] == 2.0 ** -7  # f == 1.75 and the next float above it
    assert codes[0, 3] == 0x80 and codes[0, 4] == 0x00                               # -0 stays -0
    # torch's cast of x / scale (an exact division) agrees on every byte where nothing saturates ...
    y = torch.from_numpy(x[finite]) / torch.from_numpy(scale[finite])[:, None]
    sat = (y.abs() > 448).any(dim=1).numpy()
    want = y.to(F8).view(torch.uint8).numpy()
    assert np.array_equal(codes[finite][~sat][:, :d], want[~sat])
    # ... and saturation happens only where the exponent was clamped: there the codes are the cast of the clamped quotient
    assert bool((np.log2(s[sat]) == FO.E_MAX).all()) and int(sat.sum()) == 2
    assert np.array_equal(codes[finite][sat][:, :d], y.clamp(-448, 448).to(F8).view(torch.uint8).numpy()[sat])
    # bf16 rows: the same rule on the widened values
    xb = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    cb, sb = FO.encode(xb)
    fb = np.isfinite(xb).all(axis=1)
    yb = (torch.from_numpy(xb[fb]) / torch.from_numpy(sb[fb])[:, None]).clamp(-448, 448)
    assert np.array_equal(cb[fb][:, :d], yb.to(F8).view(torch.uint8).numpy())


# ---------------------------------------------------------------- DenseFP8Index -----------------------------------------------------------
def _gauss(seed, n, d):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed))


def _write_shards(tmp_path, p, sizes, name="ctx"):
    d = tmp_path / name
    d.mkdir()
    a = 0
    for i, m in enumerate(sizes):
        with open(d / f"reps_{i:04d}.pkl", "wb") as f:
            pickle.dump(p[a:a + m].clone(), f, protocol=4)
        a += m
    assert a == len(p)
    return str(d)


def test_decode_is_exact_in_bf16_and_pads_to_32():
    p = _gauss(0, 50, 100)
    kn = DenseFP8Kernels()
    index = dense_fp8.DenseFP8Index(p, "cpu", kernels=kn, block_rows=16)
    assert kn.calls == [("encode", 16)] * 3 + [("encode", 2)]  # row blocks: the device never holds more than one in fp32
    assert (index.corpus_len, index.d, index.dp) == (50, 100, 128) and index.codes.dtype == torch.uint8 and index.codes.shape == (50, 128)
    assert index.nbytes == 50 * 128 + 50 * 4
    dec = index.decode()
    assert dec.dtype == torch.bfloat16 and dec.shape == (50, 128) and not dec[:, 100:].any()
    want = FO.decode(index.codes.numpy(), index.scale.numpy())
    assert np.array_equal(dec.double().numpy(), want)  # no rounding on the way into bf16
    rel = float(((dec[:, :100].float() - p).norm() / p.norm()) ** 2)
    print(f"relative reconstruction error {rel:.2e}")
    assert rel < 2.0 ** -8  # 3 bits of significand: at most 2^-4 relative per element, 2^-8 squared
    # the bf16 form of the same rows encodes to the same thing as its widened values
    ib = dense_fp8.DenseFP8Index(p.to(torch.bfloat16), "cpu", kernels=DenseFP8Kernels())
    cb, sb = FO.encode(p.to(torch.bfloat16).float().numpy())
    assert np.array_equal(ib.codes.numpy(), cb) and np.array_equal(ib.scale.numpy(), sb)


def test_from_dirs_round_trips_through_pickles(tmp_path):
    p = _gauss(1, 70, 40)
    path = _write_shards(tmp_path, p, [30, 25, 15])
    index = dense_fp8.DenseFP8Index.from_dirs(path, "cpu", kernels=DenseFP8Kernels())
    direct = dense_fp8.DenseFP8Index(p, "cpu", kernels=DenseFP8Kernels())
    assert index.corpus_len == 70 and index.d == 40 and index.dp == 64 and index.exact_rows is None
    assert torch.equal(index.codes, direct.codes) and torch.equal(index.scale, direct.scale)  # rows concatenated only
    kept = dense_fp8.DenseFP8Index.from_dirs(path, "cpu", kernels=DenseFP8Kernels(), keep_exact=True)
    assert torch.equal(kept.exact_rows, p)
    q = _gauss(2, 3, 40)
    v, i = index.search(q, 10)
    qc, qs = FO.encode(q.numpy())
    S = FO.score(qc, qs, index.codes.numpy(), index.scale.numpy()).astype(np.float32)
    tv, ti = TO.fold(None, S, 0, 10)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and np.array_equal(v.numpy(), tv) and np.array_equal(i.numpy(), ti)
    assert np.array_equal(index.score(q, 5, 33).numpy(), S[:, 5:38])
    with pytest.raises(FileNotFoundError):
        dense_fp8.DenseFP8Index.from_dirs(str(tmp_path), "cpu", kernels=DenseFP8Kernels())


def test_save_and_load(tmp_path):
    p = _gauss(3, 33, 48)
    index = dense_fp8.DenseFP8Index(p, "cpu", kernels=DenseFP8Kernels())
    path = str(tmp_path / "index.pt")
    index.save(path)
    blob = torch.load(path, weights_only=True)
    assert blob["format"] == "dpr_scale_amd.dense_fp8/1" and blob["d"] == 48 and set(blob) == {"format", "d", "codes", "scale"}
    back = dense_fp8.DenseFP8Index.load(path, "cpu", kernels=DenseFP8Kernels())
    assert (back.corpus_len, back.d, back.dp) == (33, 48, 64) and torch.equal(back.codes, index.codes) and torch.equal(back.scale, index.scale)
    q = _gauss(4, 2, 48)
    assert all(torch.equal(a, b) for a, b in zip(back.search(q, 5), index.search(q, 5)))
    again = dense_fp8.DenseFP8Index.from_codes(index.codes, index.scale, 48, kernels=DenseFP8Kernels())
    assert torch.equal(again.decode(), index.decode())
    torch.save({"format": "something/else"}, path)
    with pytest.raises(ValueError, match="dense_fp8/1"):
        dense_fp8.DenseFP8Index.load(path, "cpu")
    with pytest.raises(ValueError, match="codes"):
        dense_fp8.DenseFP8Index.from_codes(index.codes, index.scale, 70)
    with pytest.raises(ValueError, match="scale"):
        dense_fp8.DenseFP8Index.from_codes(index.codes, index.scale[:-1], 48)


def test_id_range_folds_equal_one_search():
    p, q = _gauss(5, 70, 32), _gauss(6, 4, 32)
    p[17] = float("nan")  # a non-finite row: scale NaN, never selected
    index = dense_fp8.DenseFP8Index(p, "cpu", kernels=DenseFP8Kernels())
    assert bool(torch.isnan(index.scale[17])) and not index.codes[17].any()
    v, i = index.search(q, 30)
    assert not bool((i == 17).any())
    for ranges, chunk in (([(0, 70)], 8), ([(0, 33), (33, 70)], 16), ([(41, 70), (0, 9), (9, 41)], None)):
        v2, i2 = index.search(q, 30, id_ranges=ranges, chunk=chunk)
        assert torch.equal(v, v2) and torch.equal(i, i2), ranges
    kn = index.kn  # few queries: an empty state starts from a head of at most index.head ids, a range of its own -- the same result
    index.head = 24
    kn.calls.clear()
    v2, i2 = index.search(q, 30, id_ranges=[(3, 70), (0, 3)])
    assert [c for c in kn.calls if c[0] == "search"] == [("search", 24), ("search", 43), ("search", 3)]
    w, j = index.search(q, 30, id_ranges=[(3, 70), (0, 3)], chunk=8)
    assert torch.equal(v, v2) and torch.equal(i, i2) and torch.equal(v, w) and torch.equal(i, j)
    kn.calls.clear()
    many = index.search(torch.cat([q] * 9), 30)  # 36 queries: one range
    assert [c for c in kn.calls if c[0] == "search"] == [("search", 70)] and torch.equal(many[1][:4], i)
    index.head = dense_fp8.HEAD_IDS
    v3, i3 = index.search(q, 30, id_ranges=[(10, 25)])  # fewer candidates than topk (one of them NaN): the tail stays unfilled
    assert bool((i3[:, 14:] == -1).all()) and bool(torch.isinf(v3[:, 14:]).all()) and bool((i3[:, :14] >= 10).all())
    for k in (0, 71):
        with pytest.raises(ValueError, match="topk"):
            index.search(q, k)
    with pytest.raises(ValueError, match="do not fit"):
        index.search(q[:, :8], 5)


def test_refine_returns_the_definitions_result_and_needs_exact_rows():
    n, d, nq, k, r = 200, 64, 5, 7, 4
    p, q = _gauss(7, n, d), _gauss(8, nq, d)
    p[100:110] = p[3]  # exact ties in the refined score: the lower id first
    index = dense_fp8.DenseFP8Index(p, "cpu", kernels=DenseFP8Kernels(), exact_rows=p)
    v, i = index.search(q, k, refine=r)
    _, cand = index.search(q, r * k)  # the definition: the fp8 top r * k, re-scored in fp32 on the exact rows, (score desc, id asc)
    for row in range(nq):
        ids = np.sort(cand[row].numpy())
        s = (p[ids] * q[row][None, :]).sum(-1).numpy()
        order = np.lexsort((ids, -s.astype(np.float64)))[:k]
        assert i[row].tolist() == ids[order].tolist() and np.array_equal(v[row].numpy(), s[order])
    assert v.shape == (nq, k) and v.dtype == torch.float32 and i.dtype == torch.int64
    va, ia = index.search(q, k, refine=1000)  # every passage is a candidate: the exact fp32 top-k
    S = (p[None, :, :] * q[:, None, :]).sum(-1).numpy()
    tv, ti = TO.fold(None, S, 0, k)
    assert np.array_equal(ia.numpy(), ti) and np.array_equal(va.numpy(), tv)
    vb, ib = index.search(q, 12, id_ranges=[(20, 30)], refine=2)  # fewer candidates than topk: -inf / -1 behind them
    assert bool((ib[:, 10:] == -1).all()) and bool(torch.isinf(vb[:, 10:]).all()) and bool(((ib[:, :10] >= 20) & (ib[:, :10] < 30)).all())
    bf = dense_fp8.DenseFP8Index(p, "cpu", kernels=DenseFP8Kernels(), exact_rows=p.to(torch.bfloat16))
    vc, ic = bf.search(q, k, refine=r)
    assert vc.dtype == torch.float32 and ic.shape == (nq, k)
    plain = dense_fp8.DenseFP8Index(p, "cpu", kernels=DenseFP8Kernels())
    with pytest.raises(ValueError, match="exact_rows"):
        plain.search(q, k, refine=2)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="refine"):
            index.search(q, k, refine=bad)
    with pytest.raises(ValueError, match="exact_rows"):
        dense_fp8.DenseFP8Index(p, "cpu", kernels=DenseFP8Kernels(), exact_rows=p[:-1])


@pytest.mark.parametrize("shard", [1, 2])
def test_search_shards_fp8_equals_the_bf16_path_on_a_grid_corpus(shard, tmp_path):
    rng = np.random.default_rng(9)
    p, q = torch.from_numpy(FO.grid(rng, 90, 48)), torch.from_numpy(FO.grid(rng, 6, 48))
    cp, sp = FO.encode(p.numpy())
    assert np.array_equal(FO.decode(cp, sp)[:, :48], p.double().numpy())  # e4m3 with a row scale holds the grid without loss
    path = _write_shards(tmp_path, p, [25, 25, 25, 15])  # a short last file: the reference's zero vectors and id offsets
    kn = DenseFP8Kernels()
    want_v, want_i = retrieval.search_shards(q, path, 20, shard=shard, device="cpu", kernels=kn)
    got_v, got_i = retrieval.search_shards(q, path, 20, shard=shard, device="cpu", kernels=kn, quantizer="fp8")
    assert torch.equal(got_v, want_v) and torch.equal(got_i, want_i)
    assert int(want_i.max()) >= 90 - 15  # ids run over all shards
    with pytest.raises(ValueError, match="quantizer"):
        retrieval.search_shards(q, path, 20, device="cpu", kernels=kn, quantizer="int8")


# ---------------------------------------------------------------- ABI --------------------------------------------------------------------
_ONE = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch
_GOOD = dict(Qc=_ONE, qs=_ONE, nq=2, Cc=_ONE, cs=_ONE, n=100, dp=64, b=0, e=100, k=5, chunk=64, vals=_ONE, idx=_ONE, first=1, ws=_ONE, wsb=1 << 20,
             st=None)
_BAD = [  # (what is wrong, code, a word of the error text)
    (dict(Qc=None), -1, b"NULL"), (dict(qs=None), -1, b"NULL"), (dict(Cc=None), -1, b"NULL"), (dict(cs=None), -1, b"NULL"),
    (dict(vals=None), -1, b"NULL"), (dict(idx=None), -1, b"NULL"),
    (dict(Qc=ctypes.c_void_p(264)), -1, b"aligned"), (dict(Cc=ctypes.c_void_p(260)), -1, b"aligned"), (dict(cs=ctypes.c_void_p(258)), -1, b"aligned"),
    (dict(ws=ctypes.c_void_p(264)), -1, b"aligned"),
    (dict(dp=48), -1, b"multiple of 32"), (dict(dp=0), -1, b"multiple of 32"),
    (dict(nq=0), -1, b"queries"), (dict(nq=-3), -1, b"queries"),
    (dict(nq=1 << 20, chunk=1 << 20), -1, b"candidate slots"),
    (dict(n=0), -1, b"n_ctx"), (dict(n=1 << 31, e=1 << 31), -1, b"n_ctx"),
    (dict(k=0), -1, b"topk"), (dict(k=101), -1, b"topk"),
    (dict(b=50, e=40), -1, b"range"), (dict(b=7, e=7), -1, b"range"), (dict(e=101), -1, b"range"), (dict(b=-1), -1, b"range"),
    (dict(chunk=12), -1, b"chunk"), (dict(chunk=0), -1, b"chunk"),
    (dict(ws=None), -4, b"workspace"), (dict(wsb=16), -4, b"workspace"),
    (dict(n=6000, e=6000, k=5000, wsb=2 * 64 * 8 + 256), -4, b"workspace"),  # k > 4096: the wide selection's state is missing
]


def test_abi_exports_binds_and_validates_on_the_host():
    from dpr_scale_amd import _lib

    lib = _lib.lib
    for s in ("dprhot_fp8_encode", "dprhot_dense_fp8_workspace_bytes", "dprhot_dense_fp8_score", "dprhot_dense_fp8_search"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert _lib.dense_fp8_workspace_bytes(4, 64) == 4 * 64 * 8 + 256 == _lib.search_workspace_bytes(4, 64)
    out = ctypes.c_size_t(0)
    for args, word in (((0, 64), b"queries"), ((2, 12), b"chunk"), ((2, 0), b"chunk"), ((1 << 20, 1 << 20), b"candidate slots")):
        assert lib.dprhot_dense_fp8_workspace_bytes(*args, ctypes.byref(out)) == -1 and word in lib.dprhot_last_error(), args
    assert lib.dprhot_dense_fp8_workspace_bytes(2, 64, None) == -1
    for bad, code, word in _BAD:
        assert set(bad) <= set(_GOOD), bad
        rc = lib.dprhot_dense_fp8_search(*[bad.get(k, v) for k, v in _GOOD.items()])
        err = lib.dprhot_last_error()
        assert rc == code and word in err, (bad, rc, err)
        if code == -4:
            assert b"dense_fp8_search needs" in err and b"dprhot_dense_fp8_workspace_bytes" in err, err
            assert (b"dprhot_topk_wide_workspace_bytes" in err) == ("k" in bad), err
    S = dict(Qc=_ONE, qs=_ONE, nq=2, Cc=_ONE, cs=_ONE, n=100, dp=64, db=0, cols=10, S=_ONE, ld=16, st=None)
    for bad, word in ((dict(S=None), b"NULL"), (dict(cols=0), b"cols"), (dict(ld=8), b"ld"), (dict(ld=12), b"multiple of 8"), (dict(db=95), b"corpus"),
                      (dict(S=ctypes.c_void_p(260)), b"aligned"), (dict(dp=40), b"multiple of 32"), (dict(qs=None), b"NULL")):
        rc = lib.dprhot_dense_fp8_score(*[bad.get(k, v) for k, v in S.items()])
        assert rc == -1 and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())
    E = dict(rows=_ONE, bf=0, n=10, d=100, dp=128, codes=_ONE, scale=_ONE, st=None)
    for bad, word in ((dict(rows=None), b"NULL"), (dict(codes=None), b"NULL"), (dict(scale=None), b"NULL"), (dict(codes=ctypes.c_void_p(264)), b"aligned"),
                      (dict(rows=ctypes.c_void_p(258)), b"aligned"), (dict(scale=ctypes.c_void_p(258)), b"aligned"), (dict(dp=100), b"multiple of 32"),
                      (dict(d=129), b"d=129"), (dict(d=0), b"d=0"), (dict(n=0), b"rows"), (dict(n=1 << 31), b"rows")):
        rc = lib.dprhot_fp8_encode(*[bad.get(k, v) for k, v in E.items()])
        assert rc == -1 and word in lib.dprhot_last_error(), (bad, lib.dprhot_last_error())


# ---------------------------------------------------------------- resources --------------------------------------------------------------
def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    report = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
    assert os.path.isfile(report), "the library's Makefile writes the compiler's resource report next to it"
    cur, rows = None, {}
    for ln in open(report, errors="replace"):
        m = re.search(r" Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)", ln)
        if m and cur:
            rows[cur][m.group(1)] = int(m.group(2))
    mine = {k: v for k, v in rows.items() if "11dfp8_kernel" in k or "17fp8_encode_kernel" in k}
    assert len(mine) == 6, sorted(mine)  # the store and the filter epilogue on the 128- and the 32-query tile; fp32 and bf16 rows
    for name, r in mine.items():
        assert r == {"ScratchSize [bytes/lane]": 0, "SGPRs Spill": 0, "VGPRs Spill": 0}, (name, r)
