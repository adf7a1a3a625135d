"""Product-quantised postings on the CPU: pq_decode, the numpy restatement of the encode rule against a
float64 argmin, host-side validation of the three new entry points, the drop-in CITADELPQRetrievalTask's scope and the compiler's
resource report of the new kernels."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _pq_oracle as PO  # noqa: E402
from dpr_scale_amd import ivf  # noqa: E402

REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")


def _bf16_values(a):
    return torch.from_numpy(a).to(torch.bfloat16).float().numpy()


@pytest.mark.parametrize("dsub,m", [(2, 16), (4, 8), (8, 8)])
def test_pq_decode_against_a_loop(dsub, m):
    g = torch.Generator().manual_seed(dsub)
    codebook = torch.randn(m, 256, dsub, generator=g).to(torch.bfloat16)
    codes = torch.randint(0, 256, (37, m), generator=g).to(torch.uint8)
    codes[0], codes[1] = 0, 255
    got = ivf.pq_decode(codes, codebook)
    assert got.dtype == torch.bfloat16 and got.shape == (37, m * dsub)
    assert np.array_equal(got.float().numpy(), PO.decode(codes.numpy(), codebook.float().numpy()))
    assert ivf.pq_decode(codes[:0], codebook).shape == (0, m * dsub)
    with pytest.raises(ValueError, match="codes"):
        ivf.pq_decode(codes[:, :-1], codebook)


@pytest.mark.parametrize("dsub", [2, 4, 8])
def test_encode_rule_agrees_with_a_float64_argmin(dsub):
    g = np.random.default_rng(100 + dsub)
    m = 32 // dsub
    x = _bf16_values(g.standard_normal((400, 32)).astype(np.float32))
    cb = _bf16_values(g.standard_normal((m, 256, dsub)).astype(np.float32))
    cb[0, 9], cb[0, 200] = cb[0, 4], cb[0, 4]  # equal centroids: an exact tie wherever one of them is nearest
    x[7:12, :dsub] = cb[0, 4]
    x[5] = np.nan
    codes = PO.encode(x, cb)
    D = PO.distances64(x, cb)
    srt = np.sort(D, -1)
    unique = srt[..., 0] < srt[..., 1]  # (False for the NaN row as well)
    assert unique.mean() > 0.9
    assert np.array_equal(codes[unique], D.argmin(-1)[unique])
    assert codes[7, 0] == 4 and not codes[5].any()
    # a tie goes to the lowest index, also when the first of the equal centroids is not centroid 0
    tied = D[:, 0, 4] == np.where(np.isnan(D[:, 0, :]), np.inf, D[:, 0, :]).min(-1)
    assert tied.sum() >= 5 and (codes[tied, 0] == 4).all() and (codes[:, 0] != 9).all() and (codes[:, 0] != 200).all()


def test_abi_and_host_validation():
    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import HipKernels

    assert _lib.version() == 174
    for s in ("dprhot_pq_encode", "dprhot_ivf_pq_score", "dprhot_ivf_pq_search"):
        assert hasattr(_lib.lib, s) and s in _lib.SIGNATURES
    assert callable(HipKernels.pq_encode) and callable(HipKernels.ivf_pq_score) and callable(HipKernels.ivf_pq_search)
    lib = _lib.lib
    one = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch
    INVALID, UNSUPPORTED = -1, -3

    def named(defaults, kw):
        assert set(kw) <= set(defaults), kw
        return [kw.get(k, v) for k, v in defaults.items()]

    enc = lambda **kw: lib.dprhot_pq_encode(*named(dict(vec=one, n=10, dp=32, cb=one, dsub=4, codes=one, st=None), kw))
    score = lambda **kw: lib.dprhot_ivf_pq_score(*named(dict(
        pc=one, cb=one, dsub=4, pd=one, eo=one, P=10, V=4, dp=32, ev=one, eq=one, ne=2, be=one, bo=one, nb=1, nq=1, b=0, cols=64, S=one,
        ld=64, st=None), kw))
    search = lambda **kw: lib.dprhot_ivf_pq_search(*named(dict(
        pc=one, cb=one, dsub=4, pd=one, eo=one, P=10, V=4, dp=32, ev=one, eq=one, ne=2, be=one, bo=one, nb=1, nq=1, cq=None, cd=None, dc=0,
        cr=0, n=100, b=0, e=100, k=5, chunk=64, vals=one, idx=one, first=1, ws=one, wsb=1 << 20, st=None), kw))
    for f, nulls in ((enc, ("vec", "cb", "codes")), (score, ("pc", "cb", "pd", "eo", "ev", "S")), (search, ("pc", "cb", "pd", "eo", "vals", "ws"))):
        for name in nulls:
            rc = f(**{name: None})
            assert rc == (-4 if name == "ws" else INVALID), (f, name, rc)
        assert f(dsub=3) == INVALID and b"dsub" in lib.dprhot_last_error()
        assert f(dsub=0) == INVALID and f(dsub=16) == INVALID
        assert f(dp=48) == INVALID and b"multiple of 32" in lib.dprhot_last_error()
        assert f(dp=0) == INVALID
        assert f(dp=128) == UNSUPPORTED and b"dp=128" in lib.dprhot_last_error()
        assert f(dp=96) == UNSUPPORTED
    assert enc(n=-1) == INVALID
    assert enc(n=0, vec=None, codes=None) == 0  # nothing to encode: nothing is launched
    assert score(cb=ctypes.c_void_p(264)) == INVALID and b"aligned" in lib.dprhot_last_error()
    # the limits of the dense entry points hold unchanged
    assert search(n=2 ** 31) == INVALID and b"corpus_len" in lib.dprhot_last_error()
    assert search(P=2 ** 40) == INVALID and search(k=0) == INVALID and search(k=101) == INVALID
    assert search(ne=4097) == INVALID and b"entries per query" in lib.dprhot_last_error()
    assert search(chunk=12) == INVALID and search(b=50, e=40) == INVALID
    assert search(cq=one, cd=one, dc=16, cr=100) == INVALID and b"cls_doc" in lib.dprhot_last_error()
    assert search(wsb=16) == -4
    assert score(b=2 ** 31 - 10) == INVALID
    # an empty batch and an index without postings launch nothing (no device is touched: this runs without one)
    assert score(ne=0, nb=0) == 0 and score(P=0) == 0


def test_python_side_refuses_what_the_kernels_do_not_take():
    rows = torch.zeros((4, 32), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="sub_vec_dim"):
        ivf.train_pq(rows, dsub=3)
    with pytest.raises(NotImplementedError, match="at most 64"):
        ivf.train_pq(torch.zeros((4, 128), dtype=torch.bfloat16), dsub=4)
    with pytest.raises(ValueError, match="codebook"):
        ivf.IVFPQIndex.from_packed(torch.zeros(4, dtype=torch.int32), torch.zeros((4, 8), dtype=torch.uint8),
                                   torch.zeros((8, 256, 4)), torch.zeros(2, dtype=torch.int64), None, 10, 32)
    with pytest.raises(TypeError):
        ivf.IVFPQIndex()
    for f in (ivf.load_index, ivf.IndexBuilder.finish):
        p = inspect.signature(f).parameters
        assert p["quantizer"].default is None and p["sub_vec_dim"].default == 4


def test_pq_index_surface_and_nbytes():
    P, m, dsub = 10, 8, 4
    pq = ivf.IVFPQIndex.from_packed(torch.zeros(P, dtype=torch.int32), torch.zeros((P, m), dtype=torch.uint8),
                                    torch.zeros((m, 256, dsub), dtype=torch.bfloat16), torch.tensor([0, P]), None, 7, 30)
    assert (pq.dp, pq.d, pq.dsub, pq.n_postings, pq.n_experts, pq.dc) == (32, 30, 4, P, 1, 0)
    assert pq.nbytes == P * 4 + P * m + m * 256 * dsub * 2 + 2 * 8
    for name in ("search", "search_packed", "default_chunk", "latency", "decode", "save"):
        assert hasattr(pq, name)
    assert not hasattr(pq, "post_vec") and pq.default_chunk(4) == 8
    dense = pq.decode()
    assert type(dense) is ivf.IVFIndex and dense.post_vec.shape == (P, 32) and dense.nbytes == P * 4 + P * 64 + 2 * 8


def test_dropin_pq_task_scope():
    from dpr_scale_amd.task.citadel_retrieval import CITADELPQRetrievalTask, CITADELRetrievalTask

    base = dict(ctx_embeddings_dir="x", checkpoint_path="", transform=None, model=None, datamodule=None, optim=None)
    for dsub in (2, 4, 8):
        task = CITADELPQRetrievalTask(quantizer="pq", sub_vec_dim=dsub, **base)
        assert task.quantizer == "pq" and task.sub_vec_dim == dsub and task.save_quantized is False
    assert CITADELPQRetrievalTask._eval_step is CITADELRetrievalTask._eval_step
    with pytest.raises(NotImplementedError, match="sub_vec_dim=3"):
        CITADELPQRetrievalTask(quantizer="pq", sub_vec_dim=3, **base)
    with pytest.raises(NotImplementedError, match="cuda=False"):
        CITADELPQRetrievalTask(quantizer="pq", cuda=False, **base)
    with pytest.raises(NotImplementedError, match="portion=0.5"):
        CITADELPQRetrievalTask(quantizer="pq", portion=0.5, **base)
    with pytest.raises(NotImplementedError, match="hnsw_index=True"):
        CITADELPQRetrievalTask(quantizer="pq", hnsw_index=True, **base)
    with pytest.raises(NotImplementedError, match="quantizer"):
        CITADELPQRetrievalTask(quantizer="sq", **base)
    with pytest.raises(NotImplementedError, match="product quantisation"):  # the plain class is as it was
        CITADELRetrievalTask(quantizer="pq", **base)
    a = inspect.signature(CITADELRetrievalTask.__init__).parameters
    b = inspect.signature(CITADELPQRetrievalTask.__init__).parameters
    assert b["quantizer"].default == "pq" and b["sub_vec_dim"].default == a["sub_vec_dim"].default == 4


def test_pq_kernels_never_spill():
    cur, rows = None, {}
    for ln in open(REPORT, errors="replace"):
        m = re.search(r" Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur:
            rows[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    score = {k: v for k, v in rows.items() if re.search(r"dprhot\d+ivf_pq_score_kernel", k)}
    encode = {k: v for k, v in rows.items() if re.search(r"dprhot\d+pq_encode_kernel", k)}
    assert len(score) == 6 and len(encode) == 3, sorted(rows)  # dsub in {2, 4, 8} x dp in {32, 64}; dsub in {2, 4, 8}
    for name, r in {**score, **encode}.items():
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
    # the 32 KiB table plus the codebook, dp * 512 bytes
    assert sorted(r["LDS Size"] for r in score.values()) == [32768 + 32 * 512] * 3 + [32768 + 64 * 512] * 3
