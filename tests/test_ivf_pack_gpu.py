"""dprhot_ivf_compact / dprhot_ivf_gather on the GPU against the test-only torch stand-in (tests/_ivf_pack_standin.py), bit for bit:
the compaction at every size around the 64-slot step of a wave and around the four-sequence workgroup, the gather's rounding chain in
the three input formats, guard bands around every output, and the builders end to end on the fixtures the reference's own writer and
query step produced.  Every comparison is torch.equal; nothing here has a tolerance."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ivf_fixture as F  # noqa: E402
import _ivf_pack_inputs as I  # noqa: E402
from _ivf_pack_standin import IvfPackKernels  # noqa: E402

pytestmark = pytest.mark.gpu

WITNESS = 1 + 2.0 ** -8 + 2.0 ** -12  # -> 1.0 through fp16 and then bf16, -> 1 + 2^-7 straight to bf16
# (L, K): L K = 1, 63, 64 (2-D ids and K = 8), 65, 129, 520 = 65 x 8
SLOT_SHAPES = [(1, 1), (63, 1), (64, 1), (8, 8), (65, 1), (129, 1), (65, 8)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def kn():
    from dpr_scale_amd.hotpath import HipKernels

    return HipKernels()


def _bits(t):
    t = t.cpu()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _compact_case(seed, B, L, K, kind):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 30522, (B, L, K), generator=g)
    w = torch.rand(B, L, K, generator=g)
    w = torch.where(torch.rand(B, L, K, generator=g) < 0.3, torch.full_like(w, 0.25), w)  # many weights EQUAL the threshold 0.25
    lens = torch.randint(0, L + 1, (B,), generator=g)
    att = (torch.arange(L)[None, :] < lens[:, None]).long()
    if kind == "all_kept":
        w, att = w + 1.0, torch.ones(B, L, dtype=torch.long)
    elif kind == "none_kept":
        w = torch.full_like(w, 0.25)
    elif kind == "one_padding_sequence":
        att[B // 2] = 0
    rows = torch.randint(0, 2 ** 31 - 1, (B,), generator=g)
    return ids, w, att, rows


def _check_compact(kn, dev, ids, w, att, rows, test, minw):
    want = IvfPackKernels().ivf_compact(ids, w, att, rows, test, minw)
    got = kn.ivf_compact(ids.to(dev), None if w is None else w.to(dev), att.to(dev), rows.to(dev), test, minw)
    assert got[:2] == want[:2], (got[:2], want[:2])
    for a, b, what in zip(got[2:], want[2:], ("seq_off", "expert", "row", "slot", "weight")):
        assert _same(a, b), what
    return want[0]


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("L,K", SLOT_SHAPES)
def test_compact_matches_the_standin(kn, dev, B, L, K):
    total = 0
    for j, kind in enumerate(("random", "one_padding_sequence", "all_kept", "none_kept")):
        ids, w, att, rows = _compact_case(100 * B + 10 * L + K + j, B, L, K, kind)
        n = _check_compact(kn, dev, ids, w, att, rows, True, 0.25)  # strict: a weight equal to the threshold is dropped
        assert (kind != "none_kept" or n == 0) and (kind != "all_kept" or n == B * L * K)
        total += n
        _check_compact(kn, dev, ids, w, att, rows, False, 0.0)      # attention only
        _check_compact(kn, dev, ids, None, att, rows, True, 0.0)    # NULL weights: every weight is 1
    assert total > 0


def test_compact_drops_nan_weights_and_keeps_2d_ids(kn, dev):
    from dpr_scale_amd import ivf

    qr = I.gaussian_repr(3, B=3, L=70, K=1, d=8, coil=True)
    qr["expert_weights"][1, 2] = float("nan")
    x, ids, w, att, coil = ivf._slots(qr)
    assert coil and ids.shape == (3, 70, 1)
    rows = torch.arange(3)
    n = _check_compact(kn, dev, ids, w, att, rows, True, 0.0)
    assert n < int(att.sum())  # NaN > 0 is false


class _Guards:
    """torch.empty for HIP tensors, replaced: the tensor is the interior of a larger byte buffer filled with a pattern."""
    GUARD, PATTERN = 4096, 0xA5

    def __init__(self):
        self.orig, self.regions = torch.empty, []

    def empty(self, *size, dtype=None, device=None, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        size = tuple(int(s) for s in size)
        dt = dtype if dtype is not None else torch.get_default_dtype()
        n = int(math.prod(size)) * self.orig((), dtype=dt).element_size()
        if device is None or torch.device(device).type != "cuda" or kw or n == 0:
            return self.orig(size, dtype=dtype, device=device, **kw)
        raw = torch.full((n + 2 * self.GUARD,), self.PATTERN, dtype=torch.uint8, device=device)
        self.regions.append((raw, n))
        return raw[self.GUARD:self.GUARD + n].view(dt).view(size)

    def check(self):
        torch.cuda.synchronize()
        for raw, n in self.regions:
            assert bool((raw[:self.GUARD] == self.PATTERN).all()), f"bytes BEFORE a {n}-byte buffer were overwritten"
            assert bool((raw[self.GUARD + n:] == self.PATTERN).all()), f"bytes BEHIND a {n}-byte buffer were overwritten"
        return len(self.regions)


@pytest.mark.parametrize("B,L,K", [(3, 65, 8), (70, 129, 1), (1, 1, 1)])
def test_outputs_sit_between_intact_guard_bands(kn, dev, monkeypatch, B, L, K):
    ids, w, att, rows = _compact_case(7, B, L, K, "random")
    if B == 1:
        att[:] = 1
        w[:] = 1.0
    want = IvfPackKernels().ivf_compact(ids, w, att, rows, True, 0.25)
    n = want[0]
    assert n > 0
    g = _Guards()
    monkeypatch.setattr(torch, "empty", g.empty)
    args = (ids.to(dev), w.to(dev), att.to(dev), rows.to(dev))
    got = kn.ivf_compact(*args, True, 0.25, capacity=n)  # record arrays of exactly n entries
    short = kn.ivf_compact(*args, True, 0.25, capacity=n // 2)  # fewer: the records beyond are not written, n is still reported
    x = torch.randn(B, L, 20, generator=torch.Generator().manual_seed(1))
    outs = [kn.ivf_gather(x.to(dev), w.to(dev), got[5], None, K, True, torch.bfloat16, 32),
            kn.ivf_gather(x.to(dev), w.to(dev), got[5], None, K, False, torch.float32, None)]
    assert g.check() >= 5 + 5 + 2
    monkeypatch.undo()
    assert got[0] == n == short[0] and short[3].shape[0] == n // 2
    for a, b, c in zip(got[2:], want[2:], short[2:]):
        assert _same(a, b) and _same(c[: n // 2], b[: n // 2])
    ref = IvfPackKernels()
    assert _same(outs[0], ref.ivf_gather(x, w, want[5], None, K, True, torch.bfloat16, 32))
    assert _same(outs[1], ref.ivf_gather(x, w, want[5], None, K, False, torch.float32, None))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_gather_matches_the_standin(kn, dev, dtype):
    ref = IvfPackKernels()
    g = torch.Generator().manual_seed(17)
    B, L, K = 6, 11, 3
    for d in (20, 32, 40, 128):
        x = torch.randn(B, L, d, generator=g)
        x[0, 0, :3] = torch.tensor([3.0e-6, -2.0e-7, 6.0e-5])  # products in and below fp16's subnormal range
        x, w = x.to(dtype), torch.rand(B, L, K, generator=g).to(dtype)
        xd, wd = x.to(dev), w.to(dev)
        for n in (0, 1, 63, 64, 65, 1000):
            slot = torch.randint(0, B * L * K, (n,), generator=g).to(torch.int32)
            if n:
                slot[0] = 1  # token row 0
            for perm in (None, torch.arange(n), torch.arange(n - 1, -1, -1)):
                pd = None if perm is None else perm.to(dev)
                for entry16 in (False, True):
                    for out_dtype, ld in ((torch.float32, d), (torch.bfloat16, (d + 31) // 32 * 32)):
                        got = kn.ivf_gather(xd, wd, slot.to(dev), pd, K, entry16, out_dtype, ld)
                        assert got.shape == (n, ld)
                        assert _same(got, ref.ivf_gather(x, w, slot, perm, K, entry16, out_dtype, ld)), (d, n, entry16, out_dtype)
                        assert not got[:, d:].float().any()
        # NULL weights: the rows as they are, K = 1
        slot = torch.arange(B * L, dtype=torch.int32)
        assert _same(kn.ivf_gather(xd, None, slot.to(dev), None, 1, False, torch.bfloat16, (d + 31) // 32 * 32),
                     ref.ivf_gather(x, None, slot, None, 1, False, torch.bfloat16, (d + 31) // 32 * 32))


def test_gather_takes_a_strided_view_and_mixed_dtypes(kn, dev):
    ref = IvfPackKernels()
    g = torch.Generator().manual_seed(4)
    x, w = torch.randn(5, 7, 48, generator=g), torch.rand(5, 7, 2, generator=g)
    slot = torch.randint(0, 70, (90,), generator=g).to(torch.int32)
    view = x.to(dev)[:, :, 8:28]  # row stride 48, 20 columns
    assert _same(kn.ivf_gather(view, w.to(dev), slot.to(dev), None, 2, True, torch.bfloat16, 32),
                 ref.ivf_gather(x[:, :, 8:28], w, slot, None, 2, True, torch.bfloat16, 32))
    for xd, wd in ((torch.bfloat16, torch.float32), (torch.float16, torch.bfloat16), (torch.float32, torch.float16)):
        xx, ww = x.to(xd), w.to(wd)
        assert _same(kn.ivf_gather(xx.to(dev), ww.to(dev), slot.to(dev), None, 2, False, torch.float32, None),
                     ref.ivf_gather(xx, ww, slot, None, 2, False, torch.float32, None))


def test_gather_rounding_witnesses(kn, dev):
    x = torch.tensor([[[WITNESS, 1.0, 70000.0, -70000.0]]])
    one = torch.ones(1, 1, 1)
    slot = torch.zeros(1, dtype=torch.int32, device=dev)
    e = kn.ivf_gather(x.to(dev), one.to(dev), slot, None, 1, True, torch.bfloat16, 32).float().cpu()
    assert e[0, :4].tolist() == [1.0, 1.0, float("inf"), float("-inf")]  # fp32 -> fp16 -> bf16; fp16 overflow gives inf, then inf
    f = kn.ivf_gather(x.to(dev), one.to(dev), slot, None, 1, True, torch.float32, None).cpu()
    assert f[0].tolist() == [1 + 2.0 ** -8, 1.0, float("inf"), float("-inf")]
    s = kn.ivf_gather(x.to(dev), one.to(dev), slot, None, 1, False, torch.bfloat16, 32).float().cpu()
    assert s[0, :4].tolist() == [1 + 2.0 ** -7, 1.0, 70144.0, -70144.0]  # fp32 -> bf16 directly is another chain
    # a NaN weight never reaches the gather: the compaction drops it (dpr_scale_amd.ivf keeps w > 0 on both sides)
    from dpr_scale_amd import ivf

    qr = {"expert_repr": x.to(dev), "expert_ids": torch.zeros(1, 1, 1, dtype=torch.long, device=dev),
          "expert_weights": torch.full((1, 1, 1), float("nan"), device=dev), "attention_mask": torch.ones(1, 1, dtype=torch.long, device=dev)}
    assert ivf.pack_queries_device(qr, [], kernels=kn).n_entries == 0


def _golden_on_device(name, dev):
    meta, z, qr, cr = I.golden_inputs(name)
    return meta, z, I.to_device(qr, dev), I.to_device(cr, dev)


@pytest.mark.parametrize("name", F.NAMES)
def test_fixtures_end_to_end_on_the_device(kn, dev, name, tmp_path):
    from dpr_scale_amd import ivf

    meta, z, qr, cr = _golden_on_device(name, dev)
    b = ivf.IndexBuilder(meta["corpus_len"], kernels=kn)
    half = I.NDOC // 2
    for lo, hi in ((0, half), (half, I.NDOC)):
        b.add({k: v[lo:hi] for k, v in cr.items()}, list(range(lo, hi)))
    I.check_tree_against_fixture(b.write(str(tmp_path), 0), z)  # the device writer gives the golden postings
    cls_q, emb, wts = F.queries(meta, z)
    qb = ivf.pack_queries_device(qr, qr.get("cls_repr", []), kernels=kn)
    assert qb.ent_vec.device.type == "cuda" and I.same_batch(qb, ivf.pack_queries(cls_q, emb, wts))  # the host packer's bits
    index = b.finish()
    v, i = index.search_packed(qb, meta["topk"])
    assert np.array_equal(v.cpu().numpy(), z["top_scores"]) and np.array_equal(i.cpu().numpy(), z["top_ids"])
    assert I.same_index(index, ivf.load_index(str(tmp_path), meta["corpus_len"], dev, kernels=kn))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("coil", [False, True])
def test_pack_queries_device_equals_the_host_path(kn, dev, dtype, coil):
    from dpr_scale_amd import ivf

    qr = I.gaussian_repr(21, B=5, L=9, K=3, d=20, dtype=dtype, coil=coil)
    cls = torch.randn(5, 12, generator=torch.Generator().manual_seed(3))
    want = ivf.pack_queries(cls, *ivf.query_dicts(qr, 5))
    got = ivf.pack_queries_device(I.to_device(qr, dev), cls.to(dev), kernels=kn)
    assert I.same_batch(got, want) and got.n_entries > 0
    again = ivf.pack_queries_device(I.to_device(qr, dev), cls.to(dev), kernels=kn)
    assert I.same_batch(again, got)  # two runs are bit-identical


def test_eval_step_with_and_without_device_pack(kn, dev):
    from dpr_scale_amd import ivf
    from dpr_scale_amd.task.citadel_retrieval import CITADELRetrievalTask

    cr = I.gaussian_repr(31, B=200, L=12, K=3, d=32, n_experts=40)
    qr = I.gaussian_repr(32, B=5, L=9, K=3, d=32, n_experts=40)
    g = torch.Generator().manual_seed(33)
    cr["cls_repr"], qr["cls_repr"] = torch.randn(200, 16, generator=g), torch.randn(5, 16, generator=g)
    b = ivf.IndexBuilder(200, kernels=kn)
    b.add(I.to_device(cr, dev), torch.arange(200))
    index = b.finish()
    assert index.n_postings > 1000
    out = I.to_device(qr, dev)

    class Enc(torch.nn.Module):
        def forward(self, token_ids, **kw):
            return dict(out)

    results = []
    for device_pack in (True, False):
        task = CITADELRetrievalTask(ctx_embeddings_dir="unused", checkpoint_path="", topk=10, transform=None, model=None, datamodule=None,
                                    optim=None)
        task.device_pack, task.index, task.query_encoder = device_pack, index, Enc()
        batch = {"query_ids": {"input_ids": torch.zeros((5, 10), dtype=torch.long)}, "topic_ids": [f"t{j}" for j in range(5)]}
        results.append(task._eval_step(batch, 0))
        assert task.latency["encode_time"] > 0 and index.latency["search_time"] > 0
    assert results[0] == results[1]
    scores, ids = results[0][0], results[0][1]
    assert len(scores) == 5 and len(ids[0]) == 10 and len(set(ids[0])) == 10 and scores[0] == sorted(scores[0], reverse=True)


def test_the_per_query_cap_raises_at_4097_entries(kn, dev):
    from dpr_scale_amd import ivf

    big = {"expert_repr": torch.ones(2, 4097, 4, device=dev), "expert_ids": torch.zeros(2, 4097, dtype=torch.long, device=dev),
           "expert_weights": torch.ones(2, 4097, device=dev), "attention_mask": torch.ones(2, 4097, dtype=torch.long, device=dev)}
    big["attention_mask"][0, 0] = 0
    with pytest.raises(ValueError, match="query 1 has 4097 entries; at most 4096"):
        ivf.pack_queries_device(big, [], kernels=kn)
    big["attention_mask"][1, 77] = 0
    qb = ivf.pack_queries_device(big, [], kernels=kn)
    assert qb.n_entries == 2 * 4096 and qb.bexp.tolist() == [0] and qb.boff.tolist() == [0, 8192]
    assert qb.ent_q.tolist() == [0] * 4096 + [1] * 4096
