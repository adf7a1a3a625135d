"""Index postings and query batches built from the encoders' repr tensors, on the CPU: ivf.IndexBuilder, ivf.pack_queries_device and
the writer drop-ins driven through the test-only torch stand-in (tests/_ivf_pack_standin.py) against the fixtures the reference's own
writer and query step produced (tests/golden/ivf_*.npz, inputs rebuilt from the fixture's seed), the host packer, the ABI surface and
the host-side validation of dprhot_ivf_compact / dprhot_ivf_gather."""
import ast
import ctypes
import inspect
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ivf_fixture as F  # noqa: E402
import _ivf_pack_inputs as I  # noqa: E402
from _ivf_pack_standin import IvfPackKernels  # noqa: E402
from dpr_scale_amd import ivf  # noqa: E402

REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
WITNESS = 1 + 2.0 ** -8 + 2.0 ** -12  # -> 1.0 through fp16 and then bf16, -> 1 + 2^-7 straight to bf16


def _builder(meta, cr, kn=None):
    """The fixture's contexts in two `add` calls of 10 docs, as the fixture was made."""
    b = ivf.IndexBuilder(meta["corpus_len"], kernels=kn or IvfPackKernels())
    half = I.NDOC // 2
    for lo, hi in ((0, half), (half, I.NDOC)):
        assert b.add({k: v[lo:hi] for k, v in cr.items()}, list(range(lo, hi))) > 0
    return b


@pytest.mark.parametrize("name", F.NAMES)
def test_writer_reproduces_the_reference_files(name, tmp_path):
    meta, z, _, cr = I.golden_inputs(name)
    _builder(meta, cr).write(str(tmp_path), 0)
    I.check_tree_against_fixture(str(tmp_path), z)


@pytest.mark.parametrize("name", F.NAMES)
def test_pack_queries_device_equals_the_host_packer(name):
    meta, z, qr, _ = I.golden_inputs(name)
    cls_q, emb, wts = F.queries(meta, z)
    want = ivf.pack_queries(cls_q, emb, wts)
    got = ivf.pack_queries_device(qr, qr.get("cls_repr", []), kernels=IvfPackKernels())
    assert I.same_batch(got, want)
    assert I.same_batch(got, ivf.pack_queries(qr.get("cls_repr", []), *ivf.query_dicts(qr, meta["nq"])))


@pytest.mark.parametrize("name", F.NAMES)
def test_finish_searches_like_the_reference_and_equals_load_index(name, tmp_path):
    meta, z, _, cr = I.golden_inputs(name)
    kn = IvfPackKernels()
    b = _builder(meta, cr, kn)
    index = b.finish()
    cls_q, emb, wts = F.queries(meta, z)
    v, i = index.search(cls_q, emb, wts, meta["topk"])
    assert np.array_equal(v.numpy(), z["top_scores"]) and np.array_equal(i.numpy(), z["top_ids"])
    loaded = ivf.load_index(b.write(str(tmp_path), 0), meta["corpus_len"], "cpu", kernels=kn)
    assert I.same_index(index, loaded)
    assert index.dp % 32 == 0 and (index.cls is None or index.cls.shape[0] == meta["corpus_len"] + 8)


@pytest.mark.parametrize("dtype,wdtype", [(torch.float32, None), (torch.bfloat16, None), (torch.float16, None),
                                          (torch.bfloat16, torch.float32), (torch.float16, torch.bfloat16)])
@pytest.mark.parametrize("coil", [False, True])
def test_pack_queries_device_equals_host_path_on_gaussian_batches(dtype, wdtype, coil):
    qr = I.gaussian_repr(11, B=5, L=9, K=3, d=20, dtype=dtype, wdtype=wdtype, coil=coil)
    cls = torch.randn(5, 12, generator=torch.Generator().manual_seed(3))
    for n in (5, 3):
        want = ivf.pack_queries(cls[:n], *ivf.query_dicts(qr, n))
        assert I.same_batch(ivf.pack_queries_device(qr, cls[:n], n, kernels=IvfPackKernels()), want)
        assert want.n_entries > 0 and want.ent_vec.shape[1] == 32


def test_pack_queries_device_edges():
    kn = IvfPackKernels()
    qr = I.gaussian_repr(5, B=2, L=4, K=2, d=20)
    qr["attention_mask"] = torch.zeros(2, 4, dtype=torch.long)  # no entry at all: the width comes from d
    want = ivf.pack_queries([], *ivf.query_dicts(qr, 2), d=20)
    got = ivf.pack_queries_device(qr, [], kernels=kn)
    assert I.same_batch(got, want) and got.n_entries == 0 and got.ent_vec.shape == (0, 32) and got.boff.tolist() == [0]
    big = {"expert_repr": torch.ones(2, 4097, 4), "expert_ids": torch.zeros(2, 4097, dtype=torch.long),
           "expert_weights": torch.ones(2, 4097), "attention_mask": torch.ones(2, 4097, dtype=torch.long)}
    big["attention_mask"][0, 0] = 0  # query 0 has 4096 entries, query 1 has 4097
    with pytest.raises(ValueError, match="query 1 has 4097 entries; at most 4096"):
        ivf.pack_queries_device(big, [], kernels=kn)
    big["attention_mask"][1, 5] = 0
    assert ivf.pack_queries_device(big, [], kernels=kn).n_entries == 2 * 4096
    with pytest.raises(ValueError, match="differ in length"):
        ivf.pack_queries_device(qr, torch.zeros(3, 8), kernels=kn)


def test_rounding_chain_of_the_standin():
    kn = IvfPackKernels()
    x = torch.tensor([[WITNESS, 1.0, 70000.0, 3.0e-6]])
    slot = torch.zeros(1, dtype=torch.int32)
    one = torch.ones(1, 1)
    # CITADEL query entry: fp32 product -> fp16 -> bf16
    e = kn.ivf_gather(x, one, slot, None, 1, True, torch.bfloat16, 32)
    assert e.shape == (1, 32) and e[0, :4].float().tolist() == [1.0, 1.0, float("inf"), x[0, 3].half().bfloat16().float().item()]
    assert not e[0, 4:].float().any()
    # COIL query entry / in-memory index: fp32 product -> bf16
    assert kn.ivf_gather(x, one, slot, None, 1, False, torch.bfloat16, 32)[0, 0].item() == 1 + 2.0 ** -7
    assert torch.equal(x.half().bfloat16(), torch.tensor([[1.0, 1.0, float("inf"), 3.0e-6]]).half().bfloat16())
    # the product is rounded first, in the dtype torch gives `one weight * one row`
    g = torch.Generator().manual_seed(0)
    xs, ws = torch.randn(7, 5, 8, generator=g), torch.rand(7, 5, 2, generator=g)
    slots = torch.arange(70, dtype=torch.int32)
    for xd, wd in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16),
                   (torch.bfloat16, torch.float32), (torch.float16, torch.bfloat16)):
        xx, ww = xs.to(xd), ws.to(wd)
        prod = torch.stack([wk * xx.reshape(-1, 8)[j // 2] for j, wk in enumerate(ww.reshape(-1))])  # as the host loops multiply
        assert prod.dtype == xd
        assert torch.equal(kn.ivf_gather(xx, ww, slots, None, 2, False, torch.float32), prod.float())
        assert torch.equal(kn.ivf_gather(xx, ww, slots, None, 2, True, torch.bfloat16, 8), prod.half().float().bfloat16())
        perm = torch.arange(69, -1, -1)
        assert torch.equal(kn.ivf_gather(xx, ww, slots, perm, 2, False, torch.float32), prod.float().flip(0))


def test_compaction_order_and_weight_tests_of_the_standin():
    kn = IvfPackKernels()
    ids = torch.arange(2 * 3 * 2).reshape(2, 3, 2)
    w = torch.tensor([[[0.5, 0.0], [0.25, 0.25], [1.0, 1.0]], [[0.0, 0.0], [float("nan"), 0.3], [0.25, 0.26]]])
    att = torch.tensor([[1, 1, 0], [1, 1, 1]])
    rows = torch.tensor([7, 9])
    n, most, off, e, r, s, ww = kn.ivf_compact(ids, w, att, rows, True, 0.25)
    assert (n, most, off.tolist()) == (3, 2, [0, 1, 3]) and e.tolist() == [0, 9, 11] and r.tolist() == [7, 9, 9] and s.tolist() == [0, 9, 11]
    n, most, off, e, r, s, ww = kn.ivf_compact(ids, w, att, rows, False, 0.0)
    assert (n, most, off.tolist()) == (10, 6, [0, 4, 10]) and s.tolist() == [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]
    n, _, _, e, _, _, _ = kn.ivf_compact(ids, None, att, rows, True, 0.0, capacity=4)
    assert n == 10 and e.tolist() == [0, 1, 2, 3]


def _reference_init(cls_name):
    from oracle import ref_shim

    if not ref_shim.reference_available():
        pytest.skip("reference tree not present")
    src = open(os.path.join(ref_shim.REFERENCE_ROOT, "dpr_scale", "task", "citadel_eval_task.py")).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    init = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    names = [a.arg for a in init.args.args if a.arg != "self"]
    defaults = [ast.literal_eval(d) for d in init.args.defaults]
    return names, dict(zip(names[len(names) - len(defaults):], defaults))


@pytest.mark.parametrize("cls_name", ["GenerateMultiVecEmbeddingsTask", "GenerateMultiVecQueryEmbeddingsTask"])
def test_dropin_signatures_match_reference(cls_name):
    from dpr_scale_amd.task import citadel_eval

    names, want = _reference_init(cls_name)
    sig = inspect.signature(getattr(citadel_eval, cls_name).__init__).parameters
    assert [p for p in sig if p not in ("self", "kwargs")] == names
    assert {k: sig[k].default for k in want} == want
    assert all(sig[k].default is inspect.Parameter.empty for k in names if k not in want)


class _Enc(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, token_ids, **kw):
        return dict(self.out)


_BASE = dict(transform=None, model=None, datamodule=None, optim=None)


def _writer(tmp_path, cr, **kw):
    from dpr_scale_amd.task.citadel_eval import GenerateMultiVecEmbeddingsTask

    task = GenerateMultiVecEmbeddingsTask(ctx_embeddings_dir=str(tmp_path / "ctx"), checkpoint_path="", **kw, **_BASE)
    task.kernels = IvfPackKernels()
    task.context_encoder = _Enc(cr)
    return task


@pytest.mark.parametrize("name", ["ivf_coil_cls", "ivf_citadel23", "ivf_citadel23_cls"])
def test_writer_dropin_writes_the_reference_files(name, tmp_path):
    meta, z, _, cr = I.golden_inputs(name)
    task = _writer(tmp_path, cr, add_context_id=False)
    assert os.path.isdir(task.ctx_embeddings_dir) and task.weight_threshold == 0.0
    half = I.NDOC // 2
    outs = []
    for lo, hi in ((0, half), (half, I.NDOC)):
        task.context_encoder = _Enc({k: v[lo:hi] for k, v in cr.items()})
        batch = {"contexts_ids": {"input_ids": torch.zeros((hi - lo, I.LD + 1), dtype=torch.long)}, "corpus_ids": [str(i) for i in range(lo, hi)]}
        outs.append(task.test_step(batch, 0))
    task.test_epoch_end(outs)  # (no process group: no barrier)
    I.check_tree_against_fixture(task.ctx_embeddings_dir, z)


def test_writer_dropin_threshold_is_strict_and_context_ids(tmp_path):
    cr = {"expert_repr": torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4) / 8,
          "expert_ids": torch.tensor([[[1, 2], [2, 1], [1, 3]], [[3, 1], [1, 2], [2, 2]]]),
          "expert_weights": torch.tensor([[[0.5, 0.25], [0.75, 0.2], [0.9, 0.9]], [[0.25, 0.3], [0.0, 0.26], [1.0, 0.5]]]),
          "attention_mask": torch.tensor([[1, 1, 0], [1, 1, 1]])}
    batch = {"contexts_ids": {"input_ids": torch.tensor([[101, 11, 12, 13], [101, 21, 22, 23]])}, "corpus_ids": [4, 6]}
    task = _writer(tmp_path / "a", cr, add_context_id=False, weight_threshold=0.25)
    task.test_epoch_end([task.test_step(batch, 0)])
    files, cls = I.read_tree(task.ctx_embeddings_dir)
    assert cls is None and sorted(files) == [1, 2]  # expert 3 only ever has weight 0.25 (== threshold: dropped) or a padded token
    ids, w, v = files[1]
    assert ids.tolist() == [4, 6] and torch.equal(w, torch.tensor([0.5, 0.3]))
    assert torch.equal(v, torch.stack([0.5 * cr["expert_repr"][0, 0], torch.tensor(0.3) * cr["expert_repr"][1, 0]]))
    ids, w, v = files[2]
    assert ids.tolist() == [4, 6, 6, 6] and torch.equal(w, torch.tensor([0.75, 0.26, 1.0, 0.5]))
    # add_context_id: every attended slot whatever its weight, third column = the token id input_ids[b][1:][t]
    task = _writer(tmp_path / "b", cr, add_context_id=True, weight_threshold=0.25)
    task.test_epoch_end([task.test_step(batch, 0)])
    files, _ = I.read_tree(task.ctx_embeddings_dir)
    assert sorted(files) == [1, 2, 3]
    ids, w, tok = files[1]
    assert ids.tolist() == [4, 4, 6, 6] and torch.equal(w, torch.tensor([0.5, 0.2, 0.3, 0.0]))
    assert tok.dtype == torch.float32 and tok.tolist() == [11.0, 12.0, 21.0, 22.0]
    ids, w, tok = files[3]
    assert ids.tolist() == [6] and tok.tolist() == [21.0]


@pytest.mark.parametrize("name", ["ivf_coil_cls", "ivf_citadel23", "ivf_citadel23_cls"])
def test_query_writer_dropin(name, tmp_path):
    from dpr_scale_amd.task.citadel_eval import GenerateMultiVecQueryEmbeddingsTask

    meta, z, qr, _ = I.golden_inputs(name)
    out_dir = str(tmp_path / "q")
    task = GenerateMultiVecQueryEmbeddingsTask(ctx_embeddings_dir=str(tmp_path / "ctx"), checkpoint_path="", add_context_id=False,
                                               query_emb_output_dir=out_dir, **_BASE)
    assert (task.hnsw_index, task.output_path) == (False, "/tmp/results.jsonl")
    task.kernels = IvfPackKernels()
    task.query_encoder = _Enc(qr)
    batch = {"query_ids": {"input_ids": torch.zeros((I.NQ, I.LQ), dtype=torch.long)}, "topic_ids": meta["topics"]}
    task.test_epoch_end([task.test_step(batch, 0)])
    load = lambda f: pickle.load(open(os.path.join(out_dir, f), "rb"))
    assert load("query_id.pkl") == meta["topics"]
    emb, wts = load("query_repr.pkl"), load("query_weight.pkl")
    # the fixture's entries in listed order; this writer keeps fp32 (citadel_eval_task.py:162-168), the fixture's vectors are exact in fp16
    _, want_emb, want_w = F.queries(meta, z, dtype=torch.float32)
    assert len(emb) == meta["nq"] == len(wts)
    for got, want, gw, ww in zip(emb, want_emb, wts, want_w):
        assert list(got) == list(want) and list(gw) == list(want)  # same experts in the same first-seen order
        for e in want:
            assert all(a.dtype == torch.float32 and torch.equal(a, b) for a, b in zip(got[e], want[e])) and len(got[e]) == len(want[e])
            assert all(a.dtype == torch.float32 and a.dim() == 0 and a.item() == b.item() for a, b in zip(gw[e], ww[e]))
            assert got[e][0].untyped_storage().nbytes() == got[e][0].numel() * 4
    if "cls_q" in z:
        assert np.array_equal(load("query_cls.pkl").numpy(), z["cls_q"])
    else:
        assert not os.path.exists(os.path.join(out_dir, "query_cls.pkl"))


def test_retrieval_dropin_keeps_the_host_path_on_cpu():
    from dpr_scale_amd.task.citadel_retrieval import CITADELRetrievalTask

    assert CITADELRetrievalTask.device_pack is True
    qr = I.gaussian_repr(2, B=3, L=5, K=2, d=8)
    emb, wts = ivf.query_dicts(qr, 2)
    assert len(emb) == 2 and all(v.dtype == torch.float16 for d in emb for lst in d.values() for v in lst)
    first = next(iter(emb[0].items()))
    assert isinstance(first[0], int) and wts[0][first[0]][0].dtype == torch.float16


def test_abi_surface_and_host_validation():
    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import HipKernels

    assert _lib.version() == 174
    for s in ("dprhot_ivf_compact", "dprhot_ivf_gather"):
        assert hasattr(_lib.lib, s) and s in _lib.SIGNATURES
    assert callable(HipKernels.ivf_compact) and callable(HipKernels.ivf_gather)
    lib = _lib.lib
    one = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch
    cargs = lambda **kw: [kw.get(k, v) for k, v in dict(ids=one, w=one, att=one, rows=one, B=2, L=3, K=2, test=1, minw=0.0, off=one, oe=one,
                                                        orow=one, oslot=one, ow=one, cap=12, st=None).items()]
    assert lib.dprhot_ivf_compact(*cargs(K=9)) == -1 and b"K=9" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_compact(*cargs(K=0)) == -1 and lib.dprhot_ivf_compact(*cargs(L=0)) == -1
    assert lib.dprhot_ivf_compact(*cargs(B=0)) == -1 and lib.dprhot_ivf_compact(*cargs(B=65536)) == -1
    assert lib.dprhot_ivf_compact(*cargs(B=65535, L=8193, K=4)) == -1 and b"2^31" in lib.dprhot_last_error()
    for k in ("ids", "att", "rows", "off", "oe", "orow", "oslot", "ow"):
        assert lib.dprhot_ivf_compact(*cargs(**{k: None})) == -1 and b"NULL" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_compact(*cargs(cap=-1)) == -1
    gargs = lambda **kw: [kw.get(k, v) for k, v in dict(x=one, xld=32, rows=10, w=one, slot=one, perm=None, n=5, d=32, K=2, prod=0, entry=0,
                                                        kind=1, out=one, ld=32, st=None).items()]
    assert lib.dprhot_ivf_gather(*gargs(d=0)) == -1 and lib.dprhot_ivf_gather(*gargs(ld=31)) == -1 and lib.dprhot_ivf_gather(*gargs(xld=8)) == -1
    assert lib.dprhot_ivf_gather(*gargs(prod=3)) == -1 and b"prod_round" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_gather(*gargs(entry=2)) == -1 and b"entry_round" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_gather(*gargs(kind=2)) == -1 and b"out_kind" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_gather(*gargs(K=9)) == -1 and lib.dprhot_ivf_gather(*gargs(n=-1)) == -1 and lib.dprhot_ivf_gather(*gargs(rows=0)) == -1
    assert lib.dprhot_ivf_gather(*gargs(out=None)) == -1 and lib.dprhot_ivf_gather(*gargs(slot=None)) == -1
    assert lib.dprhot_ivf_gather(*gargs(x=None)) == -1 and b"NULL" in lib.dprhot_last_error()
    assert lib.dprhot_ivf_gather(*gargs(n=0, out=None, slot=None, x=None)) == 0  # nothing to do: nothing is launched


def test_new_kernels_are_in_the_resource_report_without_scratch():
    cur, rows = None, {}
    for ln in open(REPORT, errors="replace"):
        m = re.search(r" Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", ln)
        if m and cur:
            rows[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    for k in ("ivf_count_kernel", "ivf_scan_kernel", "ivf_emit_kernel", "ivf_gather_kernel"):
        mine = {n: r for n, r in rows.items() if f"dprhot{len(k)}{k}" in n}
        assert mine, k
        for n, r in mine.items():
            assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (n, r)
