"""ColBERT retrieval on the CPU: the float64 restatement against the multi-vector oracle and the fixtures of the reference's training
score (scripts/make_colbert_golden.py), ColBERTIndex / TokenIndexBuilder / load_index and the two tasks driven through the test-only
stand-in (tests/_colbert_oracle.py), ColBERTEncoder, the ABI surface with the host-side validation of dprhot_colbert_*, and the
compiler's resource report of csrc/colbert.h."""
import ctypes
import inspect
import json
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _colbert_oracle as CO  # noqa: E402
import _multivec_oracle as MO  # noqa: E402
from dpr_scale_amd import colbert  # noqa: E402

REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")
_BASE = dict(transform=None, model=None, datamodule=None, optim=None)


def load(pool):
    z = np.load(os.path.join(ROOT, "tests", "golden", f"colbert_{pool}.npz"))
    return json.loads(str(z["meta"])), z


def fixture_index(z, meta, **kw):
    return colbert.ColBERTIndex.from_repr(torch.from_numpy(z["c"]), torch.from_numpy(z["att"]), list(range(meta["N"])), meta["corpus_len"],
                                          "cpu", kernels=CO.ColbertKernels(), **kw)


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_oracle_equals_the_training_score_on_grid_inputs(pool):
    q, c, att = CO.make_padded(11, nq=4, LQ=6, N=19, LD=9, d=20, q_pad=2)
    want = MO.expert_sim_score({"expert_repr": q}, {"expert_repr": c}, query_pool=pool)
    got = CO.score(q, CO.passages_of(c, att), pool)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    # an all-negative passage: the training score sees the padded slot's 0, retrieval clamps
    q1 = torch.ones(1, 2, 4)
    c1 = torch.cat([-torch.ones(1, 2, 4), torch.zeros(1, 1, 4)], 1)
    assert MO.expert_sim_score({"expert_repr": q1}, {"expert_repr": c1}, query_pool=pool).item() == 0.0
    assert CO.score(q1, [c1[0, :2]], pool).item() == 0.0


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_fixtures_reproduce_through_the_standin(pool):
    meta, z = load(pool)
    assert meta["pool"] == pool and (z["att"].sum(1) < meta["LD"]).all() and sorted(z["att"].sum(1)) == sorted(list(range(12)) * 2)
    q = torch.from_numpy(z["q"])
    assert np.array_equal(CO.score(q, CO.passages_of(torch.from_numpy(z["c"]), torch.from_numpy(z["att"])), pool).float().numpy(), z["scores"])
    index = fixture_index(z, meta)
    assert index.dp == 32 and index.d == 24 and index.n_blk == int(np.ceil(z["att"].sum(1) / 16).sum())
    S = index.score(q, 0, None, pool)
    assert S.dtype == torch.float32 and np.array_equal(S.numpy(), z["scores"])
    assert np.array_equal(index.score(q, 5, 7, pool).numpy(), z["scores"][:, 5:12])
    for kw in (dict(), dict(chunk=8), dict(chunk=16, id_ranges=[(13, 24), (0, 5), (5, 13)])):
        v, i = index.search({"expert_repr": q}, meta["topk"], query_pool=pool, **kw)
        assert v.dtype == torch.float32 and i.dtype == torch.int64
        assert np.array_equal(v.numpy(), z["top_values"]) and np.array_equal(i.numpy(), z["top_ids"])
    with pytest.raises(ValueError, match="topk"):
        index.search(q, meta["corpus_len"] + 1)
    with pytest.raises(NotImplementedError, match="pooling"):
        index.search(q, 3, query_pool="mean")
    with pytest.raises(ValueError, match="features"):
        index.search(q[:, :, :8], 3)
    assert index.latency["search_time"] > 0 and "encode_time" in index.latency


def test_layout_blocks_zero_tails_and_absent_ids():
    rows = torch.arange(1, 1 + 37 * 3, dtype=torch.float32).reshape(37, 3) / 4
    index = colbert.ColBERTIndex([5, 1, 3], [17, 0, 20], rows, 7, "cpu", kernels=CO.ColbertKernels())
    assert index.doc_blk.tolist() == [0, 0, 0, 0, 2, 2, 4, 4] and index.n_blk == 4 and index.tok.shape == (64, 32)
    want = rows.to(torch.bfloat16)
    assert torch.equal(index.tok[32:49, :3], want[:17]) and torch.equal(index.tok[0:20, :3], want[17:])
    assert not index.tok[49:64].any() and not index.tok[20:32].any() and not index.tok[:, 3:].any()
    assert index.nbytes == 64 * 32 * 2 + 8 * 8
    S = index.score(torch.ones(1, 2, 3), 0, None, "sum")
    assert S[0, [0, 1, 2, 4, 6]].eq(0).all() and S[0, 3] > 0 and S[0, 5] > 0
    with pytest.raises(ValueError, match="more than once"):
        colbert.ColBERTIndex([2, 4, 2], [1, 1, 1], rows[:3], 7, "cpu")
    with pytest.raises(ValueError, match="corpus_len"):
        colbert.ColBERTIndex([7], [1], rows[:1], 7, "cpu")
    with pytest.raises(ValueError, match="token rows"):
        colbert.ColBERTIndex([1], [2], rows[:1], 7, "cpu")
    empty = colbert.ColBERTIndex([], [], rows[:0], 3, "cpu", kernels=CO.ColbertKernels())
    assert empty.n_blk == 0 and not empty.score(torch.ones(2, 1, 3)).any()


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_builder_files_and_load_index_round_trip(pool, tmp_path):
    meta, z = load(pool)
    q, c, att = (torch.from_numpy(z[k]) for k in ("q", "c", "att"))
    kn = CO.ColbertKernels()
    whole = fixture_index(z, meta)
    # one rank; passage 7 is never added: an absent id
    b = colbert.TokenIndexBuilder(meta["corpus_len"], kernels=kn)
    keep = [i for i in range(meta["N"]) if i != 7]
    assert b.add({"expert_repr": c[keep[:10]]}, att[keep[:10]], keep[:10]) == int(att[keep[:10]].sum())
    b.add(c[keep[10:]], att[keep[10:]], keep[10:])
    path = b.write(str(tmp_path / "one"), 0)
    assert os.path.basename(path) == "tokens_0000.pkl"
    ids, lens, reprs = pickle.load(open(path, "rb"))
    assert ids.dtype == torch.int64 and lens.dtype == torch.int32 and reprs.dtype == torch.bfloat16
    assert ids.tolist() == keep and lens.tolist() == att[keep].sum(1).tolist() and reprs.shape == (int(att[keep].sum()), meta["d"])
    built, loaded = b.finish(), colbert.load_index(str(tmp_path / "one"), meta["corpus_len"], "cpu", kernels=kn)
    for index in (built, loaded):
        assert torch.equal(index.tok, built.tok) and torch.equal(index.doc_blk, built.doc_blk)
        assert index.doc_blk[8] == index.doc_blk[7]
        S = index.score(q, 0, None, pool).numpy()
        assert np.array_equal(np.delete(S, 7, 1), np.delete(z["scores"], 7, 1)) and (S[:, 7] == 0).all()
    # two ranks, interleaved passages, written in the other order: the same index as the whole corpus in one piece
    for rank, sel in ((1, list(range(0, 24, 2))), (0, list(range(23, 0, -2)))):
        b = colbert.TokenIndexBuilder()
        b.add(c[sel], att[sel], sel)
        b.write(str(tmp_path / "two"), rank)
    two = colbert.load_index(str(tmp_path / "two"), meta["corpus_len"], "cpu", chunk=8, kernels=kn)
    assert torch.equal(two.tok, whole.tok) and torch.equal(two.doc_blk, whole.doc_blk)
    v, i = two.search(q, meta["topk"], query_pool=pool)
    assert np.array_equal(v.numpy(), z["top_values"]) and np.array_equal(i.numpy(), z["top_ids"])
    with pytest.raises(FileNotFoundError):
        colbert.load_index(str(tmp_path / "none"), 3, "cpu")
    with pytest.raises(ValueError, match="corpus_len"):
        colbert.TokenIndexBuilder().finish()


class _Enc(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, token_ids, **kw):
        return dict(self.out)


@pytest.mark.parametrize("pool", ["sum", "max"])
def test_tasks_run_end_to_end_on_the_standin(pool, tmp_path):
    from dpr_scale_amd.task.citadel_eval import GenerateMultiVecEmbeddingsTask
    from dpr_scale_amd.task.citadel_retrieval import CITADELRetrievalTask
    from dpr_scale_amd.task.colbert_retrieval import ColBERTRetrievalTask, GenerateColBERTEmbeddingsTask

    meta, z = load(pool)
    q, c, att = (torch.from_numpy(z[k]) for k in ("q", "c", "att"))
    ctx = str(tmp_path / "ctx")
    writer = GenerateColBERTEmbeddingsTask(ctx_embeddings_dir=ctx, checkpoint_path="", add_context_id=False, **_BASE)
    a = inspect.signature(GenerateMultiVecEmbeddingsTask.__init__).parameters
    b = inspect.signature(GenerateColBERTEmbeddingsTask.__init__).parameters
    assert list(a) == list(b) and all(a[k].default == b[k].default for k in a)
    writer.kernels = CO.ColbertKernels()
    outs = []
    for lo, hi in ((0, 12), (12, 24)):
        writer.context_encoder = _Enc({"expert_repr": c[lo:hi]})
        full = torch.cat([torch.ones(hi - lo, 1, dtype=torch.long), att[lo:hi]], 1)  # position 0 is dropped by the task
        batch = {"contexts_ids": {"input_ids": torch.zeros_like(full), "attention_mask": full}, "corpus_ids": [str(i) for i in range(lo, hi)]}
        outs.append(writer.test_step(batch, 0))
    assert outs == [int(att[:12].sum()), int(att[12:].sum())]
    writer.test_epoch_end(outs)  # (no process group: no barrier)
    assert sorted(os.listdir(ctx)) == ["tokens_0000.pkl"]

    task = ColBERTRetrievalTask(ctx_embeddings_dir=ctx, checkpoint_path="", topk=meta["topk"], query_pool=pool,
                                output_path=str(tmp_path / "out"), **_BASE)
    assert isinstance(task, CITADELRetrievalTask) and ColBERTRetrievalTask.__init__ is CITADELRetrievalTask.__init__
    assert ColBERTRetrievalTask.merge_trec_results is CITADELRetrievalTask.merge_trec_results
    assert ColBERTRetrievalTask.merge_qa_results is CITADELRetrievalTask.merge_qa_results
    task.kernels = CO.ColbertKernels()
    task.ctxs = range(meta["corpus_len"])
    task.index = task._load_index("cpu")
    assert isinstance(task.index, colbert.ColBERTIndex) and task.index.corpus_len == meta["corpus_len"]
    task.query_encoder = _Enc({"expert_repr": q})
    topics = [f"t{n}" for n in range(meta["nq"])]
    out = task.test_step({"query_ids": {"input_ids": torch.zeros((meta["nq"], meta["LQ"] + 1), dtype=torch.long)}, "topic_ids": topics}, 0)
    assert np.array_equal(np.array(out[0], np.float32), z["top_values"]) and np.array_equal(np.array(out[1]), z["top_ids"])
    task.test_epoch_end([out])
    lines = open(os.path.join(task.output_path, "retrieval_0000.trec")).read().splitlines()
    assert len(lines) == meta["nq"] * meta["topk"]
    assert lines[0] == f"t0 Q0 {z['top_ids'][0, 0]} 1 {z['top_values'][0, 0]:.6f} dpr-scale"
    assert lines[-1] == f"t2 Q0 {z['top_ids'][2, -1]} {meta['topk']} {z['top_values'][2, -1]:.6f} dpr-scale"


def test_refusals_stay_and_point_at_each_other(tmp_path):
    from dpr_scale_amd.task.citadel_eval import GenerateMultiVecEmbeddingsTask, GenerateMultiVecQueryEmbeddingsTask
    from dpr_scale_amd.task.colbert_retrieval import ColBERTRetrievalTask, GenerateColBERTEmbeddingsTask

    base = dict(ctx_embeddings_dir=str(tmp_path), checkpoint_path="", **_BASE)
    rep = {"expert_repr": torch.zeros(2, 3, 4)}
    ids = {"input_ids": torch.zeros((2, 4), dtype=torch.long), "attention_mask": torch.ones((2, 4), dtype=torch.long)}
    t = GenerateMultiVecEmbeddingsTask(add_context_id=False, **base)
    t.context_encoder = _Enc(rep)
    with pytest.raises(NotImplementedError, match="ColBERT"):
        t.test_step({"contexts_ids": ids, "corpus_ids": ["0", "1"]}, 0)
    t = GenerateMultiVecQueryEmbeddingsTask(add_context_id=False, **base)
    t.query_encoder = _Enc(rep)
    with pytest.raises(NotImplementedError, match="ColBERT"):
        t.test_step({"query_ids": ids, "topic_ids": ["a", "b"]}, 0)
    with_ids = dict(rep, expert_ids=torch.zeros(2, 3, dtype=torch.long))
    t = GenerateColBERTEmbeddingsTask(add_context_id=False, **base)
    t.context_encoder = _Enc(with_ids)
    with pytest.raises(NotImplementedError, match="GenerateMultiVecEmbeddingsTask"):
        t.test_step({"contexts_ids": ids, "corpus_ids": ["0", "1"]}, 0)
    for kw in (dict(quantizer="pq"), dict(cuda=False), dict(portion=0.5), dict(hnsw_index=True)):
        with pytest.raises(NotImplementedError):
            ColBERTRetrievalTask(**kw, **base)
    t = ColBERTRetrievalTask(**base)
    t.query_encoder = _Enc(with_ids)
    with pytest.raises(NotImplementedError, match="CITADELRetrievalTask"):
        t.test_step({"query_ids": ids, "topic_ids": ["a", "b"]}, 0)


def test_colbert_encoder_keys_shapes_and_zeroed_pads():
    from dpr_scale_amd.models.colbert_model import ColBERTEncoder

    torch.manual_seed(0)
    cfg = dict(vocab_size=50, hidden_size=16, num_hidden_layers=1, num_attention_heads=2, intermediate_size=32, max_position_embeddings=16)
    tokens = {"input_ids": torch.randint(0, 50, (3, 7)), "attention_mask": torch.tensor([[1] * 7, [1] * 4 + [0] * 3, [1] + [0] * 6])}
    for dim, width in ((None, 16), (0, 16), (8, 8), (-1, 16)):
        enc = ColBERTEncoder(cfg, dropout=0.0, projection_dim=dim).eval()
        assert sorted(n for n, _ in enc.named_children()) == ["project", "transformer"]
        assert isinstance(enc.project, torch.nn.Identity) == (not dim)
        with torch.no_grad():
            out = enc(tokens, unused=1)
        assert list(out) == ["expert_repr"] and out["expert_repr"].shape == (3, 6, width)
        x = out["expert_repr"]
        assert not x[1, 3:].any() and not x[2].any() and x[0].abs().sum(-1).gt(0).all() and x[1, :3].abs().sum(-1).gt(0).all()
    sig = inspect.signature(ColBERTEncoder.__init__).parameters
    assert list(sig) == ["self", "model_path", "dropout", "projection_dim"]
    assert (sig["model_path"].default, sig["dropout"].default, sig["projection_dim"].default) == ("roberta-base", 0.1, None)


def test_abi_surface_and_host_validation():
    from dpr_scale_amd import _lib
    from dpr_scale_amd.hotpath import HipKernels

    assert _lib.version() == 174
    for s in ("dprhot_colbert_workspace_bytes", "dprhot_colbert_score", "dprhot_colbert_search"):
        assert hasattr(_lib.lib, s) and s in _lib.SIGNATURES
    assert callable(HipKernels.colbert_score) and callable(HipKernels.colbert_search) and callable(HipKernels.colbert_workspace)
    lib, out = _lib.lib, ctypes.c_size_t(0)
    assert lib.dprhot_colbert_workspace_bytes(32, 65536, ctypes.byref(out)) == 0 and 32 * 65536 * 4 <= out.value < 32 * 65536 * 4 + 256
    assert lib.dprhot_colbert_workspace_bytes(32, 65530, ctypes.byref(out)) == -1  # chunk % 8
    assert lib.dprhot_colbert_workspace_bytes(0, 64, ctypes.byref(out)) == -1 and lib.dprhot_colbert_workspace_bytes(1, 64, None) == -1
    assert _lib.colbert_workspace_bytes(3, 64) == 768
    one = ctypes.c_void_p(256)  # never dereferenced: validation is host code and fails before any launch
    args = lambda **kw: [kw.get(k, v) for k, v in dict(
        tok=one, blk=one, nb=10, n=100, dp=32, q=one, nq=2, LQ=5, pool=0, b=0, e=100, k=5, chunk=64, vals=one, idx=one, first=1, ws=one,
        wsb=1 << 20, st=None).items()]
    search = lib.dprhot_colbert_search
    assert search(*args(LQ=0)) == -1 and search(*args(LQ=513)) == -1 and b"LQ=513" in lib.dprhot_last_error()
    assert search(*args(dp=20)) == -1 and search(*args(dp=0)) == -1 and b"multiple of 32" in lib.dprhot_last_error()
    assert search(*args(n=2 ** 31)) == -1 and b"corpus_len" in lib.dprhot_last_error() and search(*args(n=0)) == -1
    assert search(*args(nb=2 ** 36)) == -1 and b"2^36" in lib.dprhot_last_error() and search(*args(nb=-1)) == -1
    assert search(*args(k=0)) == -1 and search(*args(k=101)) == -1 and b"topk" in lib.dprhot_last_error()
    assert search(*args(chunk=12)) == -1 and search(*args(chunk=0)) == -1 and b"chunk" in lib.dprhot_last_error()
    assert search(*args(pool=2)) == -1 and search(*args(pool=-1)) == -1 and b"pool" in lib.dprhot_last_error()
    assert search(*args(b=50, e=40)) == -1 and search(*args(e=101)) == -1 and search(*args(nq=0)) == -1
    assert search(*args(tok=ctypes.c_void_p(8))) == -1 and b"aligned" in lib.dprhot_last_error()
    for k in ("tok", "blk", "q", "vals", "idx"):
        assert search(*args(**{k: None})) == -1 and b"NULL" in lib.dprhot_last_error()
    assert search(*args(dp=2048)) == -3  # DPRHOT_E_UNSUPPORTED
    assert search(*args(wsb=16)) == -4 and search(*args(ws=None)) == -4  # workspace too small
    assert search(*args(k=5000, n=6000, e=6000, wsb=2 * 64 * 4)) == -4  # k > 4096 needs the wide selection's state too
    sargs = lambda **kw: [kw.get(k, v) for k, v in dict(tok=one, blk=one, nb=10, n=100, dp=32, q=one, nq=2, LQ=5, pool=1, b=0, cols=64, S=one,
                                                        ld=64, st=None).items()]
    score = lib.dprhot_colbert_score
    assert score(*sargs(LQ=513)) == -1 and score(*sargs(dp=48)) == -1 and score(*sargs(n=2 ** 31)) == -1 and score(*sargs(nb=2 ** 36)) == -1
    assert score(*sargs(pool=7)) == -1 and score(*sargs(S=None)) == -1 and score(*sargs(ld=63)) == -1 and score(*sargs(cols=0)) == -1
    assert score(*sargs(b=40, cols=64)) == -1 and b"outside the corpus" in lib.dprhot_last_error() and score(*sargs(b=-1)) == -1


def test_colbert_kernels_never_spill():
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
    mine = {k: v for k, v in rows.items() if re.search(r"dprhot\d+cb_\w+_kernel", k)}
    assert len(mine) == 5, sorted(rows)  # dp = 32, 64, 96, 128 and the any-width instantiation
    for name, r in mine.items():
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
