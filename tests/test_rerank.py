"""The rerank stage on the CPU: the golden files of the reference's two rerank tasks (scripts/make_rerank_golden.py) against the
float64 oracle, the orchestration of hotpath.expert_score_only / rerank_score and both drop-in tasks on a stand-in kernel object,
the host-side argument checks of dprhot_maxsim_score, and the compiler's resource report for ms_score_kernel."""
import ctypes
import glob
import inspect
import json
import os
import pickle
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _multivec_oracle as MO
from conftest import ROOT
from oracle import ref_shim

GOLDEN = os.path.join(ROOT, "tests", "golden")
MULTIVEC_CASES = [f"rerank_{tag}_{pool}" for tag in ("colbert", "coil", "citadel11", "citadel23") for pool in ("sum", "max")] + [
    "rerank_citadel23_sum_cls"]
SHAPES = {"colbert": dict(KQ=1, KD=1), "coil": dict(KQ=1, KD=1), "citadel": dict(KQ=2, KD=3)}
needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference tree not present")


def load_case(name):
    """(meta, query_repr, context_repr, arrays) of a golden file; the repr dicts are empty for the dense case."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    qr = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("q_")}
    cr = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("c_")}
    return meta, qr, cr, z


class ToyEncoder(torch.nn.Module):
    """Returns rows of fixed reprs (a dict, or a tensor for the dense task), as an encoder would for the current batch."""

    def __init__(self, r, dev):
        super().__init__()
        self.r = {k: v.to(dev) for k, v in r.items()} if isinstance(r, dict) else r.to(dev)
        self.rows = slice(None)
        self.scale = torch.nn.Parameter(torch.ones(()))  # (reprs come out of a module with parameters: they carry a grad_fn)

    def forward(self, ids, **kw):
        if isinstance(self.r, dict):
            out = {k: v[self.rows] for k, v in self.r.items()}
            out["expert_repr"] = out["expert_repr"] * self.scale
            return out
        return self.r[self.rows] * self.scale


def make_rerank_task(cls, out_dir, kernels, **kw):
    task = cls(checkpoint_path="", output_dir=out_dir, transform=None, model=None, datamodule=None, optim=None, **kw)
    task.kernels = kernels
    task.trainer = SimpleNamespace(strategy=object(), max_epochs=1)
    return task


def run_task(task, q, c, meta, dev=torch.device("cpu")):
    """test_step on the two batches of the golden run, then test_epoch_end; returns (step outputs, unpickled files)."""
    task.query_encoder, task.context_encoder = ToyEncoder(q, dev).to(dev), ToyEncoder(c, dev).to(dev)
    B, split = meta["B"], meta["split"]
    outs = []
    for lo, hi in ((0, split), (split, B)):
        task.query_encoder.rows = task.context_encoder.rows = slice(lo, hi)
        with torch.no_grad():  # (Lightning runs the test hooks without grad)
            outs.append(task.test_step({"query_ids": None, "contexts_ids": None, "qid": meta["qids"][lo:hi],
                                        "ctx_id": meta["ctx_ids"][lo:hi]}, 0))
    task.test_epoch_end(outs)
    files = {}
    for name in ("scores", "qids", "ctx_ids"):
        with open(os.path.join(task.output_dir, f"{name}_{task.global_rank:04}.pkl"), "rb") as f:
            files[name] = pickle.load(f)
    return outs, files


def check_files(task, outs, files, meta, z):
    """File names, pickled types and values against the golden run of the reference's task (scores bit for bit)."""
    assert sorted(os.listdir(task.output_dir)) == ["ctx_ids_0000.pkl", "qids_0000.pkl", "scores_0000.pkl"]
    for o in outs:
        assert type(o) is list and len(o) == 3 and o[2].device.type == "cpu" and o[2].dtype == torch.float32 and o[2].dim() == 1
        assert o[2].grad_fn is None
    s = files["scores"]
    assert isinstance(s, torch.Tensor) and s.dtype == torch.float32 and tuple(s.shape) == (meta["B"],)
    assert type(files["qids"]) is list and type(files["ctx_ids"]) is list
    assert files["qids"] == meta["qids"] and files["ctx_ids"] == meta["ctx_ids"]
    assert [type(x) for x in files["qids"]] == [int] * meta["B"] and [type(x) for x in files["ctx_ids"]] == [str] * meta["B"]
    MO.assert_exact("scores file", s, torch.from_numpy(z["file_scores"]).double())
    with open(os.path.join(task.output_dir, "scores_0000.pkl"), "rb") as f:
        assert f.read(2) == b"\x80\x04"  # pickle protocol 4


@pytest.fixture
def standin():
    from _rerank_standin import RerankKernels

    return RerankKernels()


def test_golden_files_are_all_here():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "rerank_*.npz")))
    assert have == sorted(MULTIVEC_CASES + ["rerank_dense"])
    for name in have:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 16 * 1024


@pytest.mark.parametrize("name", MULTIVEC_CASES)
def test_golden_scores_reproduce_through_the_oracle(name):
    meta, qr, cr, z = load_case(name)
    B = meta["B"]
    assert qr["expert_repr"].shape[0] == cr["expert_repr"].shape[0] == B and not bool(cr["expert_repr"][B - 1].any())
    q = {k: v for k, v in qr.items() if k != "cls_repr"}
    c = {k: v for k, v in cr.items() if k != "cls_repr"}
    S = MO.expert_sim_score(q, c, None, True, meta["pool"])
    assert tuple(S.shape) == (B, 1)
    assert torch.equal(S[:, 0], torch.from_numpy(z["expert_scores"]).double())
    total = S[:, 0]
    if meta["cls"]:
        total = total + (qr["cls_repr"].double() * cr["cls_repr"].double()).sum(1)
    assert torch.equal(total, torch.from_numpy(z["scores"]).double())
    assert np.array_equal(z["scores"], z["file_scores"])


def test_golden_dense_scores_reproduce():
    meta, _, _, z = load_case("rerank_dense")
    want = (torch.from_numpy(z["q"]).double() * torch.from_numpy(z["c"]).double()).sum(1)
    assert torch.equal(want, torch.from_numpy(z["scores"]).double()) and np.array_equal(z["scores"], z["file_scores"])


@pytest.mark.parametrize("kind", MO.KINDS)
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("pool", ["sum", "max"])
@pytest.mark.parametrize("masked", [False, True])
def test_score_only_orchestration_on_standin(kind, M, pool, masked, standin):
    from dpr_scale_amd import hotpath

    B = 3
    qr, cr, mask = MO.make_inputs(8 + M, kind, B=B, LQ=5, Nc=B * M, LD=7, d=20, masked=(B * M - 2,), all_pad=(B * M - 1,), **SHAPES[kind])
    f32 = lambda r: {k: (v.float().requires_grad_(True) if v.is_floating_point() else v) for k, v in r.items()}
    gq, gc = f32(qr), f32(cr)
    m = mask if masked else None
    S = hotpath.expert_score_only(gq, gc, m, pool, standin)
    assert tuple(S.shape) == (B, M) and S.dtype == torch.float32 and S.grad_fn is None and not S.requires_grad
    assert standin.score_calls == [(B, B * M, M, {"sum": 0, "max": 1}[pool])]
    S0 = MO.expert_sim_score(qr, cr, m, True, pool)
    assert torch.equal(S.double(), S0)
    if masked:
        assert bool(torch.isinf(S).reshape(-1)[B * M - 2]) and int(torch.isinf(S).sum()) == 1


@pytest.mark.parametrize("kind", MO.KINDS)
@pytest.mark.parametrize("with_cls", [False, True])
def test_rerank_score_on_standin(kind, with_cls, standin):
    from dpr_scale_amd import hotpath

    B = 4
    qr, cr, _ = MO.make_inputs(21, kind, B=B, LQ=6, Nc=B, LD=9, d=40, all_pad=(B - 1,), **SHAPES[kind])
    qr, cr = {k: (v.float() if v.is_floating_point() else v) for k, v in qr.items()}, {k: (v.float() if v.is_floating_point() else v)
                                                                                      for k, v in cr.items()}
    want = MO.expert_sim_score(qr, cr, None, True, "sum")[:, 0]
    if with_cls:
        g = np.random.default_rng(3)
        qr["cls_repr"] = torch.from_numpy(g.integers(-4, 5, size=(B, 16)).astype(np.float32) / 4.0)
        cr["cls_repr"] = torch.from_numpy(g.integers(-4, 5, size=(B, 16)).astype(np.float32) / 4.0)
        want = want + (qr["cls_repr"].double() * cr["cls_repr"].double()).sum(1)
    got = hotpath.rerank_score(qr, cr, "sum", standin)
    assert tuple(got.shape) == (B,) and got.grad_fn is None
    assert torch.equal(got.double(), want)


def test_value_errors(standin):
    from dpr_scale_amd import hotpath

    qr, cr, _ = MO.make_inputs(1, "colbert", B=2, LQ=3, Nc=5, LD=4, d=8)
    with pytest.raises(ValueError, match="not a multiple"):
        hotpath.expert_score_only(qr, cr, None, "sum", standin)
    qr, cr, _ = MO.make_inputs(1, "citadel", B=1, LQ=2, Nc=2, LD=2, d=8, KQ=1, KD=9, n_experts=12)
    with pytest.raises(ValueError, match="1..8"):
        hotpath.expert_score_only(qr, cr, None, "sum", standin)
    with pytest.raises(NotImplementedError):
        hotpath.expert_score_only(qr, cr, None, "mean", standin)
    qr, cr, _ = MO.make_inputs(1, "colbert", B=2, LQ=3, Nc=4, LD=4, d=8)
    with pytest.raises(ValueError, match="aligned pairs"):
        hotpath.rerank_score(qr, cr, "sum", standin)
    with pytest.raises(ValueError, match="mask of 3 entries"):
        hotpath.expert_score_only(qr, cr, torch.zeros(3, dtype=torch.bool), "sum", standin)
    assert standin.score_calls == []


@pytest.mark.parametrize("name", MULTIVEC_CASES)
def test_multivec_task_end_to_end_on_standin(name, standin, tmp_path):
    from dpr_scale_amd.task.rerank import RerankMultiVecRetrieverTask

    meta, qr, cr, z = load_case(name)
    out_dir = str(tmp_path / "rerank" / "out")  # (created by the constructor, parents included)
    task = make_rerank_task(RerankMultiVecRetrieverTask, out_dir, standin, query_pool=meta["pool"])
    assert os.path.isdir(out_dir)
    outs, files = run_task(task, qr, cr, meta)
    check_files(task, outs, files, meta, z)
    assert [c[:2] for c in standin.score_calls] == [(meta["split"],) * 2, (meta["B"] - meta["split"],) * 2]


def test_dense_task_end_to_end_on_standin(standin, tmp_path):
    from dpr_scale_amd.task.rerank import RerankDenseRetrieverTask

    meta, _, _, z = load_case("rerank_dense")
    task = make_rerank_task(RerankDenseRetrieverTask, str(tmp_path / "out"), standin)
    outs, files = run_task(task, torch.from_numpy(z["q"]), torch.from_numpy(z["c"]), meta)
    check_files(task, outs, files, meta, z)


def test_setup_loads_the_checkpoint(standin, tmp_path, monkeypatch):
    from dpr_scale_amd.task import rerank
    from dpr_scale_amd.task.dpr_task import DenseRetrieverTask

    seen = []
    monkeypatch.setattr(DenseRetrieverTask, "setup", lambda self, stage: seen.append(stage))
    task = make_rerank_task(rerank.RerankMultiVecRetrieverTask, str(tmp_path / "out"), standin)
    task.probe = torch.nn.Linear(2, 2)
    ckpt = str(tmp_path / "c.ckpt")
    state = {k: torch.full_like(v, 0.5) for k, v in task.state_dict().items()}
    torch.save({"state_dict": state}, ckpt)
    task.checkpoint_path = ckpt
    task.setup("test")
    assert seen == ["train"] and bool((task.probe.weight == 0.5).all())


def test_constructor_signatures():
    from dpr_scale_amd.task import rerank
    from dpr_scale_amd.task.citadel_task import MultiVecRetrieverTask
    from dpr_scale_amd.task.dpr_task import DenseRetrieverTask

    for cls, base in ((rerank.RerankMultiVecRetrieverTask, MultiVecRetrieverTask), (rerank.RerankDenseRetrieverTask, DenseRetrieverTask)):
        assert issubclass(cls, base)
        assert list(inspect.signature(cls.__init__).parameters) == ["self", "checkpoint_path", "output_dir", "kwargs"]
        assert list(inspect.signature(cls.forward).parameters) == ["self", "query_ids", "ctx_ids"]


@needs_reference
def test_constructor_signatures_equal_reference():
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_rerank_golden", os.path.join(ROOT, "scripts", "make_rerank_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.install_stubs()
    from dpr_scale.task.citadel_eval_task import RerankMultiVecRetrieverTask as RefMulti
    from dpr_scale.task.dpr_rerank_task import RerankDenseRetrieverTask as RefDense

    from dpr_scale_amd.task import rerank

    assert str(inspect.signature(rerank.RerankMultiVecRetrieverTask.__init__)) == str(inspect.signature(RefMulti.__init__))
    assert str(inspect.signature(rerank.RerankDenseRetrieverTask.__init__)) == str(inspect.signature(RefDense.__init__))


def test_maxsim_score_argument_validation_is_host_side():
    from dpr_scale_amd import _lib

    lib = _lib.lib
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: validation fails first
    args = lambda **kw: dict(dict(Nq=2, LQ=4, Nc=4, LD=8, dp=32, KQ=1, KD=1, pool=0, M=2, ids=None, w=None, q=fake, c=fake, S=fake), **kw)

    def score(a):
        return lib.dprhot_maxsim_score(a["q"], a["c"], a["Nq"], a["LQ"], a["Nc"], a["LD"], a["dp"], a["ids"], a["ids"], a["w"], a["w"],
                                       a["KQ"], a["KD"], a["pool"], a["M"], None, a["S"], None)

    err = lib.dprhot_last_error
    assert score(args(dp=40)) == -1 and b"multiple of 32" in err()
    assert score(args(LQ=513)) == -1 and b"limited to 512" in err()
    assert score(args(LD=513)) == -1 and b"limited to 512" in err()
    assert score(args(LQ=0)) == -1 and b"bad shape" in err()
    assert score(args(LD=0)) == -1 and b"bad shape" in err()
    assert score(args(ids=fake, KQ=9)) == -1 and b"1..8" in err()
    assert score(args(ids=fake, KD=9)) == -1 and b"1..8" in err()
    assert score(args(ids=fake, KQ=0)) == -1 and b"1..8" in err()
    assert score(args(KD=2)) == -1 and b"without expert ids" in err()
    assert score(args(KQ=2)) == -1 and b"without expert ids" in err()
    assert score(args(pool=2)) == -1 and b"pool" in err()
    assert score(args(pool=-1)) == -1 and b"pool" in err()
    assert score(args(M=0)) == -1 and b"pairwise" in err()
    assert score(args(M=3)) == -1 and b"pairwise" in err()
    assert score(args(Nc=5)) == -1 and b"pairwise" in err()
    for missing in ("q", "c", "S"):
        assert score(args(**{missing: None})) == -1 and b"NULL pointer" in err()
    assert score(args(Nq=0, Nc=0, q=None, c=None, S=None)) == 0  # nothing to score: no launch, nothing dereferenced


REPORT = os.path.join(ROOT, "dpr_scale_amd", "resource_usage.txt")


@pytest.mark.skipif(not os.path.isfile(REPORT), reason="no resource report next to the library (built without the Makefile)")
def test_score_kernels_use_no_scratch():
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
    ms = {k: v for k, v in rows.items() if re.search(r"dprhot\d+ms_score_kernel", k)}
    assert len(ms) == 16, sorted(ms)  # KQT in {1, 2, 4, 8} x ids x weights
    for name, r in ms.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == (4096 + 512) * 4, (name, r)  # the value table and the split planes' argmax, nothing dynamic
