"""Reranking a batch of aligned (query, passage) pairs (citadel_eval_task.py:238-265): three ways to the same [B] scores on one GPU.

    a  score_only   hotpath.rerank_score: one launch, no tables (csrc/maxsim.h ms_score_kernel)
    b  training_fwd hotpath.expert_sim_score(pairwise=True) under no_grad: the training forward's two launches and its workspace of
                    value / argmax / raw tables -- the only way to these numbers before the score-only kernel
    c  torch_bmm    the reference's formulation in torch ops: the token-level score tensor, then max and pool

a and b must be torch.equal, c must agree to accumulation error, before anything is timed.  The arms alternate within one process;
each sample times `--inner` back-to-back calls between two device events and every figure is the median of `--steps` samples.
Prints one JSON line per shape: per-call times, torch.cuda.max_memory_allocated above the inputs for each arm, and the bytes of the
tables that arm b holds and arm a does not.

    python bench_rerank.py [--steps 10] [--warmup 3] [--inner 20] [--only NAME]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LQ, LD = 32, 180
SHAPES = [dict(name=f"{tag}_{B}", kind=kind, B=B, d=d, KQ=KQ, KD=KD)
          for B in (128, 1024)  # the reference's default test_batch_size, and a large batch
          for tag, kind, d, KQ, KD in (("colbert", "colbert", 128, 1, 1), ("citadel_k1", "citadel", 32, 1, 1),
                                       ("citadel_kd5", "citadel", 32, 1, 5))]
MEMORY_CAP_SHAPE = "citadel_kd5_1024"  # where arm a's peak must undercut arm b's by at least the tables


def torch_bmm_score(qr, cr, pool="sum"):
    """The reference's rerank formulation: bmm to [B, LQ, LD], match and weight per slot pair, max over passage slots, pool."""
    s = torch.bmm(qr["expert_repr"], cr["expert_repr"].permute(0, 2, 1))
    if "expert_ids" in qr:
        match = qr["expert_ids"][:, :, :, None, None] == cr["expert_ids"][:, None, None]  # B, LQ, KQ, LD, KD
        w = qr["expert_weights"][:, :, :, None, None] * cr["expert_weights"][:, None, None]
        v = s[:, :, None, :, None] * torch.where(match, w, torch.zeros((), dtype=w.dtype, device=w.device))
        s = v.view(v.shape[0], v.shape[1] * v.shape[2], v.shape[3] * v.shape[4])
    m = s.max(-1).values
    return m.sum(1) if pool == "sum" else m.max(1).values


def inputs(sh, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, d = sh["B"], sh["d"]
    q = (torch.randn(B, LQ, d, generator=g) / d ** 0.5).to(torch.bfloat16).float().to(dev)
    c = (torch.randn(B, LD, d, generator=g) / d ** 0.5).to(torch.bfloat16).float().to(dev)
    qr, cr = {"expert_repr": q}, {"expert_repr": c}
    if sh["kind"] == "citadel":
        E = 64
        qr["expert_ids"] = torch.randint(0, E, (B, LQ, sh["KQ"]), generator=g).to(dev)
        cr["expert_ids"] = torch.randint(0, E, (B, LD, sh["KD"]), generator=g).to(dev)
        qr["expert_weights"] = torch.rand(B, LQ, sh["KQ"], generator=g).to(dev)
        cr["expert_weights"] = torch.rand(B, LD, sh["KD"], generator=g).to(dev)
    return qr, cr


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    from dpr_scale_amd import hotpath

    assert torch.cuda.is_available(), "bench_rerank.py needs a HIP device"
    dev = torch.device("cuda", 0)
    for sh in SHAPES:
        if a.only and sh["name"] != a.only:
            continue
        qr, cr = inputs(sh, dev)
        B, KQ = sh["B"], sh["KQ"]
        arms = {"score_only": lambda: hotpath.rerank_score(qr, cr, "sum"),
                "training_fwd": lambda: hotpath.expert_sim_score(qr, cr, None, True, "sum")[:, 0],
                "torch_bmm": lambda: torch_bmm_score(qr, cr, "sum")}
        n_tables = 3 if "expert_weights" in qr else 2  # value, argmax (and the raw dot product when there are weights)
        row = dict(shape=sh["name"], pairs=B, LQ=LQ, LD=LD, d=sh["d"], KQ=KQ, KD=sh["KD"], steps=a.steps, inner=a.inner,
                   table_bytes=n_tables * B * LQ * KQ * 4, token_tensor_bytes=4 * B * LQ * KQ * LD * sh["KD"])
        with torch.no_grad():
            out = {}
            for name, fn in arms.items():
                out[name], row[f"{name}_peak_bytes"] = peak(fn)
            assert torch.equal(out["score_only"], out["training_fwd"]), "score-only and training forward differ"
            rel = float((out["torch_bmm"] - out["score_only"]).abs().max() / out["torch_bmm"].abs().max().clamp_min(1e-30))
            row["check"] = dict(score_only_equals_training_fwd=True, torch_bmm_rel=rel)
            assert rel <= 1e-3, row["check"]
            row["peak_saving_bytes"] = row["training_fwd_peak_bytes"] - row["score_only_peak_bytes"]
            if sh["name"] == MEMORY_CAP_SHAPE:
                assert row["peak_saving_bytes"] >= 3 * B * LQ * KQ * 4, row
            for fn in arms.values():
                for _ in range(a.warmup):
                    sample(fn, a.inner)
            ts = {name: [] for name in arms}
            for _ in range(a.steps):  # alternate: a drift of the machine lands on every arm alike
                for name, fn in arms.items():
                    ts[name].append(sample(fn, a.inner))
        for name, t in ts.items():
            t.sort()
            row[f"{name}_ms"] = t[len(t) // 2]
            row[f"{name}_ms_min_max"] = [t[0], t[-1]]
        row["speedup_vs_training_fwd"] = row["training_fwd_ms"] / row["score_only_ms"]
        row["speedup_vs_torch_bmm"] = row["torch_bmm_ms"] / row["score_only_ms"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
