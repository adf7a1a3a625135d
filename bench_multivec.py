"""Late-interaction expert scoring (ColBERT / COIL / CITADEL, citadel_task.py:155-238): one forward + backward of the fused HIP path
(hotpath.expert_sim_score) against the reference's torch formulation on the same GPU.  Both are checked against each other before
timing.  Prints one JSON line per shape: median step times, torch.cuda.max_memory_allocated above the inputs for each, and whether
the torch formulation ran out of memory.

    python bench_multivec.py [--steps 10] [--warmup 3] [--only NAME]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = [
    dict(name="colbert_pairwise", kind="colbert", B=32, M=2, LQ=32, LD=180, d=128, KQ=1, KD=1, pairwise=True),
    dict(name="colbert_at_scale", kind="colbert", B=128, Nc=1024, LQ=32, LD=256, d=128, KQ=1, KD=1, pairwise=False),
    dict(name="citadel_k1", kind="citadel", B=32, Nc=256, LQ=32, LD=180, d=32, KQ=1, KD=1, pairwise=False),
    dict(name="citadel_kd5", kind="citadel", B=32, Nc=256, LQ=32, LD=180, d=32, KQ=1, KD=5, pairwise=False),
]


def torch_expert_score(qr, cr, pairwise, pool="sum"):
    """The reference's formulation (citadel_task.py:155-238): the full token-level tensor, then max and sum."""
    q, c = qr["expert_repr"], cr["expert_repr"]
    B = q.shape[0]
    if pairwise:
        M = c.shape[0] // B
        s = torch.einsum("bid,bmjd->bimj", q, c.view(B, M, c.shape[1], c.shape[2]))
    else:
        s = torch.matmul(q.reshape(-1, q.shape[-1]), c.reshape(-1, c.shape[-1]).t()).view(q.shape[0], q.shape[1], c.shape[0], c.shape[1])
    if "expert_ids" in qr:
        qi, ci, qw, cw = qr["expert_ids"], cr["expert_ids"], qr["expert_weights"], cr["expert_weights"]
        match = qi[:, :, :, None, None, None] == ci[None, None, None]
        w = qw[:, :, :, None, None, None] * cw[None, None, None]
        v = s[:, :, None, :, :, None] * torch.where(match, w, torch.zeros((), device=w.device))
        s = v.reshape(B, v.shape[1] * v.shape[2], v.shape[3], v.shape[4] * v.shape[5])
    return s.max(-1).values.sum(1) if pool == "sum" else s.max(-1).values.max(1).values


def inputs(sh, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    B = sh["B"]
    Nc = B * sh["M"] if sh["pairwise"] else sh["Nc"]
    q = (torch.randn(B, sh["LQ"], sh["d"], generator=g) / sh["d"] ** 0.5).to(torch.bfloat16).float().to(dev)
    c = (torch.randn(Nc, sh["LD"], sh["d"], generator=g) / sh["d"] ** 0.5).to(torch.bfloat16).float().to(dev)
    qr, cr = {"expert_repr": q}, {"expert_repr": c}
    if sh["kind"] == "citadel":
        E = 64
        qr["expert_ids"] = torch.randint(0, E, (B, sh["LQ"], sh["KQ"]), generator=g).to(dev)
        cr["expert_ids"] = torch.randint(0, E, (Nc, sh["LD"], sh["KD"]), generator=g).to(dev)
        qr["expert_weights"] = torch.rand(B, sh["LQ"], sh["KQ"], generator=g).to(dev)
        cr["expert_weights"] = torch.rand(Nc, sh["LD"], sh["KD"], generator=g).to(dev)
    return qr, cr


def leafs(r):
    return {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in r.items()}


def step(fn, qr, cr, dS):
    lq, lc = leafs(qr), leafs(cr)
    S = fn(lq, lc)
    (S * dS).sum().backward()
    return S.detach(), lq["expert_repr"].grad, lc["expert_repr"].grad


def timed(fn, qr, cr, dS, steps, warmup):
    for _ in range(warmup):
        step(fn, qr, cr, dS)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(fn, qr, cr, dS)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def peak(fn, qr, cr, dS):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = step(fn, qr, cr, dS)
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    from dpr_scale_amd import hotpath

    dev = torch.device("cuda", 0)
    for sh in SHAPES:
        if a.only and sh["name"] != a.only:
            continue
        qr, cr = inputs(sh, dev)
        B = sh["B"]
        Y = sh["M"] if sh["pairwise"] else sh["Nc"]
        dS = torch.randn(B, Y, device=dev)
        fused = lambda lq, lc: hotpath.expert_sim_score(lq, lc, None, sh["pairwise"])
        ref = lambda lq, lc: torch_expert_score(lq, lc, sh["pairwise"])
        row = dict(shape=sh["name"], B=B, Y=Y, LQ=sh["LQ"], LD=sh["LD"], d=sh["d"], KQ=sh["KQ"], KD=sh["KD"],
                   token_tensor_bytes=4 * B * sh["LQ"] * sh["KQ"] * Y * sh["LD"] * sh["KD"])
        (S1, dq1, dc1), row["fused_peak_bytes"] = peak(fused, qr, cr, dS)
        row["fused_ms"] = timed(fused, qr, cr, dS, a.steps, a.warmup)
        try:
            (S0, dq0, dc0), row["torch_peak_bytes"] = peak(ref, qr, cr, dS)
            rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
            row["check"] = dict(S=rel(S1, S0), dq=rel(dq1, dq0), dc=rel(dc1, dc0))
            assert row["check"]["S"] <= 1e-2 and row["check"]["dq"] <= 2e-2 and row["check"]["dc"] <= 2e-2, row["check"]
            row["torch_ms"] = timed(ref, qr, cr, dS, a.steps, a.warmup)
            row["speedup"] = row["torch_ms"] / row["fused_ms"]
        except torch.cuda.OutOfMemoryError as e:
            row["torch_oom"] = str(e).split("\n")[0][:200]
            torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
