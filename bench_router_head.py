#!/usr/bin/env python3
"""Forward + backward of the CITADEL encoder head (hotpath.router_head, csrc/router_head.h) against the reference's formulation in torch
ops (citadel_model.py:50-73) on the same GPU.  The two arms alternate in one process, median of 10 (as bench_multivec.py); per arm the
time and torch.cuda.max_memory_allocated above the inputs.  The fused arm is also put against the streaming floor: logits read twice
and dlogits written once at the 6.29 TB/s measured copy of DESIGN.md section 4.

    python bench_router_head.py [--out profiles/router_head_bench.jsonl] [--reps 10] [--small]
"""
import argparse
import json
import statistics
import time

import torch

COPY_TBS = 6.29
V = 30522
SHAPES = {"query": (32, 32), "passage": (256, 180)}  # sequences x tokens (CLS excluded)


def torch_head(logits, attention_mask, k):
    x = logits[:, 1:, :]
    am = attention_mask[:, 1:]
    full = torch.log(1 + torch.relu(x)) * am.unsqueeze(-1)
    w, ids = torch.topk(full, dim=2, k=k)
    rm = torch.zeros_like(full).scatter_(dim=2, index=ids, src=(w > 0.).to(w.dtype)).sum(1)
    return {"router_repr": full.max(1).values, "expert_weights": w, "router_mask": rm, "router_softmax_repr": torch.softmax(x, dim=-1).sum(1)}


def one(arm, logits, mask, k, g, soft):
    from dpr_scale_amd.hotpath import router_head

    logits.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    ret = router_head(logits, mask, topk=k, want_softmax=soft) if arm == "fused" else torch_head(logits, mask, k)
    loss = (ret["router_repr"].float() * g[0]).sum() + (ret["expert_weights"].float() * g[1]).sum()
    if soft:
        loss = loss + (ret["router_softmax_repr"].float() * g[2]).sum()
    loss.backward()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() - base
    del ret, loss
    return dt, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/router_head_bench.jsonl")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="the query shape only")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, (B, T) in SHAPES.items():
        if args.small and name != "query":
            continue
        for dtype in (torch.float32, torch.bfloat16):
            gen = torch.Generator(device=dev).manual_seed(1)
            logits = (torch.randn((B, T + 1, V), generator=gen, device=dev) * 2).to(dtype).requires_grad_(True)
            mask = torch.ones((B, T + 1), dtype=torch.long, device=dev)
            mask[:, (T + 1) * 3 // 4:] = 0
            for k in (1, 5):
                g = [torch.randn(s, generator=gen, device=dev) for s in ((B, V), (B, T, k), (B, V))]
                for soft in (False, True):
                    rec = {"shape": name, "B": B, "T": T, "V": V, "dtype": str(dtype).split(".")[-1], "k": k, "g_soft": soft, "reps": args.reps}
                    times = {"fused": [], "torch": []}
                    peaks = {}
                    for arm in ("fused", "torch"):  # warm-up; an arm that cannot run (out of memory) is reported, not hidden
                        try:
                            one(arm, logits, mask, k, g, soft)
                        except RuntimeError as e:
                            rec[f"{arm}_error"] = str(e).splitlines()[0][:200]
                            times.pop(arm)
                            torch.cuda.empty_cache()
                    for _ in range(args.reps):
                        for arm in list(times):
                            dt, peaks[arm] = one(arm, logits, mask, k, g, soft)
                            times[arm].append(dt)
                    esize = logits.element_size()
                    floor_s = 3 * B * (T + 1) * V * esize / (COPY_TBS * 1e12)
                    for arm, ts in times.items():
                        rec[f"{arm}_ms"] = round(statistics.median(ts) * 1e3, 4)
                        rec[f"{arm}_peak_mib"] = round(peaks[arm] / 2 ** 20, 1)
                    rec["floor_ms"] = round(floor_s * 1e3, 4)
                    if "fused_ms" in rec:
                        rec["fused_fraction_of_floor"] = round(floor_s * 1e3 / rec["fused_ms"], 4)
                    if "fused_ms" in rec and "torch_ms" in rec:
                        rec["speedup"] = round(rec["torch_ms"] / rec["fused_ms"], 2)
                    print(json.dumps(rec), flush=True)
                    rows.append(rec)
            del logits
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
