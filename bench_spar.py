"""SPAR search (dpr_scale_amd/spar.py, csrc/spar.h) over a synthetic corpus of 1 M passages, d1 = d2 = 768, k = 100, for one weight and
for the reference's grid of 19 (spar_weight_tuning.py:132), three arms on the same GPU, the same vectors and the same queries:

  fused    SparIndex.search: the two resident indexes, all weights in ONE pass (dprhot_spar_search)
  concat   what the library offered before it: hotpath.CorpusSearch over a concatenated bf16 copy [n, d1 + d2] of the corpus (built
           once outside the timing; its bytes are what the fused arm does not need), ONCE PER WEIGHT, the weight folded into the query
           vector before it is rounded to bf16 (spar_retrieval.py:155)
  torch    chunked einsum of both halves in bf16 with fp32 results, s1 + w * s2 and a top-k merge per weight

Before timing, the fused arm's top-k scores are held against the concat arm's rank by rank (if two score functions differ by at most e
everywhere, so do their r-th largest values).  Each arm accumulates exact bf16 products in fp32: it is within
2^-23 * ((d1 + 1) A1 + |w| (d2 + 1) A2) of the exact score of ITS operands, A = |Q| |C|^T; the concat arm's operands differ from the fused
arm's by the rounding of w * q2 to bf16, at most 2^-9 |w| A2.  A1 and A2 are bounded by Cauchy-Schwarz: |q| * max |c|.

Arms alternate in one process; medians (and minima) after warm-up; one JSON line per (nq, W), appended to profiles/spar_bench.jsonl.
`fused_median_below_concat_min` is the project's rule for "one pass beats W searches"; for W = 1 the ratio is reported as it falls.

    python bench_spar.py [--steps 5] [--warmup 2] [--docs 1000000] [--only NQxW] [--no-torch]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

D1 = D2 = 768
TOPK = 100
GRID = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.25, 1.43, 1.67, 2, 2.5, 3.33, 5.0, 10.0]
CASES = [(1, 1), (1, 19), (1024, 1), (1024, 19)]  # (nq, W)


def randn_bf16(n, d, gen, dev):
    out = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    for a in range(0, n, 1 << 18):
        out[a:a + (1 << 18)] = torch.randn((min(1 << 18, n - a), d), generator=gen, device=dev) / d ** 0.5
    return out


def concat_arm(kn, Ccat, q1, q2, weights, k):
    from dpr_scale_amd import hotpath

    out = []
    for w in weights:
        s = hotpath.CorpusSearch(torch.cat([q1, w * q2], 1), k, kernels=kn)
        s.add(Ccat, 0)
        out.append(s.result())
    return torch.stack([v for v, _ in out]), torch.stack([i for _, i in out])


def torch_arm(c1, c2, q1, q2, weights, k, chunk):
    q1b, q2b = q1.to(torch.bfloat16), q2.to(torch.bfloat16)
    best = [None] * len(weights)
    for j0 in range(0, c1.shape[0], chunk):
        s1 = torch.einsum("nd,cd->nc", q1b, c1[j0:j0 + chunk]).float()
        s2 = torch.einsum("nd,cd->nc", q2b, c2[j0:j0 + chunk]).float()
        for j, w in enumerate(weights):
            v, i = torch.topk(torch.addcmul(s1, s2, torch.tensor(w, device=s1.device)), min(k, s1.shape[1]), dim=1)
            i = i + j0
            if best[j] is not None:
                v, sel = torch.topk(torch.cat([best[j][0], v], 1), k, dim=1)
                i = torch.gather(torch.cat([best[j][1], i], 1), 1, sel)
            best[j] = (v, i)
    return torch.stack([v for v, _ in best]), torch.stack([i for _, i in best])


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def med(x):
    return round(float(torch.tensor(x, dtype=torch.float64).median()), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--only", default=None, help="NQxW, e.g. 1024x19")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spar_bench.jsonl"))
    a = ap.parse_args()
    from dpr_scale_amd import hotpath, spar

    dev = torch.device("cuda", 0)
    kn = hotpath.default_kernels()
    gen = torch.Generator(device=dev).manual_seed(0)
    c1, c2 = randn_bf16(a.docs, D1, gen, dev), randn_bf16(a.docs, D2, gen, dev)
    index = spar.SparIndex(c1, c2, dev, kernels=kn)
    del c1, c2
    Ccat = torch.cat([index.c1, index.c2], 1).contiguous()  # the copy the concat arm needs and the fused arm does not
    cmax1, cmax2 = float(index.c1.float().norm(dim=1).max()), float(index.c2.float().norm(dim=1).max())
    for nq, W in CASES:
        if a.only and a.only != f"{nq}x{W}":
            continue
        weights = GRID[:W] if W > 1 else [1.0]
        q1, q2 = randn_bf16(nq, D1, gen, dev).float(), randn_bf16(nq, D2, gen, dev).float()
        arms = {"fused": lambda: index.search(q1, q2, weights, TOPK),
                "concat": lambda: concat_arm(kn, Ccat, q1, q2, weights, TOPK),
                "concat_again": lambda: concat_arm(kn, Ccat, q1, q2, weights, TOPK)}  # the bar against itself: the run-to-run spread
        if not a.no_torch:
            arms["torch"] = lambda: torch_arm(index.c1, index.c2, q1, q2, weights, TOPK, 65536 if nq == 1 else 8192)
        (fv, fi), (cv, ci) = arms["fused"](), arms["concat"]()
        wt = torch.tensor(weights, device=dev).abs().view(-1, 1)
        A1, A2 = q1.norm(dim=1)[None, :] * cmax1, q2.norm(dim=1)[None, :] * cmax2  # [1, nq]
        tol = 2 * 2.0 ** -23 * ((D1 + 1) * A1 + wt * (D2 + 1) * A2) + 2.0 ** -9 * wt * A2  # [W, nq]
        diff = (fv - cv).abs()
        check = dict(max_score_diff=float(diff.max()), tol_min=float(tol.min()), ids_equal=float((fi == ci).float().mean()),
                     scores_within_bound=bool((diff <= tol[:, :, None]).all()))
        assert check["scores_within_bound"], check  # (ids may differ only where two scores are closer than the bound)
        times = {n: [] for n in arms}
        for n, fn in arms.items():
            for _ in range(a.warmup):
                fn()
        for _ in range(a.steps):
            for n, fn in arms.items():  # arms alternate
                times[n].append(timed(fn)[0])
        rows = W * nq
        out = dict(bench="spar_search", docs=a.docs, d1=D1, d2=D2, nq=nq, W=W, topk=TOPK, chunk=index.default_chunk(rows), steps=a.steps,
                   index_bytes=(index.c1.numel() + index.c2.numel()) * 2, concat_copy_bytes=Ccat.numel() * 2, check=check)
        for n in arms:
            out[f"{n}_ms"], out[f"{n}_ms_min"], out[f"{n}_ms_max"] = med(times[n]), round(min(times[n]), 3), round(max(times[n]), 3)
        cmin = min(out["concat_ms_min"], out["concat_again_ms_min"])
        out["concat_over_fused"] = round(out["concat_ms"] / out["fused_ms"], 3)
        out["fused_median_below_concat_min"] = bool(out["fused_ms"] < cmin)
        out["fused_max_below_concat_min"] = bool(out["fused_ms_max"] < cmin)
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
