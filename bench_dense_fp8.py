"""The fp8 dense index (dpr_scale_amd/dense_fp8.py, csrc/dense_fp8.h) against the bf16 search it sits next to, over a synthetic corpus
of 1 M passages, d = 768, k = 100, for 1, 32 and 1024 queries, two arms on the same GPU, the same vectors and the same queries:

  bf16   hotpath.CorpusSearch over the resident bf16 corpus [n, d] (dprhot_search on the GEMM engine): 2 d bytes per passage
  fp8    DenseFP8Index.search: e4m3fn codes + one scale per row (dprhot_dense_fp8_search), d + 4 bytes per passage; the queries are
         quantised inside the timed call

Before timing, the fp8 search is held against the top-k of its own score matrix (the first 8 queries: a score depends on its two rows
only) with torch.equal.  Reported besides the times: the index bytes of both arms, the encode time of the corpus, and the share of the
bf16 top-100 that the fp8 top-100 holds, without refine and with refine=4 on the bf16 rows.  The data are i.i.d. Gaussian rows: the
shares say nothing about trained embeddings.

Arms alternate in one process; median (min - max) after warm-up; one JSON line per nq, appended to profiles/dense_fp8_bench.jsonl.  No
speed ratio is fixed in advance: `fp8_median_below_bf16_min` / `bf16_median_below_fp8_min` are the project's rule for "faster".

    python bench_dense_fp8.py [--steps 5] [--warmup 2] [--docs 1000000] [--only NQ]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

D = 768
TOPK = 100
CASES = [1, 32, 1024]  # nq


def randn_bf16(n, d, gen, dev):
    out = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    for a in range(0, n, 1 << 18):
        out[a:a + (1 << 18)] = torch.randn((min(1 << 18, n - a), d), generator=gen, device=dev) / d ** 0.5
    return out


def bf16_arm(kn, Cb, q, k):
    from dpr_scale_amd import hotpath

    s = hotpath.CorpusSearch(q, k, kernels=kn)
    s.add(Cb, 0)
    return s.result()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def med(x):
    return round(float(torch.tensor(x, dtype=torch.float64).median()), 3)


def share(found, wanted):
    """Mean over the queries of |found row & wanted row| / k."""
    hit = (found[:, :, None] == wanted[:, None, :]).any(dim=2)
    return round(float(hit.float().mean()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--only", type=int, default=None, help="nq")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_fp8_bench.jsonl"))
    a = ap.parse_args()
    from dpr_scale_amd import dense_fp8, hotpath

    dev = torch.device("cuda", 0)
    kn = hotpath.default_kernels()
    gen = torch.Generator(device=dev).manual_seed(0)
    Cb = randn_bf16(a.docs, D, gen, dev)
    encode_ms, index = timed(lambda: dense_fp8.DenseFP8Index(Cb, dev, kernels=kn, exact_rows=Cb))  # (first call: includes the code load)
    encode_ms, index = timed(lambda: dense_fp8.DenseFP8Index(Cb, dev, kernels=kn, exact_rows=Cb))
    for nq in CASES:
        if a.only and a.only != nq:
            continue
        q = randn_bf16(nq, D, gen, dev).float()
        arms = {"fp8": lambda: index.search(q, TOPK),
                "bf16": lambda: bf16_arm(kn, Cb, q, TOPK),
                "bf16_again": lambda: bf16_arm(kn, Cb, q, TOPK)}  # the bar against itself: the run-to-run spread
        (fv, fi), (bv, bi) = arms["fp8"](), arms["bf16"]()
        m = min(nq, 8)
        tv, ti = kn.topk(index.score(q[:m]).contiguous(), TOPK)
        check = dict(search_is_topk_of_own_scores=bool(torch.equal(fv[:m], tv) and torch.equal(fi[:m], ti)), queries_checked=m)
        assert check["search_is_topk_of_own_scores"], check
        _, ri = index.search(q, TOPK, refine=4)
        recall = dict(fp8_top100_of_bf16_top100=share(fi, bi), fp8_top10_of_bf16_top10=share(fi[:, :10], bi[:, :10]),
                      refine4_top100_of_bf16_top100=share(ri, bi), refine4_top10_of_bf16_top10=share(ri[:, :10], bi[:, :10]))
        refine_ms = med([timed(lambda: index.search(q, TOPK, refine=4))[0] for _ in range(3)])
        times = {n: [] for n in arms}
        for n, fn in arms.items():
            for _ in range(a.warmup):
                fn()
        for _ in range(a.steps):
            for n, fn in arms.items():  # arms alternate
                times[n].append(timed(fn)[0])
        out = dict(bench="dense_fp8_search", docs=a.docs, d=D, nq=nq, topk=TOPK, chunk=index.default_chunk(nq), steps=a.steps, warmup=a.warmup,
                   fp8_index_bytes=index.nbytes, bf16_index_bytes=Cb.numel() * 2, encode_ms=round(encode_ms, 3), check=check, recall=recall,
                   fp8_refine4_ms=refine_ms)
        for n in arms:
            out[f"{n}_ms"], out[f"{n}_ms_min"], out[f"{n}_ms_max"] = med(times[n]), round(min(times[n]), 3), round(max(times[n]), 3)
        bmin = min(out["bf16_ms_min"], out["bf16_again_ms_min"])
        out["bf16_over_fp8"] = round(out["bf16_ms"] / out["fp8_ms"], 3)
        out["fp8_median_below_bf16_min"] = bool(out["fp8_ms"] < bmin)
        out["bf16_median_below_fp8_min"] = bool(max(out["bf16_ms"], out["bf16_again_ms"]) < out["fp8_ms_min"])
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
