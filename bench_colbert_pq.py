"""The product-quantised ColBERT index (dpr_scale_amd/colbert.py, csrc/colbert_pq.h) against the dense index it
replaces, on the three rows of bench_colbert.py (the same synthetic corpus, the same queries) at dsub = 8 and 4:

  dense    ColBERTIndex.search: dprhot_colbert_search over bf16 rows -- the comparator, unchanged code
  pq       ColBERTPQIndex.search: dprhot_colbert_pq_search over 8-bit codes and one codebook

Before timing, the pq arm's scores and ids are held with torch.equal against decode().search (the dense kernel over the decoded rows):
the contract.  The two arms alternate in one process; median, minimum and maximum of `--steps` (at least 10) runs after warm-up.
Reported besides: index bytes of both, train and encode time, the score kernel alone by device events (dprhot_colbert_score /
dprhot_colbert_pq_score over the corpus in chunks), and for this Gaussian data the relative reconstruction error and the share of the
dense arm's top-100 that the pq arm's top-100 holds -- a floor (i.i.d. Gaussian rows have no structure for a codebook to find; DESIGN.md
section 10.2), not a quality claim.  The verdict of a row follows the project's rule: "faster" / "slower" when one arm's
median lies below the other's minimum, "inside the spread" otherwise.  One JSON line per row and dsub, appended to
profiles/colbert_pq_bench.jsonl.

    python bench_colbert_pq.py [--steps 10] [--warmup 2] [--only NAME] [--dsub 8 4] [--iters 10]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from bench_colbert import SHAPES, event_ms, make, med, score_only, timed  # noqa: E402


def pq_score_only(index, q, chunk):
    kn = index._kernels()
    S = torch.empty((q.shape[0], chunk), dtype=torch.float32, device=index.device)
    for j0 in range(0, index.corpus_len, chunk):
        kn.colbert_pq_score(index, q, 0, j0, min(chunk, index.corpus_len - j0), S)


def quantize(index, dsub, iters):
    """(ColBERTPQIndex, train ms, encode ms): ColBERTIndex.quantize in its two steps, each timed with a device synchronisation."""
    from dpr_scale_amd import colbert

    real = torch.nonzero(colbert._real_rows(index.blk_rows)).reshape(-1)
    pick = colbert._sample(int(real.shape[0]), 65536, 0)
    sample = index.tok[real[pick.to(index.device)]] if pick is not None else index.tok[real]
    del real
    train_ms, codebook = timed(lambda: colbert.train_pq(sample, dsub=dsub, iters=iters))
    encode_ms, pq = timed(lambda: index.quantize(dsub=dsub, codebook=codebook))
    return pq, train_ms, encode_ms


def verdict(a, b):
    """`a` against `b` (lists of ms): faster / slower when the median of one lies below the minimum of the other."""
    if med(a) < min(b):
        return "faster"
    if med(b) < min(a):
        return "slower"
    return "inside the spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None)
    ap.add_argument("--dsub", type=int, nargs="+", default=[8, 4])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colbert_pq_bench.jsonl"))
    a = ap.parse_args()
    from dpr_scale_amd import colbert

    dev = torch.device("cuda", 0)
    shapes = [sh for sh in SHAPES if not a.only or sh["name"] == a.only]
    for docs in sorted({sh["docs"] for sh in shapes}):
        torch.cuda.empty_cache()
        index, lens = make(next(sh for sh in shapes if sh["docs"] == docs), dev)
        T = int(lens.sum())
        for dsub in a.dsub:
            pq, train_ms, encode_ms = quantize(index, dsub, a.iters)
            dec = pq.decode()
            # relative reconstruction error over a sample of token rows
            real = torch.nonzero(colbert._real_rows(pq.blk_rows)).reshape(-1)[:: max(1, T >> 20)]
            x, y = index.tok[real].float(), dec.tok[real].float()
            rel_err = float(((x - y) ** 2).sum() / (x ** 2).sum())
            del x, y, real
            checks = {}
            for sh in shapes:
                if sh["docs"] != docs:
                    continue
                g = torch.Generator(device=dev).manual_seed(1)
                q = (torch.randn((sh["nq"], sh["LQ"], sh["d"]), generator=g, device=dev) / sh["d"] ** 0.5).to(torch.bfloat16)
                q[0, -3:] = 0  # padded query tokens
                (pv, pi), (dv, di) = pq.search(q, 100), dec.search(q, 100)
                assert torch.equal(pv, dv) and torch.equal(pi, di), f"{sh['name']} dsub={dsub}: the pq search is not decode().search"
                _, ti = index.search(q, 100)
                checks[sh["name"]] = (q, float((pi.unsqueeze(2) == ti.unsqueeze(1)).any(2).float().mean()))
            del dec
            torch.cuda.empty_cache()
            for sh in shapes:
                if sh["docs"] != docs:
                    continue
                q, recall = checks[sh["name"]]
                nq, LQ = sh["nq"], sh["LQ"]
                chunk = index.default_chunk(nq)
                reps = max(a.steps, 10)
                ds = event_ms(lambda: score_only(index, q, chunk), reps + a.warmup)[a.warmup:]
                ps = event_ms(lambda: pq_score_only(pq, q, chunk), reps + a.warmup)[a.warmup:]
                for k in (100, 1000):
                    arms = {"dense": lambda: index.search(q, k), "pq": lambda: pq.search(q, k)}
                    times = {n: [] for n in arms}
                    for fn in arms.values():
                        for _ in range(a.warmup):
                            fn()
                    for _ in range(reps):
                        for n, fn in arms.items():  # arms alternate
                            times[n].append(timed(fn)[0])
                    out = dict(bench="colbert_pq_search", shape=sh["name"], docs=docs, tokens=T, nq=nq, LQ=LQ, d=sh["d"], dsub=dsub, topk=k,
                               chunk=chunk, dense_index_bytes=index.nbytes, pq_index_bytes=pq.nbytes,
                               bytes_ratio=round(index.nbytes / pq.nbytes, 2), train_ms=round(train_ms, 1), train_iters=a.iters,
                               encode_ms=round(encode_ms, 1), rel_reconstruction_error=round(rel_err, 4), recall_of_dense_top100=round(recall, 4),
                               equal_to_decode_search=True)
                    for n, t in (("dense", times["dense"]), ("pq", times["pq"]), ("dense_score", ds), ("pq_score", ps)):
                        out[f"{n}_ms"], out[f"{n}_ms_min"], out[f"{n}_ms_max"] = med(t), round(min(t), 3), round(max(t), 3)
                    out["pq_search_is"] = verdict(times["pq"], times["dense"])
                    out["pq_score_is"] = verdict(ps, ds)
                    out["search_ratio_dense_over_pq"] = round(out["dense_ms"] / out["pq_ms"], 3)
                    line = json.dumps(out)
                    print(line, flush=True)
                    os.makedirs(os.path.dirname(a.out), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
            del pq, checks
        del index
    return 0


if __name__ == "__main__":
    t0 = time.perf_counter()
    rc = main()
    print(f"# done in {time.perf_counter() - t0:.0f} s", flush=True)
    sys.exit(rc)
