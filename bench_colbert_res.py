"""The residual-compressed ColBERT index (dpr_scale_amd/colbert.py ColBERTResidualIndex, csrc/colbert_res.h)
against the dense index it was compressed from: the same pruned search on the same GPU, the same centroids and the same queries.

Corpus   bench_colbert_cand.py's: clustered unit-norm rows, lognormal lengths (median 62, at most 180), d = 128, and its query sets.
Index    ColBERTIndex.build_centroids(n_centroids) trained on the corpus' own rows, then compress(nbits) for nbits = 1, 2, 4 (buckets
         trained on the default sample).  Before anything is timed, every residual result is checked torch.equal to
         decode().search_pruned.
Arms     (a) dense search_pruned  (b) residual search_pruned, k = 100, nprobe 1 / 2 / 4, each with ndocs None and 1024.  The arms
         alternate in one process; median, minimum and maximum of `--steps` after warm-up.  The verdict follows the project's rule: an
         arm is faster when its median lies below the other arm's minimum, otherwise the two are inside the spread.
Reported index bytes of each arm; the time to train the buckets and to encode; the two exact-stage kernels alone by device events
         (dprhot_colbert_cand_score / dprhot_colbert_res_score over every position of the lists the exact stage sees, no top-k) with the
         bytes they read from HBM (dense: the candidates' token blocks; residual: their code bytes and centroid ids) and the bytes the
         residual kernel gathers from the centroid table; the relative reconstruction error |decode - tok| / |tok|; recall@10 / @100 of
         (b) against (a).  Reconstruction error and recall are properties of this synthetic corpus, not pass criteria.
One JSON line per row, appended to --out (default profiles/colbert_res_bench.jsonl).

    python bench_colbert_res.py [--docs 1000000] [--centres 16384] [--n-centroids 16384] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from bench_colbert_cand import ROWS, event_ms, make, make_queries, med, recall, timed  # noqa: E402

NBITS, NPROBES, NDOCS, K = (1, 2, 4), (1, 2, 4), (None, 1024), 100


def rel_error(dec, dense, rows=1 << 22):
    """|decoded - original| / |original| over all token rows, in pieces."""
    num = den = 0.0
    for lo in range(0, dense.tok.shape[0], rows):
        a, b = dec.tok[lo:lo + rows].float(), dense.tok[lo:lo + rows].float()
        num += float((a - b).square().sum())
        den += float(b.square().sum())
    return (num / den) ** 0.5


def exact_lists(index, qb, nprobe, ndocs):
    """(cand_off, cand_doc, max_count): the lists search_pruned hands to the exact stage."""
    cand_off, cand_doc, _, max_count = index._candidates(qb, nprobe)
    if ndocs is not None and ndocs < max_count:
        cand_doc = index._prune(qb, 0, cand_off, cand_doc, max_count, ndocs).reshape(-1)
        cand_off = torch.arange(qb.shape[0] + 1, dtype=torch.int64, device=index.device) * ndocs
        max_count = ndocs
    return cand_off, cand_doc, max_count


def score_only(index, qb, cand_off, cand_doc, max_count, chunk):
    """The exact stage's score kernel over every position of the lists in chunks (no top-k)."""
    kn = index._kernels()
    S = torch.empty((qb.shape[0], chunk), dtype=torch.float32, device=index.device)
    for j0 in range(0, max_count, chunk):
        index._score_lists(kn, qb, 0, cand_off, cand_doc, j0, min(chunk, max_count - j0), S)


def verdict(a, b):
    """By medians against minima: which of the two arms (dicts with med / min) is faster, if either."""
    if a["med"] < b["min"]:
        return "faster"
    if b["med"] < a["min"]:
        return "slower"
    return "inside the spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--centres", type=int, default=16384)
    ap.add_argument("--n-centroids", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--train-size", type=int, default=1 << 19)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colbert_res_bench.jsonl"))
    a = ap.parse_args()
    dev, d = torch.device("cuda", 0), 128
    dense, lens, centres = make(a.docs, a.centres, d, dev)
    dense.build_centroids(a.n_centroids, iters=a.iters, train_size=a.train_size)
    torch.cuda.synchronize()

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    n_blocks = dense.doc_blk[1:] - dense.doc_blk[:-1]
    queries = [(row, make_queries(centres, row["nq"], row["LQ"], dev)) for row in ROWS]
    for nbits in NBITS:
        train_ms, res = timed(lambda: dense.compress(nbits))
        kn = dense._kernels()
        encode_ms = event_ms(lambda: kn.colbert_res_encode(dense, res.cutoffs, nbits), 3)
        dec = res.decode()
        emit(dict(bench="colbert_res_build", docs=a.docs, tokens=int(lens.sum()), n_centroids=a.n_centroids, d=d, nbits=nbits,
                  dense_bytes=dense.nbytes, res_bytes=res.nbytes, bytes_ratio=round(dense.nbytes / res.nbytes, 2),
                  token_bytes_dense=dense.dp * 2, token_bytes_res=dense.dp * nbits // 8 + 4, compress_ms=round(train_ms, 1),
                  encode_kernel_ms=med(encode_ms), rel_error=round(rel_error(dec, dense), 4),
                  cutoffs=[round(float(x), 5) for x in res.cutoffs], weights=[round(float(x), 5) for x in res.weights]))
        for row, q in queries:
            nq, LQ = row["nq"], row["LQ"]
            qb = dense._queries(q)
            for nprobe in NPROBES:
                for ndocs in NDOCS:
                    got, want = res.search_pruned(q, K, nprobe, ndocs=ndocs), dec.search_pruned(q, K, nprobe, ndocs=ndocs)
                    equal = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
                    assert equal, f"nbits={nbits} nq={nq} nprobe={nprobe} ndocs={ndocs}: the residual search differs from decode()"
                    cand_off, cand_doc, max_count = exact_lists(dense, qb, nprobe, ndocs)
                    chunk = max(8, min(dense.default_chunk(nq), (max_count + 7) // 8 * 8))
                    blocks = int(n_blocks[cand_doc[cand_doc >= 0].long()].sum())
                    out = dict(bench="colbert_res_search", docs=a.docs, n_centroids=a.n_centroids, nq=nq, LQ=LQ, d=d, nbits=nbits, nprobe=nprobe,
                               ndocs=ndocs, topk=K, max_count=max_count, cand_blocks=blocks, equal_to_decode=equal,
                               dense_hbm_bytes=blocks * 16 * dense.dp * 2, res_hbm_bytes=blocks * 16 * (dense.dp * nbits // 8 + 4),
                               res_gather_bytes=blocks * 16 * dense.dp * 2)
                    for name, index in (("dense", dense), ("res", res)):
                        ms = event_ms(lambda: score_only(index, qb, cand_off, cand_doc, max_count, chunk), a.steps + a.warmup)[a.warmup:]
                        out[f"{name}_kernel_ms"], out[f"{name}_kernel_ms_min"], out[f"{name}_kernel_ms_max"] = med(ms), round(min(ms), 3), round(max(ms), 3)
                    out["kernel_verdict"] = verdict(dict(med=out["res_kernel_ms"], min=out["res_kernel_ms_min"]),
                                                    dict(med=out["dense_kernel_ms"], min=out["dense_kernel_ms_min"]))
                    for k in (10, 100):
                        out[f"recall@{k}"] = recall(res.search_pruned(q, k, nprobe, ndocs=ndocs)[1], dense.search_pruned(q, k, nprobe, ndocs=ndocs)[1])
                    arms = {"dense": lambda: dense.search_pruned(q, K, nprobe, ndocs=ndocs), "res": lambda: res.search_pruned(q, K, nprobe, ndocs=ndocs)}
                    times = {n: [] for n in arms}
                    for _ in range(a.warmup):
                        for fn in arms.values():
                            fn()
                    for _ in range(a.steps):
                        for n, fn in arms.items():  # arms alternate
                            times[n].append(timed(fn)[0])
                    for n in arms:
                        out[f"{n}_ms"], out[f"{n}_ms_min"], out[f"{n}_ms_max"] = med(times[n]), round(min(times[n]), 3), round(max(times[n]), 3)
                    out["verdict"] = verdict(dict(med=out["res_ms"], min=out["res_ms_min"]), dict(med=out["dense_ms"], min=out["dense_ms_min"]))
                    emit(out)
        del dec, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
