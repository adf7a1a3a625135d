"""The centroid-interaction stage of the pruned ColBERT search (dpr_scale_amd/colbert.py search_pruned(ndocs=), csrc/colbert_cen.h;
DESIGN.md section 12.3) against search_pruned without it, on the same index, the same GPU and the same queries.

Corpus   bench_colbert_cand.py's (section 12.2): clustered unit-norm token rows, d = 128, its centroids and its two query sets.
Arms     search_pruned(q, 100, nprobe) without ndocs against ndocs in NDOCS, at every nprobe of bench_colbert_cand.py.  The arms
         alternate in one process; median, minimum and maximum of `--steps` runs after warm-up.  The stage's parts are timed one by one
         with a device synchronisation after each: the centroid table, cen_search, the sort of the survivors, the exact stage.
Reported a gain for a row only by the project's rule -- every run of the arm with ndocs below every run of the arm without;
         recall@10 / @100 of every arm against search_pruned without ndocs (a property of this synthetic corpus); the score kernel alone
         by device events (dprhot_colbert_cen_score over every position, no top-k) with the bytes it gathers -- per (query, candidate)
         the passage's centroid ids and one table row of LT * 4 bytes per id -- and their rate.  Kernel times by name:
         `rocprofv3 --kernel-trace --stats -- python bench_colbert_cen.py --score-only`.
One JSON line per row, appended to --out (default profiles/colbert_cen_bench.jsonl).

    python bench_colbert_cen.py [--docs 1000000] [--centres 16384] [--n-centroids 16384] [--steps 10] [--warmup 2] [--score-only]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from bench_colbert_cand import NPROBES, ROWS, event_ms, make, make_queries, med, recall, timed  # noqa: E402

NDOCS = (256, 1024, 4096)
TOPK = 100


def score_only(index, T, LQ, cand_off, cand_doc, max_count, chunk):
    """dprhot_colbert_cen_score over every candidate position in chunks (no top-k): the launches the gather rate is about."""
    kn = index._kernels()
    S = torch.empty((T.shape[0], chunk), dtype=torch.float32, device=index.device)
    for j0 in range(0, max_count, chunk):
        kn.colbert_cen_score(index, T, LQ, 0, cand_off, cand_doc, j0, min(chunk, max_count - j0), S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--centres", type=int, default=16384)
    ap.add_argument("--n-centroids", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--train-size", type=int, default=1 << 19)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--score-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colbert_cen_bench.jsonl"))
    a = ap.parse_args()
    dev, d = torch.device("cuda", 0), 128
    index, lens, centres = make(a.docs, a.centres, d, dev)
    index.build_centroids(a.n_centroids, iters=a.iters, train_size=a.train_size)
    torch.cuda.synchronize()
    before = index.nbytes
    t0 = time.perf_counter()
    doc_cen_off, doc_cen = index.doc_centroids()
    torch.cuda.synchronize()
    lists_s = time.perf_counter() - t0
    list_len = doc_cen_off[1:] - doc_cen_off[:-1]

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        if not a.score_only:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    emit(dict(bench="colbert_cen_build", docs=a.docs, tokens=int(lens.sum()), n_centroids=a.n_centroids, doc_centroids_s=round(lists_s, 3),
              n_pairs=int(doc_cen.shape[0]), mean_list=round(float(list_len.float().mean()), 2), max_list=int(list_len.max()),
              list_bytes=index.nbytes - before, index_bytes=index.nbytes))
    for row in ROWS:
        nq, LQ = row["nq"], row["LQ"]
        LT = (LQ + 15) // 16 * 16
        q = make_queries(centres, nq, LQ, dev)
        qb = index._queries(q)
        for nprobe in NPROBES:
            cand_off, cand_doc, n_cand, max_count = index._candidates(qb, nprobe)
            chunk = max(8, min(index.default_chunk(nq), (max_count + 7) // 8 * 8))
            ids = int(list_len[cand_doc.long()].sum())  # centroid ids read = table rows gathered
            gather_bytes = ids * (4 + LT * 4)
            T = index._centroid_table(qb)
            kernel_ms = event_ms(lambda: score_only(index, T, LQ, cand_off, cand_doc, max_count, chunk), a.steps + a.warmup)[a.warmup:]
            table_ms = event_ms(lambda: index._centroid_table(qb), a.steps + a.warmup)[a.warmup:]
            base = dict(bench="colbert_cen_search", docs=a.docs, n_centroids=a.n_centroids, nq=nq, LQ=LQ, d=d, nprobe=nprobe, n_cand=n_cand,
                        max_count=max_count, chunk=chunk, topk=TOPK, table_bytes=int(T.numel() * 4), ids_gathered=ids, gather_bytes=gather_bytes,
                        score_kernel_ms=med(kernel_ms), score_kernel_ms_min=round(min(kernel_ms), 3), table_kernel_ms=med(table_ms))
            base["gather_gbps"] = round(gather_bytes / (base["score_kernel_ms"] * 1e-3) / 1e9, 1)
            if a.score_only:
                emit(base)
                continue
            want = {k: index.search_pruned(q, k, nprobe)[1] for k in (10, TOPK)}
            state = {}

            def parts(ndocs):
                kn = index._kernels()

                def table():
                    state["T"] = index._centroid_table(qb)

                def cen_search():
                    values = torch.empty((nq, ndocs), dtype=torch.float32, device=dev)
                    state["ids"] = torch.empty((nq, ndocs), dtype=torch.int64, device=dev)
                    ws = kn.colbert_cen_workspace(nq, chunk, ndocs, index.doc_blk)
                    kn.colbert_cen_search(index, state["T"], LQ, 0, cand_off, cand_doc, max_count, values, state["ids"], chunk, ws)

                def sort():
                    state["keep"] = torch.sort(state["ids"].to(torch.int32), dim=1).values

                def exact():
                    off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * ndocs
                    return index._search_candidates(qb, 0, TOPK, off, state["keep"].reshape(-1), ndocs)

                return dict(table=table, cen_search=cen_search, sort=sort, exact=exact)

            arms = {"pruned": lambda: index.search_pruned(q, TOPK, nprobe)}
            for ndocs in NDOCS:
                arms[f"ndocs{ndocs}"] = lambda ndocs=ndocs: index.search_pruned(q, TOPK, nprobe, ndocs=ndocs)
                for name, fn in parts(ndocs).items():
                    arms[f"ndocs{ndocs}_{name}"] = fn
            times = {n: [] for n in arms}
            for _ in range(a.warmup):
                for fn in arms.values():
                    fn()
            for _ in range(a.steps):
                for n, fn in arms.items():  # arms alternate
                    times[n].append(timed(fn)[0])
            stat = lambda n: dict(median=med(times[n]), min=round(min(times[n]), 3), max=round(max(times[n]), 3))
            for ndocs in NDOCS:
                out = dict(base, ndocs=ndocs, stage_runs=bool(ndocs < max_count))
                for k in (10, TOPK):
                    out[f"recall@{k}"] = recall(index.search_pruned(q, k, nprobe, ndocs=ndocs)[1], want[k])
                for name, key in (("pruned", "pruned_ms"), (f"ndocs{ndocs}", "ndocs_ms")):
                    s = stat(name)
                    out[key], out[key + "_min"], out[key + "_max"] = s["median"], s["min"], s["max"]
                for name in ("table", "cen_search", "sort", "exact"):
                    out[f"{name}_ms"] = stat(f"ndocs{ndocs}_{name}")["median"]
                out["ratio"] = round(out["pruned_ms"] / out["ndocs_ms"], 2)
                out["every_ndocs_run_below_every_pruned_run"] = bool(out["ndocs_ms_max"] < out["pruned_ms_min"])
                emit(out)


if __name__ == "__main__":
    main()
