"""ColBERT search with centroid pruning (dpr_scale_amd/colbert.py search_pruned, csrc/colbert_cand.h) against
the exhaustive search on the same index, the same GPU and the same queries.

Corpus   token rows are unit-norm cluster centres plus noise, renormalised: `--centres` centres in all, every passage draws its tokens
         from a passage-specific subset of PER_DOC of them; the lengths follow bench_colbert.py (lognormal, median 62, at most 180),
         d = 128.  (A gaussian corpus has no cluster structure: its candidate sets would be the whole corpus.)  Queries are made the
         same way: LQ tokens from a query-specific subset of centres.
Index    ColBERTIndex.build_centroids(n_centroids) trained on the corpus' own rows; n_centroids is stated in every line.
Arms     (a) ColBERTIndex.search   (b) search_pruned, and its three parts timed one by one: probe, candidate union, cand_search.  The
         arms alternate in one process; medians and minima of `--steps` after warm-up.
Reported candidates per query as a share of the corpus; recall@10 and recall@100 of (b) against (a); the candidate kernel alone by
         device events (dprhot_colbert_cand_score over every position, no top-k) as bytes of the candidates' token blocks per second
         against the 6.29 TB/s a streaming read reaches on this chip.  Kernel times by name:
         `rocprofv3 --kernel-trace --stats -- python bench_colbert_cand.py --score-only`.
One JSON line per row, appended to --out (default profiles/colbert_cand_bench.jsonl).

    python bench_colbert_cand.py [--docs 1000000] [--centres 16384] [--n-centroids 16384] [--steps 10] [--warmup 2] [--score-only]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MAX_LEN, PER_DOC, NOISE = 180, 8, 0.35
STREAM_BPS = 6.29e12  # measured streaming read rate of the chip (MI355X_MICROARCH: HBM)
ROWS = [dict(nq=32, LQ=32), dict(nq=1, LQ=32)]
NPROBES = (1, 2, 4)


def clustered_rows(centres, picks, noise, g):
    """bf16 [n, d]: centre[picks] + gaussian noise of norm about `noise`, renormalised."""
    d = centres.shape[1]
    x = centres[picks] + torch.randn((picks.shape[0], d), generator=g, device=centres.device) * (noise / d ** 0.5)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)


def make(docs, n_centres, d, dev, seed=0):
    from dpr_scale_amd import colbert

    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.randn((n_centres, d), generator=g, device=dev)
    centres /= centres.norm(dim=1, keepdim=True)
    lens = torch.exp(torch.randn(docs, generator=g, device=dev) * 0.5 + 4.127).round().clamp_(1, MAX_LEN).long()  # bench_colbert.py's
    nblk = (lens + 15) // 16
    doc_blk = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(nblk, 0)]).contiguous()
    n_blk = int(doc_blk[-1])
    doc_centres = torch.randint(0, n_centres, (docs, PER_DOC), generator=g, device=dev)
    tok = torch.zeros((n_blk * 16, d), dtype=torch.bfloat16, device=dev)
    blk_doc = torch.repeat_interleave(torch.arange(docs, device=dev), nblk)
    for a in range(0, n_blk, 1 << 18):  # blocks of a piece: rows, their passage, which rows are real
        b = min(n_blk, a + (1 << 18))
        doc = blk_doc[a:b].repeat_interleave(16)
        row = torch.arange(a * 16, b * 16, device=dev)
        real = row - doc_blk[doc] * 16 < lens[doc]
        slot = torch.randint(0, PER_DOC, (int(real.sum()),), generator=g, device=dev)
        tok[row[real]] = clustered_rows(centres, doc_centres[doc[real], slot], NOISE, g)
    return colbert.ColBERTIndex.from_packed(tok, doc_blk, docs, d, blk_rows=colbert._blk_rows(lens, doc_blk)), lens, centres


def make_queries(centres, nq, LQ, dev, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    own = torch.randint(0, centres.shape[0], (nq, PER_DOC), generator=g, device=dev)
    slot = torch.randint(0, PER_DOC, (nq, LQ), generator=g, device=dev)
    q = clustered_rows(centres, torch.gather(own, 1, slot).reshape(-1), NOISE, g).view(nq, LQ, -1)
    q[0, -3:] = 0  # padded query tokens
    return q


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def event_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def med(x):
    return round(float(torch.tensor(x, dtype=torch.float64).median()), 3)


def score_only(index, qb, cand_off, cand_doc, max_count, chunk):
    """dprhot_colbert_cand_score over every candidate position in chunks (no top-k): the launches the bytes-per-second figure is about."""
    kn = index._kernels()
    S = torch.empty((qb.shape[0], chunk), dtype=torch.float32, device=index.device)
    for j0 in range(0, max_count, chunk):
        kn.colbert_cand_score(index, qb, 0, cand_off, cand_doc, j0, min(chunk, max_count - j0), S)


def recall(got, want):
    """Mean share of the exhaustive top-k ids that the pruned top-k holds."""
    hit = (got.unsqueeze(2) == want.unsqueeze(1)).any(1)
    return round(float(hit.float().mean()), 4)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colbert_cand_bench.jsonl"))
    a = ap.parse_args()
    dev, d = torch.device("cuda", 0), 128
    t0 = time.perf_counter()
    index, lens, centres = make(a.docs, a.centres, d, dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    index.build_centroids(a.n_centroids, iters=a.iters, train_size=a.train_size)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t1
    list_len = (index.cen_off[1:] - index.cen_off[:-1]).float()

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        if not a.score_only:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    emit(dict(bench="colbert_cand_build", docs=a.docs, tokens=int(lens.sum()), n_centroids=a.n_centroids, corpus_s=round(t1 - t0, 1),
              build_centroids_s=round(build_s, 1), kmeans_iters=a.iters, train_size=a.train_size, index_bytes=index.nbytes,
              token_bytes=index.tok.numel() * 2, mean_list=round(float(list_len.mean()), 1), max_list=int(list_len.max()),
              empty_lists=int((list_len == 0).sum())))
    blk_bytes = (index.doc_blk[1:] - index.doc_blk[:-1]) * 16 * index.dp * 2
    for row in ROWS:
        nq, LQ = row["nq"], row["LQ"]
        q = make_queries(centres, nq, LQ, dev)
        qb = index._queries(q)
        exh = {k: index.search(q, k) for k in (10, 100)}
        for nprobe in NPROBES:
            cand_off, cand_doc, n_cand, max_count = index._candidates(qb, nprobe)
            chunk = max(8, min(index.default_chunk(nq), (max_count + 7) // 8 * 8))
            cand_bytes = int(blk_bytes[cand_doc.long()].sum())
            kernel_ms = event_ms(lambda: score_only(index, qb, cand_off, cand_doc, max_count, chunk), a.steps + a.warmup)[a.warmup:]
            out = dict(bench="colbert_cand_search", docs=a.docs, n_centroids=a.n_centroids, nq=nq, LQ=LQ, d=d, nprobe=nprobe, n_cand=n_cand,
                       max_count=max_count, cand_share=round(n_cand / (nq * a.docs), 5), chunk=chunk, cand_block_bytes=cand_bytes,
                       kernel_ms=med(kernel_ms), kernel_ms_min=round(min(kernel_ms), 3))
            out["kernel_gbps"] = round(cand_bytes / (out["kernel_ms"] * 1e-3) / 1e9, 1)
            out["stream_share"] = round(cand_bytes / (out["kernel_ms"] * 1e-3) / STREAM_BPS, 4)
            out["kernel_floor_ms"] = round(cand_bytes / STREAM_BPS * 1e3, 3)
            if a.score_only:
                emit(out)
                continue
            for k in (10, 100):
                pv, pi = index.search_pruned(q, k, nprobe)
                out[f"recall@{k}"] = recall(pi, exh[k][1])
            k = 100
            state = {}

            def probe():
                state["cids"] = index._probe(qb, nprobe)

            def union():
                state["cand"] = index._union(qb, state["cids"])

            def cand_search():
                off, doc, _, mc = state["cand"]
                return index._search_candidates(qb, 0, k, off, doc, mc)

            arms = {"exhaustive": lambda: index.search(q, k), "pruned": lambda: index.search_pruned(q, k, nprobe), "probe": probe,
                    "union": union, "cand_search": cand_search}
            times = {n: [] for n in arms}
            for _ in range(a.warmup):
                for fn in arms.values():
                    fn()
            for _ in range(a.steps):
                for n, fn in arms.items():  # arms alternate
                    times[n].append(timed(fn)[0])
            for n in arms:
                out[f"{n}_ms"], out[f"{n}_ms_min"], out[f"{n}_ms_max"] = med(times[n]), round(min(times[n]), 3), round(max(times[n]), 3)
            out["topk"] = k
            out["speedup"] = round(out["exhaustive_ms"] / out["pruned_ms"], 2)
            out["pruned_median_below_exhaustive_min"] = bool(out["pruned_ms"] < out["exhaustive_ms_min"])
            emit(out)


if __name__ == "__main__":
    main()
