"""Product-quantised postings against the dense index (dpr_scale_amd/ivf.py, csrc/ivf_pq.h) on the two
shapes of bench_ivf.py.  Per shape the dense index is built, a codebook is trained on it and it is encoded (both timed); then the
dense search (dprhot_ivf_search) and the PQ search (dprhot_ivf_pq_search) alternate in one process and medians are reported.
Before timing the PQ search is held against the dense search over the decoded rows: it must be bit-equal.
Prints, and appends to --out, one JSON line per shape and top-k: index bytes and ms per query batch of each arm, train and encode
time, the PQ arm's recall of the dense arm's top-100 ids and the mean relative reconstruction error of the rows.

The synthetic rows are i.i.d. Gaussian: product quantisation lives on structure such rows do not have, so the recall and the
reconstruction error printed here are a floor, not what a trained encoder's index gives.

    python bench_ivf_pq.py [--steps 10] [--warmup 2] [--only NAME] [--sub-vec-dim 4] [--out profiles/ivf_pq_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ivf import SHAPES, make, timed  # noqa: E402


def recon_error(index, pq, step=1 << 22):
    """Mean over the rows of |x - decode(x)| / |x| (fp32, L2)."""
    from dpr_scale_amd import ivf

    total = 0.0
    for a in range(0, index.n_postings, step):
        x = index.post_vec[a:a + step].float()
        y = ivf.pq_decode(pq.post_code[a:a + step], pq.codebook).float()
        total += float(((x - y).norm(dim=1) / x.norm(dim=1).clamp_min(1e-30)).sum())
    return total / max(index.n_postings, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None)
    ap.add_argument("--sub-vec-dim", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "ivf_pq_bench.jsonl"))
    a = ap.parse_args()
    from dpr_scale_amd import ivf

    dev = torch.device("cuda", 0)
    for sh in SHAPES:
        if a.only and sh["name"] != a.only:
            continue
        index, qb = make(sh, dev)
        kn = index._kernels()
        train_ms, codebook = timed(lambda: ivf.train_pq(index.post_vec, dsub=a.sub_vec_dim, kernels=kn))
        kn.pq_encode(index.post_vec[:1024], codebook)  # (first launch)
        encode_ms, pq = timed(lambda: index.quantize(dsub=a.sub_vec_dim, codebook=codebook))
        err = recon_error(index, pq)
        decoded = pq.decode()
        bit_equal = all(torch.equal(x, y) for k in (100, 1000) for x, y in zip(pq.search_packed(qb, k), decoded.search_packed(qb, k)))
        assert bit_equal, "the PQ search differs from the dense search over the decoded rows"
        del decoded
        torch.cuda.empty_cache()
        dense_top = index.search_packed(qb, 100)[1]
        pq_top = pq.search_packed(qb, 100)[1]
        recall = float((dense_top.unsqueeze(2) == pq_top.unsqueeze(1)).any(2).float().mean())
        for k in (100, 1000):
            arms = {"dense": lambda: index.search_packed(qb, k), "pq": lambda: pq.search_packed(qb, k)}
            times = {n: [] for n in arms}
            for fn in arms.values():
                for _ in range(a.warmup):
                    fn()
            for _ in range(max(a.steps, 10)):
                for n, fn in arms.items():  # arms alternate
                    times[n].append(timed(fn)[0])
            out = dict(bench="ivf_pq_search", shape=sh["name"], docs=sh["docs"], postings=index.n_postings, nq=qb.nq, entries=qb.n_entries,
                       batch_experts=int(qb.bexp.shape[0]), d=sh["d"], sub_vec_dim=a.sub_vec_dim, topk=k, chunk=index.default_chunk(qb.nq),
                       dense_index_bytes=index.nbytes, pq_index_bytes=pq.nbytes, train_ms=round(train_ms, 1), encode_ms=round(encode_ms, 1),
                       pq_equals_decoded_dense=bit_equal, recall_of_dense_top100=round(recall, 4), mean_rel_recon_error=round(err, 4),
                       rows="iid gaussian (no structure for a product quantiser: recall and error are a floor)")
            for n in arms:
                t = torch.tensor(times[n])
                out[f"{n}_ms"] = round(float(t.median()), 3)
                out[f"{n}_ms_min_max"] = [round(float(t.min()), 3), round(float(t.max()), 3)]
            out["pq_over_dense"] = round(out["pq_ms"] / out["dense_ms"], 3)
            line = json.dumps(out)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        del index, pq, qb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
