"""The candidate stage of the pruned ColBERT search: the union of the probed inverted lists by kernels
(dprhot_colbert_union_count / _fill, csrc/colbert_union.h) against the torch union it replaces (`_CentroidPruning._union_torch`), on
the corpus, the centroids and the six rows of bench_colbert_cand.py (section 12.2), the same GPU and the same probed ids.

Arms     (a) _union_torch   (b) _union on the kernels; then the whole search_pruned (top-100) with either route -- the torch route
         through an index whose kernel set hides the colbert_union_* methods.  The arms alternate in one process; median, minimum and
         maximum of `--steps` runs after `--warmup`, host time around a synchronised call.
Claim    `gain_claimed` is true only where EVERY run of (b) is below EVERY run of (a) (the project's rule); it is stated per row.
Big row  `--big-nq` queries (1024) at nprobe = 4: both arms with torch.cuda.max_memory_allocated above what was allocated before the
         call; an arm that does not fit is recorded as such, the row is not shrunk.
Marks    the mark pass has no entry point of its own.  It is timed by difference, by device events: dprhot_colbert_union_count on the
         probed ids against the same call on ids that are all -1 -- the same four launches, every mark wave leaving at its id check.
         marks = the list entries the live, valid probes walk (one atomic OR each); marks_per_s = marks / the difference of the medians.
One JSON line per row, appended to --out (default profiles/colbert_union_bench.jsonl).

    python bench_colbert_union.py [--docs 1000000] [--n-centroids 16384] [--steps 10] [--warmup 2] [--big-nq 1024]
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import bench_colbert_cand as BC  # noqa: E402  (the corpus, the queries and the timers of section 12.2)


class WithoutUnion:
    """A kernel set without the colbert_union_* methods: `_union` then takes `_union_torch`."""

    def __init__(self, kn):
        self._kn = kn

    def __getattr__(self, name):
        if name.startswith("colbert_union"):
            raise AttributeError(name)
        return getattr(self._kn, name)


def stats(x):
    return BC.med(x), round(min(x), 3), round(max(x), 3)


def peak_bytes(fn):
    """(ms, bytes above what was allocated before the call, error text or None) of one call."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    try:
        ms, out = BC.timed(fn)
        del out
    except torch.OutOfMemoryError as e:
        return None, None, str(e).splitlines()[0]
    return round(ms, 3), torch.cuda.max_memory_allocated() - base, None


def marks_of(index, qb, cids):
    """The list entries that the mark pass walks: one per (live token, probed id in [0, C), entry of that list)."""
    C = index.cen_off.shape[0] - 1
    ok = (qb != 0).any(2).unsqueeze(2) & (cids >= 0) & (cids < C)
    c = cids.clamp(0, C - 1)
    return int(((index.cen_off[c + 1] - index.cen_off[c]) * ok).sum())


def mark_rate(index, qb, cids, steps, warmup):
    kn = index._kernels()
    nq = qb.shape[0]
    cand_off, totals = (torch.empty(n, dtype=torch.int64, device=qb.device) for n in (nq + 1, 2))
    ws = kn.colbert_union_workspace(nq, index.corpus_len, qb)
    none = torch.full_like(cids, -1)
    real, null = [], []
    for _ in range(steps + warmup):  # alternating
        real += BC.event_ms(lambda: kn.colbert_union_count(index, cids, qb, cand_off, totals, ws), 1)
        null += BC.event_ms(lambda: kn.colbert_union_count(index, none, qb, cand_off, totals, ws), 1)
    real, null = real[warmup:], null[warmup:]
    marks, diff = marks_of(index, qb, cids), BC.med(real) - BC.med(null)
    out = dict(marks=marks, count_ms=stats(real), count_no_marks_ms=stats(null), mark_ms_by_difference=round(diff, 4))
    # a difference inside the spread of either arm is no measurement
    out["marks_per_s"] = round(marks / (diff * 1e-3)) if diff > 0 and min(real) > max(null) else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--centres", type=int, default=16384)
    ap.add_argument("--n-centroids", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--train-size", type=int, default=1 << 19)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big-nq", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colbert_union_bench.jsonl"))
    a = ap.parse_args()
    dev, d, k = torch.device("cuda", 0), 128, 100
    index, lens, centres = BC.make(a.docs, a.centres, d, dev)
    index.build_centroids(a.n_centroids, iters=a.iters, train_size=a.train_size)
    old = copy.copy(index)
    old.kn = WithoutUnion(index._kernels())
    shape = dict(docs=a.docs, n_centroids=a.n_centroids, d=d, tokens=int(lens.sum()))

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    for row in BC.ROWS:
        nq, LQ = row["nq"], row["LQ"]
        q = BC.make_queries(centres, nq, LQ, dev)
        qb = index._queries(q)
        for nprobe in BC.NPROBES:
            cids = index._probe(qb, nprobe)
            got, want = index._union(qb, cids), index._union_torch(qb, cids)
            same = torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:] == want[2:]
            pv, pi = index.search_pruned(q, k, nprobe)
            ov, oi = old.search_pruned(q, k, nprobe)
            same_search = torch.equal(pv, ov) and torch.equal(pi, oi)
            arms = {"union_torch": lambda: index._union_torch(qb, cids), "union_kernels": lambda: index._union(qb, cids),
                    "pruned_torch": lambda: old.search_pruned(q, k, nprobe), "pruned_kernels": lambda: index.search_pruned(q, k, nprobe)}
            times = {n: [] for n in arms}
            for _ in range(a.warmup):
                for fn in arms.values():
                    fn()
            for _ in range(a.steps):
                for n, fn in arms.items():  # arms alternate
                    times[n].append(BC.timed(fn)[0])
            out = dict(bench="colbert_union", **shape, nq=nq, LQ=LQ, nprobe=nprobe, n_cand=got[2], max_count=got[3], lists_equal=same,
                       search_equal=same_search, topk=k, steps=a.steps)
            for n in arms:
                out[f"{n}_ms"], out[f"{n}_ms_min"], out[f"{n}_ms_max"] = stats(times[n])
            out["union_speedup_of_medians"] = round(out["union_torch_ms"] / out["union_kernels_ms"], 2)
            out["gain_claimed"] = bool(out["union_kernels_ms_max"] < out["union_torch_ms_min"])
            out["pruned_gain_claimed"] = bool(out["pruned_kernels_ms_max"] < out["pruned_torch_ms_min"])
            out.update(mark_rate(index, qb, cids, a.steps, a.warmup))
            emit(out)

    # the batch the retrieval task hands over: memory of both arms
    nq, LQ, nprobe = a.big_nq, 32, 4
    q = BC.make_queries(centres, nq, LQ, dev)
    qb = index._queries(q)
    cids = index._probe(qb, nprobe)
    out = dict(bench="colbert_union_big", **shape, nq=nq, LQ=LQ, nprobe=nprobe, steps=a.steps,
               union_ws_bytes=index._kernels()._lib.colbert_union_workspace_bytes(nq, a.docs), batches=len(index._union_batches(nq)))
    index._union(qb, cids)  # warm-up: the cached workspace is allocated here, and counted below as the kernels' own
    torch.cuda.synchronize()
    kn = index._kernels()
    held = sum(t.numel() for t in kn._ws.values())
    _, peak_b, _ = peak_bytes(lambda: index._union(qb, cids))
    out["kernels_peak_bytes"], out["kernels_workspace_held_bytes"] = peak_b, held
    ms_a, peak_a, err = peak_bytes(lambda: index._union_torch(qb, cids))
    out["torch_peak_bytes"], out["torch_fits"], out["torch_error"] = peak_a, err is None, err
    got = index._union(qb, cids)
    out["n_cand"], out["max_count"], out["result_bytes"] = got[2], got[3], got[1].numel() * 4 + got[0].numel() * 8
    times = {"union_torch": [], "union_kernels": []}
    for i in range(a.steps + a.warmup):
        if err is None:
            times["union_torch"].append(BC.timed(lambda: index._union_torch(qb, cids))[0])
        times["union_kernels"].append(BC.timed(lambda: index._union(qb, cids))[0])
    for n, t in times.items():
        if t:
            out[f"{n}_ms"], out[f"{n}_ms_min"], out[f"{n}_ms_max"] = stats(t[a.warmup:])
    if err is None:
        want = index._union_torch(qb, cids)
        out["lists_equal"] = torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:] == want[2:]
        out["gain_claimed"] = bool(out["union_kernels_ms_max"] < out["union_torch_ms_min"])
        del want
    del got
    out.update(mark_rate(index, qb, cids, a.steps, a.warmup))
    emit(out)


if __name__ == "__main__":
    main()
