#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/colbert_{sum,max}.npz from the reference's own citadel_task.py.

Run where the reference tree is present:   python scripts/make_colbert_golden.py
The reference cannot search ColBERT (its index writer keys every posting by expert_ids); what retrieval has to agree with is its
training score.  Every expected score below comes from the reference's MultiVecRetrieverTask.expert_sim_score (:215-238), imported
unmodified through oracle.ref_shim.make_reference_citadel_task (fp32, CPU), on a padded in-batch ColBERT batch; only `query_pool` is
set on the instance.  The expected top-k is the total order (score descending, ties to the lower doc id) over those scores.

Inputs come from tests/_colbert_oracle.make_padded (grid values: every score is exact in fp32) and are stored in the fixture: 3 queries of
5 tokens (the last token of query 0 is padding), 24 passages of 12 slots with 0 .. 11 attended tokens (each length twice, shuffled), d = 24,
topk = 10.  Every passage has at least one padded slot -- the condition under which the clamped retrieval score equals the training score
(DESIGN.md section 12); it is asserted here, as scripts/make_ivf_golden.py does for the inverted index.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402
import _colbert_oracle as CO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NQ, LQ, N, LD, D, TOPK = 3, 5, 24, 12, 24, 10


def main():
    for seed, pool in ((301, "sum"), (302, "max")):
        lengths = np.random.default_rng(seed).permutation(np.repeat(np.arange(LD), 2))
        q, c, att = CO.make_padded(seed, NQ, LQ, N, LD, D, lengths=lengths, q_pad=1)
        assert bool((att.sum(1) <= LD - 1).all()) and bool((c[att == 0] == 0).all()) and bool((q[0, -1] == 0).all())
        task = ref_shim.make_reference_citadel_task(in_batch=True)
        task.query_pool = pool
        with torch.no_grad():
            S = task.expert_sim_score({"expert_repr": q.clone()}, {"expert_repr": c.clone()}, torch.zeros(N, dtype=torch.bool), pairwise=False)
        assert S.shape == (NQ, N) and S.dtype == torch.float32
        values, ids = CO.topk(S, TOPK)
        meta = dict(case=f"colbert_{pool}", pool=pool, seed=seed, nq=NQ, LQ=LQ, N=N, LD=LD, d=D, topk=TOPK, corpus_len=N)
        path = os.path.join(OUT, f"colbert_{pool}.npz")
        np.savez_compressed(path, meta=np.array(json.dumps(meta)), q=q.numpy(), c=c.numpy(), att=att.numpy(), scores=S.numpy(),
                            top_values=values.numpy(), top_ids=ids.numpy())
        print(f"colbert_{pool}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
