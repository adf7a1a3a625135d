"""The on-disk inputs of the SPAR scripts, written from the arrays of a tests/golden/spar_*.npz fixture (and by
scripts/make_spar_golden.py from the same arrays before it runs the reference on them): a passages TSV (ids '1' .. 'n'), one JSONL of
questions and one query pickle per dataset, and the two models' reps_* shards -- model 1 in two shards, model 2 in three, so that
nothing may rely on the two directories being cut alike."""
import json
import os
import pickle

import numpy as np
import torch


def write_inputs(root, p1, p2, q1s, q2s):
    """-> dict of the keyword arguments run_spar_retrieval takes for these inputs (output_dir, weights, topk, pooling left out)."""
    root = str(root)
    n = len(p1)
    dirs = [os.path.join(root, "model_1"), os.path.join(root, "model_2")]
    for d, p, cuts in ((dirs[0], p1, [0, n // 2 + 1, n]), (dirs[1], p2, [0, n // 3, 2 * n // 3 + 2, n])):
        os.makedirs(d, exist_ok=True)
        for s, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            with open(os.path.join(d, f"reps_{s:04d}.pkl"), "wb") as f:
                pickle.dump(torch.tensor(p[a:b]), f, protocol=4)
    tsv = os.path.join(root, "passages.tsv")
    with open(tsv, "w") as f:
        f.write("id\ttext\ttitle\n")
        for i in range(n):
            f.write(f"{i + 1}\tpassage text {i}\ttitle {i}\n")
    jsonls, names = [], []
    for s, (q1, q2) in enumerate(zip(q1s, q2s)):
        name = f"query_reps_set{s}.pkl"
        for d, q in ((dirs[0], q1), (dirs[1], q2)):
            with open(os.path.join(d, name), "wb") as f:
                pickle.dump(torch.tensor(q), f, protocol=4)
        path = os.path.join(root, f"set{s}.jsonl")
        with open(path, "w") as f:
            for i in range(len(q1)):
                rec = {"question": f"question {s}-{i}", "answers": [f"answer {i}"]}
                if i % 2 == 0:
                    rec["id"] = f"s{s}q{i}"  # (every other question carries no id: the scripts fall back to its position)
                f.write(json.dumps(rec) + "\n")
        jsonls.append(path)
        names.append(name)
    return dict(jsonl_dataset_paths=jsonls, tsv_passages_path=tsv, ctx_embeddings_dir_1=dirs[0], ctx_embeddings_dir_2=dirs[1],
                output_filenames=[f"set{s}.json" for s in range(len(q1s))], query_emb_names=names)


def read_outputs(output_dir, output_filenames):
    """-> per dataset the list of records the script wrote."""
    out = []
    for name in output_filenames:
        with open(os.path.join(str(output_dir), name)) as f:
            out.append(json.load(f))
    return out


def same_ranking(scores, rows, want_scores, want_rows):
    """The rule of the fixtures: scores exactly; ids exactly wherever a score is unique within its list, tied groups as sets."""
    scores, want_scores = np.asarray(scores, dtype=np.float64), np.asarray(want_scores, dtype=np.float64)
    assert scores.shape == want_scores.shape and np.array_equal(scores, want_scores)
    for s, r, wr in zip(scores.reshape(-1, scores.shape[-1]), np.asarray(rows).reshape(-1, scores.shape[-1]),
                        np.asarray(want_rows).reshape(-1, scores.shape[-1])):
        for v in np.unique(s):
            grp = s == v
            if grp.sum() == 1:
                assert r[grp][0] == wr[grp][0]
            else:
                assert set(r[grp].tolist()) == set(wr[grp].tolist())
