"""SPAR retrieval (spar/spar_retrieval.py, spar/spar_weight_tuning.py): a dense retriever and a lexical model Lambda searched together,

    s[w](q, p) = <q1, p1> + weights[w] * <q2, p2>

on the two indexes as they are (csrc/spar.h).  The reference concatenates the two corpora into a third one and
multiplies the weight into the query half; here both indexes stay resident in bf16, the two contractions run back to back and the weight
meets the fp32 partial score in one fma -- so a whole grid of weights comes out of ONE pass over the corpus, each with its exact top-k.

    index = SparIndex.from_dirs(ctx_embeddings_dir_1, ctx_embeddings_dir_2, device)
    values, ids = index.search(q1, q2, weights, topk)        # [W, nq, topk] fp32 / int64, best first, ties to the lower passage id
    s1, s2 = index.partial_scores(q1, q2, ids)               # the two summands of every hit (score_1 / score_2 of the tuning output)

run_spar_retrieval and grid_search_weights are drop-ins for the reference's functions of the same names: same keyword arguments, same
files.  Reading questions / passages and writing JSON stay plain Python."""
import csv
import glob
import json
import os
import pickle
import tempfile

import torch

from . import hotpath
from ._chunked import ChunkedIndex, _default_kernels

_BF16 = torch.bfloat16
MAX_WEIGHTS = 32  # weights per pass (dprhot_spar_search); more are served in groups


def _load(path):
    with open(path, "rb") as f:
        return torch.as_tensor(pickle.load(f))


def shard_paths(ctx_embeddings_dir):
    paths = sorted(glob.glob(os.path.join(ctx_embeddings_dir, "reps_*")))  # spar_retrieval.py:56
    if not paths:
        raise FileNotFoundError(f"no reps_* files under {ctx_embeddings_dir}")
    return paths


def load_passage_embeddings(ctx_embeddings_dir):
    """spar_retrieval.py:54-63: every reps_* pickle in sorted order, concatenated along the rows."""
    return torch.cat([_load(p) for p in shard_paths(ctx_embeddings_dir)], dim=0)


def load_query_embeddings(ctx_embeddings_dir, query_reps_filename):
    return _load(os.path.join(ctx_embeddings_dir, query_reps_filename))


def _bf16_padded(x, dp, device):
    """[n, d] of any float type -> bf16 [n, dp] on `device`, the columns behind d zero; a tensor that already is that is returned as it is."""
    x = torch.as_tensor(x)
    if x.dtype == _BF16 and x.device == device and x.shape[1] == dp and x.is_contiguous():
        return x
    out = torch.zeros((x.shape[0], dp), dtype=_BF16, device=device)
    out[:, : x.shape[1]] = x.to(device).to(_BF16)
    return out


def _weights(weights):
    ws = [float(weights)] if isinstance(weights, (int, float)) else [float(w) for w in weights]
    if not ws:
        raise ValueError("no weights")
    return ws


class SparIndex(ChunkedIndex):
    """The two corpora of a SPAR pair, bf16 on the device, hidden sizes zero-padded to multiples of 32; passage id = row."""

    def __init__(self, p_vectors_1, p_vectors_2, device=None, chunk=None, kernels=None, widths=None):
        """widths: the models' hidden sizes (d1, d2) where the vectors passed in are already zero-padded beyond them."""
        p1, p2 = torch.as_tensor(p_vectors_1), torch.as_tensor(p_vectors_2)
        if p1.dim() != 2 or p2.dim() != 2 or p1.shape[0] != p2.shape[0]:
            raise ValueError(f"the two models must embed the same passages: {tuple(p1.shape)} and {tuple(p2.shape)}")
        if p1.shape[0] == 0:
            raise ValueError("empty corpus")
        self.device = torch.device(device) if device is not None else p1.device
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.corpus_len = int(p1.shape[0])
        self.d1, self.d2 = (int(p1.shape[1]), int(p2.shape[1])) if widths is None else (int(widths[0]), int(widths[1]))
        self.dp1, self.dp2 = (self.d1 + 31) // 32 * 32, (self.d2 + 31) // 32 * 32
        if widths is not None and (p1.shape[1], p2.shape[1]) != (self.dp1, self.dp2):
            raise ValueError(f"widths {tuple(widths)} do not pad to the vectors' {p1.shape[1]} / {p2.shape[1]} columns")
        self.c1 = _bf16_padded(p1, self.dp1, self.device)
        self.c2 = _bf16_padded(p2, self.dp2, self.device)
        self._init_search(chunk, kernels)

    @classmethod
    def from_dirs(cls, ctx_embeddings_dir_1, ctx_embeddings_dir_2, device=None, chunk=None, kernels=None):
        """Both sets of reps_* pickles, each in sorted order and concatenated along the rows only (spar_retrieval.py:54-63, :131, :138).
        The host holds one shard at a time: a shard is read, rounded to bf16 and padded on the device, and released.  The row count is
        only known once a model's last shard has been read, so the device holds that model's vectors twice while its pieces are joined
        (the pieces are freed before the second model is read); the index takes the joined tensors without another copy."""
        device = torch.device(device) if device is not None else torch.device("cuda", 0)
        sides, widths = [], []
        for d in (ctx_embeddings_dir_1, ctx_embeddings_dir_2):
            pieces, width = [], None
            for path in shard_paths(d):
                shard = _load(path)
                if width is None:
                    width = int(shard.shape[1])
                elif int(shard.shape[1]) != width:
                    raise ValueError(f"{path}: {shard.shape[1]} columns where the shards before it have {width}")
                pieces.append(_bf16_padded(shard, (width + 31) // 32 * 32, device))
                del shard
            sides.append(pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=0))
            widths.append(width)
            del pieces
        return cls(sides[0], sides[1], sides[0].device, chunk=chunk, kernels=kernels, widths=widths)

    def default_chunk(self, rows):
        """Passage ids per pass for `rows` = W * nq state rows: the workspace holds a candidate value and a column per row and id
        (8 bytes; at most 1 GiB by default, at least 1024 ids) -- a 128-wide column tile per compute unit wants thousands of ids."""
        c = self.chunk if self.chunk is not None else max(1024, min(262144, (1 << 27) // max(rows, 1)))
        c = min(c, (self.corpus_len + 7) // 8 * 8)
        return max(8, c // 8 * 8)

    def _queries(self, q1, q2):
        q1, q2 = torch.as_tensor(q1), torch.as_tensor(q2)
        if q1.dim() != 2 or q2.dim() != 2 or q1.shape[0] != q2.shape[0] or q1.shape[1] != self.d1 or q2.shape[1] != self.d2:
            raise ValueError(f"queries {tuple(q1.shape)} / {tuple(q2.shape)} do not fit an index of widths {self.d1} / {self.d2}")
        return _bf16_padded(q1, self.dp1, self.device), _bf16_padded(q2, self.dp2, self.device)

    def search(self, q1, q2, weights, topk, id_ranges=None, chunk=None):
        """(values [W, nq, topk] fp32, ids [W, nq, topk] int64): for every weight the exact top-k of <q1, p1> + w * <q2, p2> over the
        disjoint (begin, end) passage-id ranges (default: the whole corpus), best first, ties to the lower id, a NaN score never
        selected, -inf / -1 where fewer than topk candidates exist.  `weights`: a float or a sequence; more than 32 run in groups."""
        ws = _weights(weights)
        kn = self._kernels()
        q1b, q2b = self._queries(q1, q2)
        nq = q1b.shape[0]
        topk = int(topk)
        out_v, out_i = [], []
        for g0 in range(0, len(ws), MAX_WEIGHTS):
            lam = ws[g0:g0 + MAX_WEIGHTS]
            v, i = self._fold(
                len(lam) * nq, topk, id_ranges, chunk,
                lambda c: kn.spar_workspace(nq, len(lam), c, topk, q1b),
                lambda b, e, values, indices, first, c, wsp: kn.spar_search(self, q1b, q2b, lam, b, e, values, indices, first, c, wsp))
            out_v.append(v.view(len(lam), nq, topk))
            out_i.append(i.view(len(lam), nq, topk))
        return torch.cat(out_v, 0), torch.cat(out_i, 0)

    def score(self, q1, q2, weights, doc_begin=0, cols=None):
        """S [W, nq, cols] fp32 of passages doc_begin .. doc_begin + cols (default: to the end), the scores `search` ranks."""
        ws = _weights(weights)
        kn = self._kernels()
        q1b, q2b = self._queries(q1, q2)
        nq = q1b.shape[0]
        cols = self.corpus_len - doc_begin if cols is None else int(cols)
        ld = (cols + 7) // 8 * 8
        out = []
        for g0 in range(0, len(ws), MAX_WEIGHTS):
            lam = ws[g0:g0 + MAX_WEIGHTS]
            S = torch.empty((len(lam) * nq, ld), dtype=torch.float32, device=self.device)
            kn.spar_score(self, q1b, q2b, lam, doc_begin, cols, S)
            out.append(S[:, :cols].view(len(lam), nq, cols))
        return torch.cat(out, 0)

    def partial_scores(self, q1, q2, ids, block_elems=1 << 24):
        """(s1, s2) fp32, shaped like ids [..., nq, k]: <q1, p1> and <q2, p2> of the given passages, on the bf16 vectors the index
        holds, as a torch gather + row-wise dot on the device (nq * k rows per weight: off the hot path).  An id of -1 gives -inf.
        Queries are taken in blocks so that a gathered fp32 block stays near block_elems elements (64 MiB) whatever nq, k and the
        number of weights are."""
        q1b, q2b = self._queries(q1, q2)
        ids = torch.as_tensor(ids).to(self.device)
        flat = ids.reshape(-1, ids.shape[-2], ids.shape[-1])  # [L, nq, k]
        L, nq, k = flat.shape
        if nq != q1b.shape[0]:
            raise ValueError(f"ids {tuple(ids.shape)} for {q1b.shape[0]} queries")
        s1 = torch.empty(flat.shape, dtype=torch.float32, device=self.device)
        s2 = torch.empty(flat.shape, dtype=torch.float32, device=self.device)
        for out, qb, cb in ((s1, q1b, self.c1), (s2, q2b, self.c2)):
            step = max(1, int(block_elems) // max(1, k * cb.shape[1]))  # (query, leading index) pairs per block
            pairs_q = torch.arange(nq, device=self.device).repeat(L)      # pair p = (t, i) in the order of flat.view(L * nq, k)
            rows_all = flat.reshape(L * nq, k)
            flat_out = out.view(L * nq, k)
            for a in range(0, L * nq, step):
                rows = rows_all[a:a + step]
                q = qb[pairs_q[a:a + step]].float().unsqueeze(1)
                flat_out[a:a + step] = (cb[rows.clamp(min=0)].float() * q).sum(-1).masked_fill(rows < 0, float("-inf"))
        return s1.view(ids.shape), s2.view(ids.shape)


# ---- the reference's scripts -----------------------------------------------------------------------------------------------------------
def load_test_dataset(jsonl_dataset_path):
    with open(jsonl_dataset_path) as f:
        return [json.loads(line) for line in f]


_CTX_FIELDS = ("id", "title", "text")


def load_passages_tsv(tsv_passages_path):
    """The passages of a TSV whose first line names its columns (`id`, `text`, `title`, in any order), in file order: the vector in
    row r of the embeddings belongs to passages[r]."""
    with open(tsv_passages_path, newline="") as f:
        return [{k: row[k] for k in _CTX_FIELDS} for row in csv.DictReader(f, delimiter="\t")]


def _write_ranked(path, heads, passage_of, ids, **columns):
    """One JSON list, a record per query: the fields of heads[i] with `ctxs` put in (in place of an entry of that name, else behind the
    fields in front of `id`): the passages of ids[i] in rank order, each passage_of(row) (id, title, text) followed by one float per
    column, columns[name][i][rank].  Unfilled slots (row -1) are left out."""
    records = []
    for i, head in enumerate(heads):
        ctxs = [dict(passage_of(row), **{name: float(col[i][j]) for name, col in columns.items()}) for j, row in enumerate(ids[i]) if row >= 0]
        rec = {}
        for key, value in head.items():
            if key == "id" and "ctxs" not in head:
                rec["ctxs"] = ctxs
            rec[key] = ctxs if key == "ctxs" else value
        rec.setdefault("ctxs", ctxs)
        records.append(rec)
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(records, f, indent=4)


def _pool_queries(q1, q2, weight, pooling):
    if pooling == "concat":
        return torch.cat([q1, weight * q2], dim=-1)
    if pooling == "mean":
        return (q1 + weight * q2) / (1.0 + weight)
    return q1 + weight * q2


def _pool_passages(p1, p2, pooling):
    if pooling == "concat":
        return torch.cat([p1, p2], dim=-1)
    if pooling == "mean":
        return (p1 + p2) / 2.0
    return p1 + p2


def run_spar_retrieval(
    jsonl_dataset_paths,
    tsv_passages_path,
    ctx_embeddings_dir_1,
    ctx_embeddings_dir_2,
    output_dir,
    output_filenames,
    query_emb_names=["query_reps.pkl"],
    weights=None,
    save_embeddings=False,
    topk=100,
    pooling="concat",
    device=None,
    chunk=None,
    kernels=None,
):
    """spar_retrieval.py:101-222 with its keyword arguments and its files: one weight per dataset, one JSON list per dataset with
    `question`, `answers`, `id` and per ctx `id`, `title`, `text`, `score`.

    pooling='concat' searches the two indexes as they are (SparIndex): no concatenated corpus is built, the weight is applied to the fp32
    partial score instead of being rounded into the query vector.  'sum' / 'mean' mix the two models' features, which makes them ONE
    dense search: the vectors are pooled in fp32 with torch shard by shard and searched through hotpath.CorpusSearch; they need
    d1 == d2.  save_embeddings writes what the reference writes (the pooled query pickles; the pooled passages in 8 reps_000{i}.pkl
    shards) -- the only case in which the pooled corpus exists, on the host."""
    assert len(jsonl_dataset_paths) == len(query_emb_names) == len(output_filenames)
    if not weights:
        weights = [1.0] * len(jsonl_dataset_paths)
    assert len(weights) == len(query_emb_names)
    pooling = pooling.lower()
    if pooling not in ("concat", "mean", "sum"):
        raise ValueError(pooling)
    device = torch.device(device) if device is not None else torch.device("cuda", 0)
    kernels = _default_kernels(kernels)

    questions_list = [load_test_dataset(p) for p in jsonl_dataset_paths]
    passages = load_passages_tsv(tsv_passages_path)
    q1_list = [load_query_embeddings(ctx_embeddings_dir_1, n).float() for n in query_emb_names]
    q2_list = [load_query_embeddings(ctx_embeddings_dir_2, n).float() for n in query_emb_names]
    for questions, q1, q2 in zip(questions_list, q1_list, q2_list):
        assert len(questions) == len(q1) == len(q2)
    if pooling != "concat" and q1_list[0].shape[1] != q2_list[0].shape[1]:
        raise ValueError(f"pooling='{pooling}' adds the two models' vectors: widths {q1_list[0].shape[1]} and {q2_list[0].shape[1]} differ")

    os.makedirs(output_dir, exist_ok=True)
    if save_embeddings:
        for q1, q2, weight, name in zip(q1_list, q2_list, weights, query_emb_names):
            with open(os.path.join(output_dir, name), "wb") as ouf:
                pickle.dump(_pool_queries(q1, q2, weight, pooling), ouf, protocol=4)
        p = _pool_passages(load_passage_embeddings(ctx_embeddings_dir_1).float(), load_passage_embeddings(ctx_embeddings_dir_2).float(), pooling)
        assert len(passages) == len(p)
        num_shards = 8
        per = (len(p) // num_shards) + 1
        for i in range(num_shards):
            with open(os.path.join(output_dir, f"reps_000{i}.pkl"), "wb") as ouf:
                pickle.dump(torch.tensor(p[i * per:(i + 1) * per].numpy()), ouf, protocol=4)
        del p

    if pooling == "concat":
        index = SparIndex.from_dirs(ctx_embeddings_dir_1, ctx_embeddings_dir_2, device, chunk=chunk, kernels=kernels)
        assert len(passages) == index.corpus_len
        found = []
        for q1, q2, weight in zip(q1_list, q2_list, weights):
            v, i = index.search(q1, q2, weight, topk)
            found.append((v[0], i[0]))
    else:
        paths_1, paths_2 = shard_paths(ctx_embeddings_dir_1), shard_paths(ctx_embeddings_dir_2)
        searches = [hotpath.CorpusSearch(_pool_queries(q1, q2, w, pooling).to(device), topk, chunk=chunk, kernels=kernels)
                    for q1, q2, w in zip(q1_list, q2_list, weights)]
        # the two directories may be sharded differently: walk both, pool the rows they have in common, carry the rest over
        offset, rest_1, rest_2, it_1, it_2 = 0, None, None, iter(paths_1), iter(paths_2)
        while True:
            if rest_1 is None or len(rest_1) == 0:
                path = next(it_1, None)
                rest_1 = _load(path).float() if path is not None else None
            if rest_2 is None or len(rest_2) == 0:
                path = next(it_2, None)
                rest_2 = _load(path).float() if path is not None else None
            if rest_1 is None or rest_2 is None:
                assert rest_1 is None and rest_2 is None, "the two models must embed the same passages"
                break
            n = min(len(rest_1), len(rest_2))
            shard = _pool_passages(rest_1[:n].to(device), rest_2[:n].to(device), pooling)
            for s in searches:
                s.add(shard, offset)
            offset += n
            rest_1, rest_2 = rest_1[n:], rest_2[n:]
        assert len(passages) == offset
        found = [s.result() for s in searches]

    for questions, (v, i), name in zip(questions_list, found, output_filenames):
        # a record as the reference writes it: question, answers (none: an empty list), ctxs, id (none: the question's position)
        heads = [{"question": q["question"], "answers": q.get("answers", []), "id": q.get("id", str(n))} for n, q in enumerate(questions)]
        _write_ranked(os.path.join(output_dir, name), heads, lambda row: {k: passages[row][k] for k in _CTX_FIELDS}, i.cpu().tolist(),
                      score=v.cpu().tolist())


def grid_search_weights(
    ctx_emb_dir_1,
    ctx_emb_dir_2,
    pred_filename,
    query_reps_filename,
    weights=[0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.25, 1.43, 1.67, 2, 2.5, 3.33, 5.0, 10.0],
    output_dir=None,
    eval_on_ks=[1, 5, 10, 20, 50, 100],
    valid_on_k=100,
    regex=False,
    evaluate_retrieval=None,
    topk_out=200,
    device=None,
    chunk=None,
    kernels=None,
    index=None,
    tsv_passages_path=None,
):
    """spar_weight_tuning.py:127-197 with its keyword arguments, its weight{w}_{pred_filename} files (per ctx `score`, `score_1`,
    `score_2`) and its {pred_filename}.log; returns (best weight, its top-valid_on_k accuracy).

    NOT the reference's ranking: the reference cannot afford a search per weight and re-ranks, for every weight, the joint pool of each
    model's own top-100 (spar_weight_tuning.py:53-124), an approximation.  Here ONE index.search with all weights returns the EXACT
    top-topk_out of every weight over the whole corpus.  The two agree wherever a weight's exact winners lie inside that pool.

    Questions and answers are read from the prediction file of model 1 ({ctx_emb_dir_1}/{pred_filename}).  The exact winners are not
    confined to anybody's earlier lists -- for a large weight they are the lexical model's finds, which model 1's lists miss --, and
    the evaluation decides a hit by the passage TEXT, so every selected passage needs its text: pass tsv_passages_path (the corpus,
    row r = passage r; the source that covers every id).  Without it the texts are taken, as the reference takes them, from both
    models' prediction files ({ctx_emb_dir_2}/{pred_filename} too, where it exists; a ctx's `id` there is its passage row + 1, :91),
    and a selected passage that neither file holds raises LookupError: no record is ever written with an empty text.
    evaluate_retrieval(path, eval_on_ks, regex) -> {k: per-question hits} is the reference's dpr_scale.eval_dpr function, passed in;
    without it the files are written and nothing is selected (returns (None, None))."""
    assert valid_on_k in eval_on_ks, "The validation criterion is not evaluated."
    if not output_dir:
        output_dir = tempfile.mkdtemp()
    os.makedirs(output_dir, exist_ok=True)
    output_paths = [os.path.join(output_dir, f"weight{w}_{pred_filename}") for w in weights]

    with open(os.path.join(ctx_emb_dir_1, pred_filename)) as inf:
        data = json.load(inf)
    if tsv_passages_path is not None:
        passages = load_passages_tsv(tsv_passages_path)
        passage_of = lambda row: passages[row]
    else:
        known = {}
        for d in (ctx_emb_dir_2, ctx_emb_dir_1):
            path = os.path.join(d, pred_filename)
            if d == ctx_emb_dir_1 or os.path.isfile(path):
                with open(path) as inf:
                    for q in json.load(inf):
                        known.update((ctx["id"], {k: ctx[k] for k in _CTX_FIELDS}) for ctx in q["ctxs"])

        def passage_of(row):
            if str(row + 1) not in known:
                raise LookupError(f"passage id {row + 1} is among the exact winners but in neither model's {pred_filename}: "
                                  "pass tsv_passages_path (the evaluation needs its text)")
            return known[str(row + 1)]

    if index is None:
        device = torch.device(device) if device is not None else torch.device("cuda", 0)
        index = SparIndex.from_dirs(ctx_emb_dir_1, ctx_emb_dir_2, device, chunk=chunk, kernels=kernels)
    if tsv_passages_path is not None and len(passages) != index.corpus_len:
        raise ValueError(f"{tsv_passages_path} holds {len(passages)} passages, the index {index.corpus_len}")
    q1 = load_query_embeddings(ctx_emb_dir_1, query_reps_filename)
    q2 = load_query_embeddings(ctx_emb_dir_2, query_reps_filename)
    assert len(data) == len(q1) == len(q2)
    k = min(int(topk_out), index.corpus_len)
    values, ids = index.search(q1, q2, weights, k)
    s1, s2 = index.partial_scores(q1, q2, ids)
    values, ids, s1, s2 = values.cpu().tolist(), ids.cpu().tolist(), s1.cpu().tolist(), s2.cpu().tolist()
    for w, path in enumerate(output_paths):
        _write_ranked(path, data, passage_of, ids[w], score=values[w], score_1=s1[w], score_2=s2[w])
    if evaluate_retrieval is None:
        return None, None

    mean = lambda xs: float(sum(xs)) / len(xs) if hasattr(xs, "__len__") else float(xs)
    accuracies = [{kk: mean(v) for kk, v in evaluate_retrieval(p, eval_on_ks, regex).items()} for p in output_paths]
    best_acc, best_weight, best_acc_all = -1.0, -1.0, -1.0
    with open(os.path.join(output_dir, f"{pred_filename}.log"), "w") as log_file:
        for weight, acc in zip(weights, accuracies):
            print("Accuracy for weight", weight, "is:", acc, file=log_file)
            acc_k = acc[valid_on_k]
            acc_all = sum(acc[kk] * kk for kk in eval_on_ks) / len(eval_on_ks)
            print(f"Top-{valid_on_k} accuracy for weight", weight, "is", acc_k, file=log_file)
            if acc_k > best_acc or (acc_k > best_acc - 1e-8 and acc_all > best_acc_all):  # :179-186
                best_acc, best_weight, best_acc_all = acc_k, weight, acc_all
        print(f"The best weight for {pred_filename} is", best_weight, f"with top-{valid_on_k} accuracy of {best_acc}", file=log_file)
    return best_weight, best_acc
