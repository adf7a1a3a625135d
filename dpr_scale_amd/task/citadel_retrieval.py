"""Drop-in for dpr_scale.task.citadel_retrieval_task.CITADELRetrievalTask (reference: dpr_scale/task/citadel_retrieval_task.py).

Same constructor kwargs (:15-30), `_eval_step` (:84-140), `test_epoch_end` (:145-177), `merge_trec_results` (:179-201) and
`merge_qa_results` (:204-231).  The reference builds `self.index` from dpr_scale/index/inverted_vector_index.py, which it does not
ship; here the index is dpr_scale_amd.ivf.load_index (one device-resident inverted index, scored by libdprhot.so).  Query batches whose
repr tensors are on the index's device are packed there (ivf.pack_queries_device; `device_pack = False` keeps the host loop).

Scope: `cuda=False`, `portion` below 1.0 and `hnsw_index` raise NotImplementedError; `expert_parallel` (the reference's split of
experts across GPUs) is accepted and ignored: the index lives on one device.  `quantizer="pq"` raises NotImplementedError in
CITADELRetrievalTask, whose index is the plain one, and is what CITADELPQRetrievalTask is for: the same task over an
ivf.IVFPQIndex (8-bit codes over sub-vectors of `sub_vec_dim` in {2, 4, 8} features).
"""
import collections
import json
import os
import time

import torch

from .. import ivf
from .citadel_task import MultiVecRetrieverTask

_SCOPE = "inverted-index retrieval supports the plain GPU index only (no product quantisation, CPU index, partial index or hnsw)"


class PassageTable:
    """The passages file of the reference's IDCSVDataset(path, use_id=True): a tab-separated file with a header row and an `id`
    column; rows are looked up by their id string."""

    def __init__(self, path, sep="\t"):
        self.rows = {}
        with open(path, encoding="utf-8") as f:
            self.columns = self._parse(f.readline(), sep)
            for line in f:
                vals = self._parse(line, sep)
                if len(vals) == len(self.columns):
                    row = dict(zip(self.columns, vals))
                    self.rows[row["id"]] = row

    @staticmethod
    def _parse(line, sep):
        row = line.rstrip("\r\n").split(sep)
        return [v.strip('"').replace('""', '"') if v and v[0] == '"' and v[-1] == '"' else v for v in row]

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, key):
        return self.rows[key]


class CITADELRetrievalTask(MultiVecRetrieverTask):
    device_pack = True  # pack query batches on the device when the encoder outputs and the index live there (False: the host loop)

    def __init__(
        self,
        ctx_embeddings_dir,
        checkpoint_path,
        index2docid_path=None,
        hnsw_index=False,
        output_path="/tmp/results.jsonl",
        passages="",
        topk=100,
        cuda=True,
        portion=1.0,
        quantizer=None,
        sub_vec_dim=4,
        expert_parallel=True,
        **kwargs,
    ):
        super().__init__(**kwargs)
        self.ctx_embeddings_dir = ctx_embeddings_dir
        self.checkpoint_path = checkpoint_path
        self.index2docid_path = index2docid_path
        self.hnsw_index = hnsw_index
        self.output_path = output_path
        self.passages = passages
        self.topk = topk
        self.cuda = cuda
        self.quantizer = quantizer if quantizer != "None" else None
        self.sub_vec_dim = sub_vec_dim
        self.portion = portion
        self.expert_parallel = expert_parallel
        self.latency = collections.defaultdict(float)
        if self.quantizer == "pq":
            raise NotImplementedError(f'quantizer="pq": {_SCOPE}')
        if self.quantizer is not None:
            raise NotImplementedError(f"quantizer={self.quantizer!r}: {_SCOPE}")
        if not self.cuda:
            raise NotImplementedError(f"cuda=False: {_SCOPE}")
        if self.portion != 1.0 or self.hnsw_index:
            raise NotImplementedError(f"portion={self.portion}, hnsw_index={self.hnsw_index}: {_SCOPE}")

    def setup(self, stage: str):
        super().setup("train")
        print(f"Loading checkpoint from {self.checkpoint_path}")
        checkpoint = torch.load(self.checkpoint_path, map_location="cpu", weights_only=False)
        self.load_state_dict(checkpoint["state_dict"])
        print(f"Loading passages from {self.passages}")
        self.ctxs = PassageTable(self.passages)
        print("Setting up index...")
        self.index = self._load_index(self.device if self.device.type == "cuda" else None)

    def _load_index(self, device):
        return ivf.load_index(self.ctx_embeddings_dir, len(self.ctxs), device)

    def forward(self, query_ids):
        return self.encode_queries(query_ids)

    def _eval_step(self, batch, batch_idx):
        tic = time.perf_counter()
        query_ids = batch["query_ids"]
        topic_ids = batch["topic_ids"] if "topic_ids" in batch else []
        answers = batch["answers"] if "answers" in batch else []
        questions = batch["question"] if "question" in batch else []
        queries_repr = {k: v.detach() for k, v in self(query_ids).items()}
        n = len(topic_ids) if len(topic_ids) > 0 else len(query_ids["input_ids"])
        batch_top_scores, batch_top_ids = self._search(queries_repr, n, tic)
        return batch_top_scores.cpu().tolist(), batch_top_ids.cpu().tolist(), topic_ids, questions, answers

    def _search(self, queries_repr, n, tic):
        """(scores, ids) of the first n queries of the batch; `tic` is when the step began (encode_time runs up to the search)."""
        batch_cls = queries_repr["cls_repr"] if "cls_repr" in queries_repr else []
        if self.device_pack and queries_repr["expert_repr"].is_cuda and self.index.device.type == "cuda":
            # the batch is packed where the encoder left it (ivf.pack_queries_device): same tensors as the host path below, bit for bit
            qb = ivf.pack_queries_device(queries_repr, batch_cls, n, kernels=self.index._kernels())
            self.latency["encode_time"] += time.perf_counter() - tic
            tic = time.perf_counter()
            batch_top_scores, batch_top_ids = self.index.search_packed(qb, self.topk)
            self.index.latency["search_time"] += time.perf_counter() - tic
            return batch_top_scores, batch_top_ids
        batch_embeddings, batch_weights = ivf.query_dicts(queries_repr, n)
        self.latency["encode_time"] += time.perf_counter() - tic
        return self.index.search(batch_cls, batch_embeddings, batch_weights, self.topk)

    def test_step(self, batch, batch_idx):
        return self._eval_step(batch, batch_idx)

    def test_epoch_end(self, queries_reprs):
        top_scores, top_ids, topic_ids, questions, answers = [], [], [], [], []
        for b_scores, b_ids, b_topics, b_questions, b_answers in queries_reprs:
            top_scores.extend(b_scores)
            top_ids.extend(b_ids)
            topic_ids.extend(b_topics)
            questions.extend(b_questions)
            answers.extend(b_answers)
        self.latency["encode_time"] += self.index.latency["encode_time"]
        self.index.latency.pop("encode_time")
        print(dict(self.latency))
        print(dict(self.index.latency))
        if len(topic_ids) > 0:
            lines = self.merge_trec_results(topic_ids, top_ids, top_scores)
            os.makedirs(self.output_path, exist_ok=True)
            with open(os.path.join(self.output_path, f"retrieval_{self.global_rank:04}.trec"), "w") as g:
                g.writelines(lines)
        elif len(answers) > 0:
            qa = self.merge_qa_results(questions, answers, top_ids, top_scores)
            os.makedirs(self.output_path, exist_ok=True)
            with open(os.path.join(self.output_path, f"retrieval_{self.global_rank:04}.json"), "w") as g:
                g.write(json.dumps(qa, indent=4))
                g.write("\n")
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.barrier()

    def merge_trec_results(self, topic_ids, top_doc_ids, scores_list):
        i2d = []
        if self.index2docid_path is not None and os.path.exists(self.index2docid_path):
            with open(self.index2docid_path) as f:
                i2d = [line.strip() for line in f]
        assert len(top_doc_ids) == len(topic_ids) == len(scores_list)
        out = []
        for topic_id, doc_ids, scores in zip(topic_ids, top_doc_ids, scores_list):
            for rank, (doc_id, score) in enumerate(zip(doc_ids, scores)):
                name = i2d[doc_id] if i2d else doc_id
                out.append(f"{topic_id} Q0 {name} {rank + 1} {score:.6f} dpr-scale\n")
        return out

    def merge_qa_results(self, questions, answers, top_doc_ids, scores_list):
        assert len(top_doc_ids) == len(answers) == len(scores_list)
        out = []
        for question, answer, doc_ids, scores in zip(questions, answers, top_doc_ids, scores_list):
            ctxs = []
            for doc_id, score in zip(doc_ids, scores):
                row = self.ctxs[str(doc_id)]
                ctxs.append({"id": row["id"], "title": row["title"], "text": row["text"], "score": float(score)})
            out.append({"question": question, "answers": answer, "ctxs": ctxs})
        return out


class CITADELPQRetrievalTask(CITADELRetrievalTask):
    """CITADELRetrievalTask with quantizer="pq": same constructor kwargs, same _eval_step, over a product-quantised index.  `setup`
    loads `ctx_embeddings_dir/pq_index.pt` when that file exists (ivf.load_pq_index); otherwise it builds the plain index, trains a
    codebook on it and encodes it (ivf.load_index(..., quantizer="pq")) -- and writes the file when `save_quantized` is set, so that
    a large index is not retrained at every start."""

    save_quantized = False  # write ctx_embeddings_dir/pq_index.pt after quantising (True: the next setup loads it)
    PQ_FILE = "pq_index.pt"

    def __init__(self, *args, quantizer="pq", sub_vec_dim=4, **kwargs):
        if quantizer != "pq":
            raise NotImplementedError(f'quantizer={quantizer!r}: CITADELPQRetrievalTask is the quantizer="pq" task '
                                      f"(CITADELRetrievalTask takes the plain index)")
        if sub_vec_dim not in ivf.PQ_SUB_VEC_DIMS:
            raise NotImplementedError(f"sub_vec_dim={sub_vec_dim}: sub-vectors of {ivf.PQ_SUB_VEC_DIMS} features")
        super().__init__(*args, quantizer=None, sub_vec_dim=sub_vec_dim, **kwargs)  # refuses what the plain task refuses
        self.quantizer = "pq"

    def _load_index(self, device):
        path = os.path.join(self.ctx_embeddings_dir, self.PQ_FILE)
        if os.path.exists(path):
            index = ivf.load_pq_index(path, device)
            if index.corpus_len != len(self.ctxs) or index.dsub != self.sub_vec_dim:
                raise ValueError(f"{path}: an index of {index.corpus_len} passages with sub_vec_dim={index.dsub}; "
                                 f"{len(self.ctxs)} passages and sub_vec_dim={self.sub_vec_dim} were asked for")
            return index
        index = ivf.load_index(self.ctx_embeddings_dir, len(self.ctxs), device, quantizer="pq", sub_vec_dim=self.sub_vec_dim)
        if self.save_quantized:
            index.save(path)
        return index
