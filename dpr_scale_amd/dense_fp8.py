"""The fp8 dense index (csrc/dense_fp8.h): a DPR corpus resident on the device as OCP e4m3fn codes with one
power-of-two scale per row -- d + 4 bytes per passage where the bf16 rows that hotpath.CorpusSearch streams take 2 d --, searched by a
GEMM-shaped kernel on the fp8 MFMA path.  No codebook, no training; queries are quantised by the same rule as the passages.

    index = DenseFP8Index.from_dirs(ctx_embeddings_dir, device)          # or DenseFP8Index(vectors, device) / .from_codes(codes, scale, d)
    values, ids = index.search(q, topk)                                  # [nq, topk] fp32 / int64, best first, ties to the lower id
    values, ids = index.search(q, topk, refine=4)                        # 4 * topk fp8 candidates re-scored on the exact rows (exact_rows=)

    s[i][j] = (sum_t value(qc[i][t]) * value(cc[j][t]) * sq[i]) * sc[j]

The format (include/dprhot.h): codes uint8 [n, dp], dp = round_up(d, 32), zero behind d; scale fp32 [n] = 2^e, the smallest power of
two with max |x_t| <= 448 * scale (e clamped to [-64, 64]); code_t = e4m3fn(x_t / scale), round to nearest even.  A row of zeros has scale
1; a row with a non-finite element has scale NaN, all its scores are NaN and it is never selected.  Every decoded value of a finite row
is exact in bf16, so decode() is a true bf16 corpus that the bf16 kernels score as the fp8 kernel does."""
import torch

from ._chunked import ChunkedIndex, _default_kernels
from .spar import _load, shard_paths

FORMAT = "dpr_scale_amd.dense_fp8/1"
BLOCK_ROWS = 1 << 16  # rows encoded per call: what the device holds in fp32 / bf16 next to the codes (200 MB at d = 768)
FEW_QUERIES = 32      # up to here a search streams the codes once (the kernel's 32-row tile) and its launches are latency-bound
HEAD_IDS = 65536      # ... and an empty state is started from at most this many passages: the library selects the top-k of the first
                      # range it is given from a materialised score matrix, ONE workgroup per query walking all of it (242 us for
                      # 262144 ids, where the kernel that scores them takes 41); 1 M x 768, k = 100, ms per search by head size:
                      # nq = 1: 8192 0.41, 16384 0.40, 65536 0.39, 262144 0.47; nq = 32: 0.86, 0.65, 0.49, 0.50 (a short head leaves
                      # a weak threshold and long candidate lists); nq = 1024: 3.55, 2.81, 2.16, 2.12 -- no gain, so not applied there


def padded_width(d):
    return (int(d) + 31) // 32 * 32


def _rows(x):
    """fp32 or bf16 as they are, everything else as fp32 -- the two dtypes dprhot_fp8_encode reads."""
    x = torch.as_tensor(x)
    return x if x.dtype in (torch.float32, torch.bfloat16) else x.float()


def encode_rows(kn, x, dp, device, block_rows=BLOCK_ROWS):
    """(codes uint8 [n, dp], scale fp32 [n]) on `device` of the rows x [n, d] (host or device), block by block."""
    n = x.shape[0]
    codes = torch.empty((n, dp), dtype=torch.uint8, device=device)
    scale = torch.empty((n,), dtype=torch.float32, device=device)
    for a in range(0, n, block_rows):
        kn.fp8_encode(x[a:a + block_rows].to(device).contiguous(), codes[a:a + block_rows], scale[a:a + block_rows])
    return codes, scale


class DenseFP8Index(ChunkedIndex):
    """A dense corpus as e4m3fn codes + one scale per row on the device; passage id = row."""

    def __init__(self, p_vectors, device=None, chunk=None, kernels=None, exact_rows=None, block_rows=BLOCK_ROWS):
        """p_vectors [n, d], host or device, any float type: encoded on the device block_rows rows at a time, so the device never holds
        more than one block of them in fp32 / bf16.  exact_rows [n, d] (host or device, bf16 or fp32; p_vectors itself is a natural
        choice) is kept as it is for search(refine=)."""
        p = _rows(p_vectors)
        if p.dim() != 2 or p.shape[0] == 0 or p.shape[1] == 0:
            raise ValueError(f"passage vectors must be a non-empty [n, d] matrix, got {tuple(p.shape)}")
        device = torch.device(device) if device is not None else p.device
        kn = _default_kernels(kernels)
        codes, scale = encode_rows(kn, p, padded_width(p.shape[1]), device, int(block_rows))
        self._init(codes, scale, int(p.shape[1]), chunk, kn, exact_rows)

    def _init(self, codes, scale, d, chunk, kernels, exact_rows):
        self.device = codes.device
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.codes, self.scale = codes, scale
        self.corpus_len, self.d, self.dp = int(codes.shape[0]), int(d), int(codes.shape[1])
        if exact_rows is not None:
            exact_rows = _rows(exact_rows)
            if tuple(exact_rows.shape) != (self.corpus_len, self.d):
                raise ValueError(f"exact_rows {tuple(exact_rows.shape)} for an index of {self.corpus_len} x {self.d}")
        self.exact_rows = exact_rows
        self.head = HEAD_IDS
        self._init_search(chunk, kernels)

    @classmethod
    def from_codes(cls, codes, scale, d, device=None, chunk=None, kernels=None, exact_rows=None):
        """An already encoded corpus: codes uint8 [n, round_up(d, 32)], scale fp32 [n]."""
        codes, scale = torch.as_tensor(codes), torch.as_tensor(scale)
        if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[0] == 0 or codes.shape[1] != padded_width(d) or not 1 <= d:
            raise ValueError(f"codes must be uint8 [n, {padded_width(d)}] for d = {d}, got {codes.dtype} {tuple(codes.shape)}")
        if scale.dtype != torch.float32 or tuple(scale.shape) != (codes.shape[0],):
            raise ValueError(f"scale must be fp32 [{codes.shape[0]}], got {scale.dtype} {tuple(scale.shape)}")
        device = torch.device(device) if device is not None else codes.device
        self = cls.__new__(cls)
        self._init(codes.to(device).contiguous(), scale.to(device).contiguous(), int(d), chunk, kernels, exact_rows)
        return self

    @classmethod
    def from_dirs(cls, ctx_embeddings_dir, device=None, chunk=None, kernels=None, keep_exact=False, block_rows=BLOCK_ROWS):
        """Every reps_* pickle in sorted order, rows concatenated only (the SPAR reading of a directory: no zero rows behind a short
        file).  The host holds one file at a time: a file is read, encoded on the device and released; the row count is only known
        after the last file, so the device holds the codes twice while the pieces are joined.  keep_exact keeps every file on the host
        and joins them into exact_rows for search(refine=)."""
        device = torch.device(device) if device is not None else torch.device("cuda", 0)
        kn = _default_kernels(kernels)
        pieces, exact, width = [], [], None
        for path in shard_paths(ctx_embeddings_dir):
            shard = _rows(_load(path))
            if width is None:
                width = int(shard.shape[1])
            elif int(shard.shape[1]) != width:
                raise ValueError(f"{path}: {shard.shape[1]} columns where the files before it have {width}")
            pieces.append(encode_rows(kn, shard, padded_width(width), device, int(block_rows)))
            if keep_exact:
                exact.append(shard)
            del shard
        codes = pieces[0][0] if len(pieces) == 1 else torch.cat([c for c, _ in pieces], dim=0)
        scale = pieces[0][1] if len(pieces) == 1 else torch.cat([s for _, s in pieces], dim=0)
        del pieces
        return cls.from_codes(codes, scale, width, device, chunk=chunk, kernels=kn, exact_rows=torch.cat(exact, dim=0) if keep_exact else None)

    def default_chunk(self, nq):
        """Passage ids per pass: the workspace holds a candidate value and a column per query and id (8 bytes; at most 1 GiB by
        default, at least 1024 ids) -- a 128-wide column tile per compute unit wants thousands of ids."""
        c = self.chunk if self.chunk is not None else max(1024, min(262144, (1 << 27) // max(nq, 1)))
        c = min(c, (self.corpus_len + 7) // 8 * 8)
        return max(8, c // 8 * 8)

    # ---- what the index holds ---------------------------------------------------------------------------------------------------------
    @property
    def nbytes(self):
        """Bytes of the resident index: the codes and the scales (exact_rows, where given, are the caller's)."""
        return self.codes.numel() + 4 * self.scale.numel()

    def decode(self, block_rows=BLOCK_ROWS):
        """bf16 [n, dp]: value(code) * scale, exact for every finite row (a row of scale NaN decodes to NaN)."""
        out = torch.empty((self.corpus_len, self.dp), dtype=torch.bfloat16, device=self.device)
        for a in range(0, self.corpus_len, block_rows):
            v = self.codes[a:a + block_rows].view(torch.float8_e4m3fn).float()
            out[a:a + block_rows] = (v * self.scale[a:a + block_rows, None]).to(torch.bfloat16)
        return out

    def save(self, path):
        torch.save({"format": FORMAT, "d": self.d, "codes": self.codes.cpu(), "scale": self.scale.cpu()}, path)

    @classmethod
    def load(cls, path, device=None, chunk=None, kernels=None, exact_rows=None):
        blob = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(blob, dict) or blob.get("format") != FORMAT:
            raise ValueError(f"{path} is not a {FORMAT} file")
        return cls.from_codes(blob["codes"], blob["scale"], int(blob["d"]), device, chunk=chunk, kernels=kernels, exact_rows=exact_rows)

    # ---- search -----------------------------------------------------------------------------------------------------------------------
    def _queries(self, q):
        """(codes [nq, dp], scale [nq]) of the queries, quantised by the passages' rule."""
        q = _rows(q)
        if q.dim() != 2 or q.shape[0] == 0 or q.shape[1] != self.d:
            raise ValueError(f"queries {tuple(q.shape)} do not fit an index of width {self.d}")
        return encode_rows(self._kernels(), q, self.dp, self.device)

    def _search_fp8(self, qc, qs, topk, id_ranges, chunk):
        kn = self._kernels()
        nq = qc.shape[0]
        if nq <= FEW_QUERIES:  # the head of the empty state as an id range of its own: the same result, a shorter selection
            id_ranges = list(id_ranges) if id_ranges is not None else [(0, self.corpus_len)]
            b, e = int(id_ranges[0][0]), int(id_ranges[0][1])
            if e - b > self.head:
                id_ranges = [(b, b + self.head), (b + self.head, e)] + id_ranges[1:]
        return self._fold(nq, topk, id_ranges, chunk, lambda c: kn.dense_fp8_workspace(nq, c, topk, qc),
                          lambda b, e, values, indices, first, c, ws: kn.dense_fp8_search(self, qc, qs, b, e, values, indices, first, c, ws))

    def search(self, q, topk, id_ranges=None, chunk=None, refine=None):
        """(values [nq, topk] fp32, ids [nq, topk] int64): the top-k of the fp8 score over the disjoint (begin, end) passage-id ranges
        (default: the whole corpus), best first, ties to the lower id, a NaN score never selected, -inf / -1 where fewer than topk
        candidates exist.  refine=r (int >= 1): min(r * topk, corpus_len) fp8 candidates are taken, their exact_rows gathered and scored
        against the unquantised queries in fp32 with torch, and the best topk of THOSE scores returned under the same order."""
        topk = int(topk)
        qc, qs = self._queries(q)
        if refine is None:
            return self._search_fp8(qc, qs, topk, id_ranges, chunk)
        if int(refine) != refine or int(refine) < 1:
            raise ValueError(f"refine={refine!r} must be an integer >= 1")
        if self.exact_rows is None:
            raise ValueError("search(refine=) re-scores on the exact rows: pass exact_rows= when the index is built")
        if not 1 <= topk <= self.corpus_len:
            raise ValueError(f"topk={topk} out of range (1 .. corpus_len={self.corpus_len})")
        _, cand = self._search_fp8(qc, qs, min(int(refine) * topk, self.corpus_len), id_ranges, chunk)
        return self._refine(_rows(q), cand, topk)

    def _refine(self, q, cand, topk, block_elems=1 << 24):
        """The best topk of cand [nq, m] (-1 = no candidate) by the fp32 score of the exact rows: score descending, id ascending."""
        nq, m = cand.shape
        q = q.to(self.device).float()
        s = torch.empty((nq, m), dtype=torch.float32, device=self.device)
        step = max(1, int(block_elems) // max(1, m * self.d))  # queries per block: a gathered fp32 block stays near block_elems elements
        for a in range(0, nq, step):
            ids = cand[a:a + step].clamp(min=0)
            rows = self.exact_rows[ids.to(self.exact_rows.device)].to(self.device).float()  # [step, m, d]
            s[a:a + step] = (rows * q[a:a + step, None, :]).sum(-1)
        gone = (cand < 0) | torch.isnan(s)
        s = s.masked_fill(gone, float("-inf"))
        ids = cand.masked_fill(gone, torch.iinfo(torch.int64).max)
        ids, order = torch.sort(ids, dim=1, stable=True)              # id ascending ...
        s = torch.gather(s, 1, order)
        gone = torch.gather(gone, 1, order)
        s, order = torch.sort(s, dim=1, descending=True, stable=True)  # ... inside every group of equal scores
        ids = torch.gather(ids, 1, order).masked_fill(torch.gather(gone, 1, order), -1)
        return s[:, :topk].contiguous(), ids[:, :topk].contiguous()

    def score(self, q, doc_begin=0, cols=None):
        """S [nq, cols] fp32 of passages doc_begin .. doc_begin + cols (default: to the end), the scores `search` ranks."""
        kn = self._kernels()
        qc, qs = self._queries(q)
        cols = self.corpus_len - doc_begin if cols is None else int(cols)
        S = torch.empty((qc.shape[0], (cols + 7) // 8 * 8), dtype=torch.float32, device=self.device)
        kn.dense_fp8_score(self, qc, qs, int(doc_begin), cols, S)
        return S[:, :cols]
