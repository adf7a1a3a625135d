"""Exhaustive ColBERT search (dpr_scale_amd/colbert.py, csrc/colbert.h) over a synthetic corpus with a long-tailed passage length
(mean about 70 tokens, at most 180, d = 128), three arms on the same GPU, the same index and the same queries:

  fused    ColBERTIndex.search: dprhot_colbert_search over the packed token index
  maxsim   what the library offered before it: the corpus padded to one LD (resident, built once outside the timing), chunks through
           dprhot_maxsim_fwd in in-batch mode, a clamp at 0, dprhot_topk_update
  torch    torch ops on the padded corpus: chunked einsum -> amax -> clamp -> sum -> top-k merge

Before timing the fused arm's scores and ids are held against the maxsim arm's under the rounding bound of tests/test_colbert_gpu.py
(both are within (dp + LQ + 1) * 2^-23 * A of the exact score, A bounded here by Cauchy-Schwarz).  Arms alternate in one process;
medians (and minima) after warm-up; one JSON line per shape and k, appended to profiles/colbert_bench.jsonl.  Reported besides:
peak memory above the resident index per arm, the score kernel alone (device events around dprhot_colbert_score over the corpus) as
algorithmic FLOP/s (2 * nq * LQ * T * dp) against the bf16 MFMA peak and as token bytes per second against HBM.  Kernel times by
name: `rocprofv3 --kernel-trace --stats -- python bench_colbert.py --score-only --only NAME`.

    python bench_colbert.py [--steps 10] [--warmup 2] [--only NAME] [--fused-only] [--score-only] [--no-torch]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SHAPES = [
    dict(name="100k", docs=100_000, nq=32, LQ=32, d=128),
    dict(name="1m", docs=1_000_000, nq=32, LQ=32, d=128),
    dict(name="1m_1q", docs=1_000_000, nq=1, LQ=32, d=128),
]
MAX_LEN, LD_PAD = 180, 184          # LD_PAD > MAX_LEN: every padded passage keeps a padded slot (the arms then compute the same score)
PEAK_BF16_FLOPS, PEAK_HBM_BPS = 2.5e15, 8.0e12  # MI355X data sheet: dense bf16 MFMA, HBM3E


def make(sh, dev, seed=0):
    from dpr_scale_amd import colbert

    g = torch.Generator(device=dev).manual_seed(seed)
    N, d = sh["docs"], sh["d"]
    lens = torch.exp(torch.randn(N, generator=g, device=dev) * 0.5 + 4.127).round().clamp_(1, MAX_LEN).long()  # lognormal, median 62
    nblk = (lens + 15) // 16
    doc_blk = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(nblk, 0)]).contiguous()
    n_blk = int(doc_blk[-1])
    tok = torch.empty((n_blk * 16, d), dtype=torch.bfloat16, device=dev)
    for a in range(0, n_blk * 16, 1 << 22):
        tok[a:a + (1 << 22)] = torch.randn((min(1 << 22, n_blk * 16 - a), d), generator=g, device=dev) / d ** 0.5
    blk_doc = torch.repeat_interleave(torch.arange(N, device=dev), nblk)
    valid = lens[blk_doc] - 16 * (torch.arange(n_blk, device=dev) - doc_blk[blk_doc])
    tok.view(n_blk, 16, d).mul_((torch.arange(16, device=dev)[None, :] < valid[:, None]).unsqueeze(-1))  # zero rows behind a passage
    return colbert.ColBERTIndex.from_packed(tok, doc_blk, N, d), lens


def padded_corpus(index, lens):
    """bf16 [N, LD_PAD, dp]: what the maxsim and torch arms keep resident instead of the packed index."""
    N, dev = index.corpus_len, index.device
    out = torch.zeros((N, LD_PAD, index.dp), dtype=torch.bfloat16, device=dev)
    step = 1 << 16
    for a in range(0, N, step):
        b = min(N, a + step)
        j = torch.arange(LD_PAD, device=dev)[None, :]
        src = index.doc_blk[a:b, None] * 16 + j
        ok = j < lens[a:b, None]
        out[a:b][ok] = index.tok[src[ok]]
    return out


class MaxsimArm:
    """Padded chunks through dprhot_maxsim_fwd (in-batch), clamp, dprhot_topk_update."""

    def __init__(self, kn, Cpad, q, chunk):
        self.kn, self.C, self.q, self.chunk = kn, Cpad, q, chunk

    def __call__(self, k):
        nq, N = self.q.shape[0], self.C.shape[0]
        values = torch.empty((nq, k), dtype=torch.float32, device=self.q.device)
        indices = torch.empty((nq, k), dtype=torch.int64, device=self.q.device)
        for j0 in range(0, N, self.chunk):
            c = self.C[j0:j0 + self.chunk]
            S, _ = self.kn.maxsim_fwd(self.q, c, None, None, None, None, 1, 1, 0, 0, None)
            S.clamp_(min=0)
            self.kn.topk_update(S, c.shape[0], j0, values, indices, j0 == 0)
        return values, indices


def torch_arm(Cpad, q, k, chunk):
    best_v = best_i = None
    for j0 in range(0, Cpad.shape[0], chunk):
        c = Cpad[j0:j0 + chunk]
        s = torch.einsum("nid,cjd->ncij", q, c).amax(-1).clamp_(min=0).float().sum(-1)
        v, i = torch.topk(s, min(k, s.shape[1]), dim=1)
        i = i + j0
        if best_v is not None:
            v, sel = torch.topk(torch.cat([best_v, v], 1), min(k, best_v.shape[1] + v.shape[1]), dim=1)
            i = torch.gather(torch.cat([best_i, i], 1), 1, sel)
        best_v, best_i = v, i
    return best_v, best_i


def score_only(index, q, chunk):
    """dprhot_colbert_score over the whole corpus in chunks (no top-k): the launches whose time the FLOP/s figure is about."""
    kn = index._kernels()
    S = torch.empty((q.shape[0], chunk), dtype=torch.float32, device=index.device)
    for j0 in range(0, index.corpus_len, chunk):
        kn.colbert_score(index, q, 0, j0, min(chunk, index.corpus_len - j0), S)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--score-only", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colbert_bench.jsonl"))
    a = ap.parse_args()
    from dpr_scale_amd import hotpath

    dev = torch.device("cuda", 0)
    kn = hotpath.default_kernels()
    made = {}
    for sh in SHAPES:
        if a.only and sh["name"] != a.only:
            continue
        key = sh["docs"]
        if key not in made:  # the 1-query row searches the index of the 1 M shape
            made.clear()
            torch.cuda.empty_cache()
            index, lens = make(sh, dev)
            made[key] = (index, lens, None if (a.fused_only or a.score_only) else padded_corpus(index, lens))
        index, lens, Cpad = made[key]
        g = torch.Generator(device=dev).manual_seed(1)
        q = (torch.randn((sh["nq"], sh["LQ"], sh["d"]), generator=g, device=dev) / sh["d"] ** 0.5).to(torch.bfloat16)
        q[0, -3:] = 0  # padded query tokens
        nq, LQ, dp, T = sh["nq"], sh["LQ"], index.dp, int(lens.sum())
        chunk = index.default_chunk(nq)
        score_ms = event_ms(lambda: score_only(index, q, chunk), max(a.steps, 5) + a.warmup)[a.warmup:]
        if a.score_only:
            print(json.dumps(dict(bench="colbert_score", shape=sh["name"], score_ms=med(score_ms))), flush=True)
            continue
        for k in (100, 1000):
            arms = {"fused": lambda: index.search(q, k)}
            check = None
            if Cpad is not None:
                mchunk = 8192 if nq > 1 else 65536
                marm = MaxsimArm(kn, Cpad, q, mchunk)
                arms["maxsim"] = lambda: marm(k)
                arms["maxsim_again"] = lambda: marm(k)  # the bar against itself: the run-to-run spread
                if not a.no_torch:
                    arms["torch"] = lambda: torch_arm(Cpad, q, k, 2048 if nq > 1 else 16384)
                (fv, fi), (mv, mi) = arms["fused"](), arms["maxsim"]()
                # A[n, doc] <= sum_i |q_i| * max_row |c| (Cauchy-Schwarz); each arm is within (dp + LQ + 1) 2^-23 A of the exact score
                A = q.float().norm(dim=-1).sum(1) * float(index.tok.float().norm(dim=-1).max())
                tol = 2 * (dp + LQ + 1) * 2.0 ** -23 * A
                diff = (fv - mv).abs()
                same = fi == mi
                check = dict(max_score_diff=float(diff.max()), tol_min=float(tol.min()), ids_equal=float(same.float().mean()),
                             scores_within_bound=bool((diff <= tol[:, None]).all()))
                assert check["scores_within_bound"], check  # (ids may differ only where two scores are closer than the bound)
            times, peak = {n: [] for n in arms}, {}
            for n, fn in arms.items():
                for _ in range(a.warmup):
                    fn()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                fn()
                torch.cuda.synchronize()
                peak[n] = torch.cuda.max_memory_allocated() - base
            for _ in range(max(a.steps, 10)):
                for n, fn in arms.items():  # arms alternate
                    times[n].append(timed(fn)[0])
            sm = med(score_ms)
            flops = 2.0 * nq * LQ * T * dp / (sm * 1e-3)
            bps = index.tok.numel() * 2 / (sm * 1e-3)
            out = dict(bench="colbert_search", shape=sh["name"], docs=sh["docs"], tokens=T, mean_len=round(T / sh["docs"], 1), n_blk=index.n_blk,
                       nq=nq, LQ=LQ, d=sh["d"], topk=k, chunk=chunk, index_bytes=index.nbytes,
                       padded_bytes=None if Cpad is None else Cpad.numel() * 2, score_ms=sm, score_ms_min=round(min(score_ms), 3),
                       score_tflops=round(flops / 1e12, 1), mfma_peak_share=round(flops / PEAK_BF16_FLOPS, 4),
                       token_gbps=round(bps / 1e9, 1), hbm_peak_share=round(bps / PEAK_HBM_BPS, 4))
            out["bound"] = "mfma" if out["mfma_peak_share"] >= out["hbm_peak_share"] else "hbm"
            for n in arms:
                out[f"{n}_ms"], out[f"{n}_ms_min"], out[f"{n}_ms_max"] = med(times[n]), round(min(times[n]), 3), round(max(times[n]), 3)
                out[f"{n}_peak_bytes"] = int(peak[n])
            if check is not None:
                out["check"] = check
                out["speedup_vs_maxsim"] = round(out["maxsim_ms"] / out["fused_ms"], 2)
                out["fused_median_below_maxsim_min"] = bool(out["fused_ms"] < min(out["maxsim_ms_min"], out["maxsim_again_ms_min"]))
                out["fused_max_below_maxsim_min"] = bool(out["fused_ms_max"] < min(out["maxsim_ms_min"], out["maxsim_again_ms_min"]))
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
