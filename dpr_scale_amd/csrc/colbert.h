// colbert.h -- exhaustive MaxSim search of ColBERT: one chunk S[nq, cols] of
//
//   score(n, doc) = POOL over query tokens i < LQ of  max(0, max over stored tokens j of doc of <q[n, i], c[doc, j]>)
//
// The token-level products never leave the registers; nothing is kept for a backward.
//
// Index   tok bf16 [n_blk * 16, dp] (dp = d padded with zeros to a multiple of 32), token blocks of 16 rows; dblk int64 [corpus_len + 1]
//         block offsets, passage doc owns blocks dblk[doc] .. dblk[doc + 1]; the rows behind a passage's last token are zero.  A zero row
//         gives products of exactly 0, which the clamp at 0 makes neutral: every 16-row MFMA fragment belongs to ONE passage and no
//         segmented max inside a fragment exists.
// Queries q bf16 [nq, LQ, dp], padded query tokens are zero rows (they add 0).  A query is cut into FQ = ceil(LQ / 16) fragments of 16
//         tokens; the rows behind LQ are loaded as zeros.
//
// Plan    grid (runs of CB_RUNP consecutive passages of the chunk) x (groups of QPW whole queries).  A workgroup stages the token blocks
//         of its run through LDS in tiles (rows padded by 16 bytes: the 16 rows of a fragment read land on distinct banks) for its
//         four waves.  The token block is the A operand of v_mfma_f32_16x16x32_bf16, 16 query tokens are B: a lane holds four tokens of
//         one query token's column, so the running max over a passage is four fmax per block in registers and the cross-lane part
//         (two steps over the lane >> 4 groups) is paid once per passage.  The waves split the group's query fragments round robin,
//         CB_QW per wave and pass, and keep them in registers (dp <= 128; a wider dp reads them through the cache every block); a
//         fragment slot without a fragment is skipped.  A query longer than 16 * 4 * CB_QW tokens takes several passes over the run.
// Owner   wave: when a passage ends, the clamped maximum of every query token goes to an LDS table T[passage][query token].  After the
//         run ONE thread per cell (n, doc) pools the query's LQ terms in ascending token order (sum or max) and writes S.  No floating-
//         point atomics; a cell depends on its query's and its passage's rows only -- not on the chunk, the id range, the other queries
//         of the batch or the other passages of the index.
// NaN     fmax drops a NaN operand: a NaN product takes no part, as if its token were absent.
// Bounds  block offsets are clamped to [0, n_blk] and made non-decreasing before use: no row behind n_blk * 16 - 1 is read whatever
//         dblk holds; S is written at [n < nq][doc - D0 < cols] only, every such cell.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dprhot {

constexpr int CB_RUNP = 16;            // passages per workgroup
constexpr int CB_QW = 4;               // query fragments per wave and pass
constexpr int CB_FPP = 4 * CB_QW;      // query fragments per workgroup and pass
constexpr int CB_FMAX = 32;            // fragments of the longest query (DPRHOT_MAXSIM_MAX_LEN / 16)
constexpr int CB_TILE_BYTES = 24832;   // LDS budget of one token tile: 5 blocks at dp = 128, one at dp = 768 (rows padded by 16 bytes)
constexpr int CB_MAX_DP = 768;         // one block of the widest row still fits the tile

struct CbArgs {
  const uint16_t* tok;     // bf16 [n_blk * 16, dp]
  const long long* dblk;   // [corpus_len + 1]
  long long n_blk;
  int dp;
  const uint16_t* q;       // bf16 [nq, LQ, dp]
  int nq, LQ, pool;        // pool: 0 sum, 1 max
  long long D0;            // first doc id of the chunk
  int cols;                // doc ids in the chunk
  float* S;                // [nq, ld]
  long long ld;
  int FQ, QPW, TB;         // fragments per query, queries per workgroup, token blocks per tile
};

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short cb_bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float cb_f32x4;

__device__ __forceinline__ cb_bf16x8 cb_load8(const uint16_t* p, bool ok) {
  cb_bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? *reinterpret_cast<const cb_bf16x8*>(p) : z;
}

// KS = dp / 32 for dp <= 128 (query fragments in registers); KS = 0: any dp, query fragments read per block
template <int KS>
__global__ __launch_bounds__(256) void cb_score_kernel(CbArgs p) {
  extern __shared__ __align__(16) unsigned char cb_tile[];
  __shared__ long long off[CB_RUNP + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int pl0 = (int)blockIdx.x * CB_RUNP;
  const int np = p.cols - pl0 < CB_RUNP ? p.cols - pl0 : CB_RUNP;
  const int q0 = (int)blockIdx.y * p.QPW;
  const int nql = p.nq - q0 < p.QPW ? p.nq - q0 : p.QPW;
  const int F = nql * p.FQ;  // (<= CB_FMAX: the launcher's choice of QPW)
  const int ksteps = KS ? KS : p.dp / 32;
  const int cpr = ksteps * 4;           // 16-byte pieces per token row
  const int rowb = p.dp * 2 + 16;       // LDS row stride in bytes
  const int tstride = p.QPW * p.FQ * 16 + 1;  // floats per passage of the term table (+ 1: the owners' reads spread over the banks)
  float* T = reinterpret_cast<float*>(cb_tile + p.TB * 16 * rowb);  // [CB_RUNP][tstride] behind the tile

  if (tid <= np) {
    long long v = p.dblk[p.D0 + pl0 + tid];
    off[tid] = v < 0 ? 0 : v > p.n_blk ? p.n_blk : v;
  }
  __syncthreads();
  if (tid == 0)
    for (int i = 1; i <= np; ++i)
      if (off[i] < off[i - 1]) off[i] = off[i - 1];
  __syncthreads();
  const long long b0 = off[0], b1 = off[np];

  for (int f0 = 0; f0 < F; f0 += CB_FPP) {
    int fr[CB_QW];
    bool bok[CB_QW];
    const uint16_t* qp[CB_QW];
    cb_bf16x8 bq[CB_QW][KS ? KS : 1];
    float m[CB_QW];
    const int nfr = F - f0 - wave > 0 ? (F - f0 - wave + 3) / 4 : 0;  // this wave's fragments are slots i < nfr (wave-uniform)
#pragma unroll
    for (int i = 0; i < CB_QW; ++i) {
      fr[i] = f0 + i * 4 + wave;
      const bool fok = fr[i] < F;
      const int ql = fok ? fr[i] / p.FQ : 0;
      const int t = (fok ? fr[i] - ql * p.FQ : 0) * 16 + i16;
      bok[i] = fok && t < p.LQ;
      qp[i] = p.q + ((long long)(q0 + ql) * p.LQ + (bok[i] ? t : 0)) * p.dp + g4 * 8;
      m[i] = 0.f;
      if constexpr (KS > 0) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bq[i][ks] = cb_load8(qp[i] + ks * 32, bok[i]);
      }
    }
    // the maxima of passage pl are complete (m starts at 0: the clamp): one term per query token into the table
    auto finish = [&](int pl) {
#pragma unroll
      for (int i = 0; i < CB_QW; ++i) {
        if (i < nfr) {
          float v = m[i];
          v = fmaxf(v, __shfl_xor(v, 16, 64));
          v = fmaxf(v, __shfl_xor(v, 32, 64));
          if (lane < 16) T[pl * tstride + fr[i] * 16 + lane] = v;
          m[i] = 0.f;
        }
      }
    };
    int pl = 0;
    long long nxt = off[1];
    for (long long t0 = b0; t0 < b1; t0 += p.TB) {
      const int nb = (int)(b1 - t0 < p.TB ? b1 - t0 : p.TB);
      __syncthreads();  // the previous tile has been read by every wave
      {
        const uint16_t* src = p.tok + t0 * 16 * p.dp;
        const int total = nb * 16 * cpr;
        for (int c = tid; c < total; c += 256) {
          const int r = c / cpr, k = c - r * cpr;
          *reinterpret_cast<cb_bf16x8*>(cb_tile + r * rowb + k * 16) = *reinterpret_cast<const cb_bf16x8*>(src + (long long)c * 8);
        }
      }
      __syncthreads();
      for (int bl = 0; bl < nb; ++bl) {
        while (t0 + bl >= nxt) {  // (t0 + bl < off[np]: pl + 1 <= np here)
          finish(pl);
          ++pl;
          nxt = off[pl + 1];
        }
        const unsigned char* arow = cb_tile + (bl * 16 + i16) * rowb + g4 * 16;
        cb_f32x4 acc[CB_QW];
#pragma unroll
        for (int i = 0; i < CB_QW; ++i) acc[i] = cb_f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (KS > 0) {
          cb_bf16x8 a[KS];
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) a[ks] = *reinterpret_cast<const cb_bf16x8*>(arow + ks * 64);
#pragma unroll
          for (int i = 0; i < CB_QW; ++i)
            if (i < nfr) {
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], bq[i][ks], acc[i], 0, 0, 0);
            }
        } else {
          for (int ks = 0; ks < ksteps; ++ks) {
            const cb_bf16x8 a = *reinterpret_cast<const cb_bf16x8*>(arow + ks * 64);
#pragma unroll
            for (int i = 0; i < CB_QW; ++i)
              if (i < nfr) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, cb_load8(qp[i] + ks * 32, bok[i]), acc[i], 0, 0, 0);
          }
        }
        // lane holds tokens g4 * 4 + r of this block against query token i16 of fragment fr[i]
#pragma unroll
        for (int i = 0; i < CB_QW; ++i) m[i] = fmaxf(m[i], fmaxf(fmaxf(acc[i][0], acc[i][1]), fmaxf(acc[i][2], acc[i][3])));
      }
    }
    while (pl < np) {
      finish(pl);
      ++pl;
    }
  }
  __syncthreads();
  // one owner per cell: the query's LQ terms in ascending token order
  for (int t = tid; t < np * nql; t += 256) {
    const int ql = t / np, pl = t - ql * np;
    const float* tt = T + pl * tstride + ql * p.FQ * 16;
    float acc = tt[0];
    for (int i = 1; i < p.LQ; ++i) acc = p.pool ? fmaxf(acc, tt[i]) : acc + tt[i];
    p.S[(long long)(q0 + ql) * p.ld + pl0 + pl] = acc;
  }
}

}  // namespace dprhot
