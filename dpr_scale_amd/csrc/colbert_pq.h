// colbert_pq.h -- the exhaustive MaxSim search of csrc/colbert.h over a product-quantised token index.
//
// Index   the block layout of colbert.h (16 rows per block, dblk int64 [corpus_len + 1]), but a token row is code uint8 [n_blk * 16, m]
//         -- one 8-bit code per subspace of DSUB features, m = dp / DSUB -- under ONE codebook cb bf16 [m, 256, DSUB] (the layout and the
//         decode rule of csrc/ivf_pq.h), and rows uint8 [n_blk] holds the number of real token rows of every block.  The index that is
//         searched is, by definition,
//             tok[r, j * DSUB + t] = (r mod 16) < rows[r / 16] ? cb[j, code[r, j], t] : 0
//         A row at or behind rows[] is an exact zero whatever its code bytes hold (a centroid is not zero, and the clamp at 0 needs the
//         padding rows neutral); a rows[] value above 16 counts as 16.
// Score   cbpq_score_kernel is cb_score_kernel's plan (token block = A, 16 query tokens = B, running max in registers, two cross-lane
//         steps per passage, LDS term table, one owner per cell, terms pooled in token order) with ONE change: the A fragment is
//         assembled from code bytes and codebook rows at the operand read.  Lane (i16, g4) at K step ks holds features 32 ks + 8 g4 .. + 7
//         of token row i16 = 8 / DSUB whole sub-vectors: one 1-, 2- or 4-byte read of the code tile and as many DSUB-wide codebook reads
//         (16, 8 or 4 bytes), both from LDS.  The MFMA operands are bit for bit those of cb_score_kernel over the decoded index, in the
//         same K order, and so is every score.
// Plan    workgroups of CBPQ_WAVES = 8 waves: the codebook (dp * 512 bytes, 64 KiB at dp = 128) allows one workgroup per CU, so the
//         workgroup brings the waves.  A workgroup loads the codebook ONCE (the barrier behind that load is passed by every wave; the
//         kernel has no early return), keeps its CBPQ_FPP = 32 query fragments in registers (<= CB_FMAX: a single pass over the tokens
//         whatever LQ is; with fewer than 8 fragments -- one short query -- 8 / F waves share a fragment and take the passages in turn)
//         and walks RPW consecutive runs of CB_RUNP passages.  The LDS tile holds CODES -- a linear copy of the blocks'
//         bytes, 16 * m per block, and their rows[] values -- so a tile spans 16 (m = 64) to 256 (m = 4) blocks between two barriers.
// LDS     dynamic: codebook | code tile (CBPQ_TILE_BYTES) | rows of the tile (CBPQ_TILE_BLOCKS) | term table [CB_RUNP][tstride].
// NaN     as colbert.h: fmax drops a NaN product.  Bounds: block offsets clamped to [0, n_blk] and made non-decreasing; no byte behind
//         code[n_blk * 16 * m - 1] or rows[n_blk - 1] is read; S is written at [n < nq][doc - D0 < cols] only, every such cell.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "colbert.h"
#include "ivf_pq.h"

namespace dprhot {

constexpr int CBPQ_WAVES = 8;                   // waves per workgroup
constexpr int CBPQ_THREADS = 64 * CBPQ_WAVES;
constexpr int CBPQ_FPP = CBPQ_WAVES * CB_QW;    // query fragments per workgroup (= CB_FMAX: one pass)
constexpr int CBPQ_TILE_BYTES = 16384;          // code bytes per tile
constexpr int CBPQ_TILE_BLOCKS = 256;           // most blocks of one tile (m = 4 fills the tile with 256)
constexpr int CBPQ_MAX_DP = 128;                // query fragments in registers, the codebook in LDS
constexpr int CBPQ_MAX_RPW = 8;                 // most runs per workgroup

static_assert(CBPQ_FPP >= CB_FMAX, "one pass over the tokens covers the longest query");

struct CbPqArgs {
  const uint8_t* code;     // uint8 [n_blk * 16, dp / DSUB]
  const uint8_t* rows;     // uint8 [n_blk]
  const uint16_t* cb;      // bf16 [dp / DSUB, 256, DSUB]
  const long long* dblk;   // [corpus_len + 1]
  long long n_blk;
  const uint16_t* q;       // bf16 [nq, LQ, dp]
  int nq, LQ, pool;        // pool: 0 sum, 1 max
  long long D0;            // first doc id of the chunk
  int cols;                // doc ids in the chunk
  float* S;                // [nq, ld]
  long long ld;
  int FQ, QPW, TB, RPW;    // fragments per query, queries per workgroup, token blocks per tile, runs per workgroup
};

// KS = dp / 32 (1 .. 4)
template <int DSUB, int KS>
__global__ __launch_bounds__(CBPQ_THREADS) void cbpq_score_kernel(CbPqArgs p) {
  constexpr int DP = KS * 32;
  constexpr int MSUB = DP / DSUB;        // code bytes per token row
  constexpr int BLKB = 16 * MSUB;        // code bytes per block
  extern __shared__ __align__(16) unsigned char cbpq_lds[];
  __shared__ long long off[CB_RUNP + 1];
  uint16_t* CBK = reinterpret_cast<uint16_t*>(cbpq_lds);              // [MSUB][256][DSUB]
  unsigned char* tile = cbpq_lds + DP * 512;                          // [TB][16][MSUB]
  unsigned char* trow = tile + CBPQ_TILE_BYTES;                       // [TB]
  const int tstride = p.QPW * p.FQ * 16 + 1;                          // floats per passage of the term table (colbert.h)
  float* T = reinterpret_cast<float*>(trow + CBPQ_TILE_BLOCKS);       // [CB_RUNP][tstride]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;

  // every wave takes part in the codebook load; the first barrier of the run loop stands behind it
  for (int i = tid; i < DP * 32; i += CBPQ_THREADS)
    reinterpret_cast<ivf_i32x4*>(CBK)[i] = reinterpret_cast<const ivf_i32x4*>(p.cb)[i];

  const int q0 = (int)blockIdx.y * p.QPW;
  const int nql = p.nq - q0 < p.QPW ? p.nq - q0 : p.QPW;
  const int F = nql * p.FQ;  // (<= CBPQ_FPP: the launcher's choice of QPW)
  // F >= 8: wave w owns fragments w, w + 8, ... of every passage.  F < 8 (a single short query): 8 / F waves share a fragment and take
  // the run's passages in turn (passage pl belongs to group pl & (wpf - 1)), so that no wave idles; a cell of T still has ONE writer.
  const bool few = F < CBPQ_WAVES;
  const int wpf = few ? CBPQ_WAVES / F : 1, grp = few ? wave / F : 0, slot0 = few ? wave - grp * F : wave;
  const int wmask = wpf - 1;  // (8 / F is 8, 4, 2, 2, 1, 1 or 1: a power of two)
  const int nfr = few ? (grp < wpf ? 1 : 0) : (F - wave + CBPQ_WAVES - 1) / CBPQ_WAVES;  // this wave's fragments are slots i < nfr
  int fr[CB_QW];
  cb_bf16x8 bq[CB_QW][KS];
  float m[CB_QW];
#pragma unroll
  for (int i = 0; i < CB_QW; ++i) {
    fr[i] = i * CBPQ_WAVES + slot0;
    const bool fok = fr[i] < F;
    const int ql = fok ? fr[i] / p.FQ : 0;
    const int t = (fok ? fr[i] - ql * p.FQ : 0) * 16 + i16;
    const bool bok = fok && t < p.LQ;
    const uint16_t* qp = p.q + ((long long)(q0 + ql) * p.LQ + (bok ? t : 0)) * DP + g4 * 8;
    m[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bq[i][ks] = cb_load8(qp + ks * 32, bok);
  }

  const int nruns = (p.cols + CB_RUNP - 1) / CB_RUNP;
  const int run0 = (int)blockIdx.x * p.RPW;
  const int run1 = run0 + p.RPW < nruns ? run0 + p.RPW : nruns;
  for (int run = run0; run < run1; ++run) {
    const int pl0 = run * CB_RUNP;
    const int np = p.cols - pl0 < CB_RUNP ? p.cols - pl0 : CB_RUNP;
    if (tid <= np) {
      long long v = p.dblk[p.D0 + pl0 + tid];
      off[tid] = v < 0 ? 0 : v > p.n_blk ? p.n_blk : v;
    }
    __syncthreads();  // (also: the codebook is in LDS; the owners of the previous run are done with T)
    if (tid == 0)
      for (int i = 1; i <= np; ++i)
        if (off[i] < off[i - 1]) off[i] = off[i - 1];
    __syncthreads();
    const long long b0 = off[0], b1 = off[np];

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
    // the walk over the run's tiles; FEW: this wave takes the passages of its group only (compiled apart: the common walk stays free
    // of the ownership test)
    auto walk = [&](auto few_c) {
      constexpr bool FEW = decltype(few_c)::value;
      int pl = 0;
      long long nxt = off[1];
      for (long long t0 = b0; t0 < b1; t0 += p.TB) {
        const int nb = (int)(b1 - t0 < p.TB ? b1 - t0 : p.TB);
        __syncthreads();  // the previous tile has been read by every wave
        {
          const ivf_i32x4* src = reinterpret_cast<const ivf_i32x4*>(p.code + t0 * BLKB);
          const int total = nb * (BLKB / 16);  // 16-byte pieces (nb * BLKB <= CBPQ_TILE_BYTES: the launcher's choice of TB)
          for (int c = tid; c < total; c += CBPQ_THREADS) reinterpret_cast<ivf_i32x4*>(tile)[c] = src[c];
          for (int c = tid; c < nb; c += CBPQ_THREADS) trow[c] = p.rows[t0 + c];
        }
        __syncthreads();
        if (nfr > 0) {
          for (int bl = 0; bl < nb; ++bl) {
            while (t0 + bl >= nxt) {  // (t0 + bl < off[np]: pl + 1 <= np here)
              if (!FEW || (pl & wmask) == grp) finish(pl);
              ++pl;
              nxt = off[pl + 1];
            }
            if constexpr (FEW) {
              if ((pl & wmask) != grp) {  // another group's passage: on to the first block behind it (nxt > t0 + bl)
                bl = (int)(nxt - t0 < nb ? nxt - t0 : nb) - 1;
                continue;
              }
            }
            const bool rok = i16 < (int)trow[bl];
            const uint8_t* crow = tile + (bl * 16 + i16) * MSUB;
            cb_bf16x8 a[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) a[ks] = ivf_pq_frag<DSUB>(crow, CBK, (ks * 32 + g4 * 8) / DSUB, rok);
            cb_f32x4 acc[CB_QW];
#pragma unroll
            for (int i = 0; i < CB_QW; ++i) {
              acc[i] = cb_f32x4{0.f, 0.f, 0.f, 0.f};
              if (i < nfr) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], bq[i][ks], acc[i], 0, 0, 0);
              }
            }
            // lane holds tokens g4 * 4 + r of this block against query token i16 of fragment fr[i]
#pragma unroll
            for (int i = 0; i < CB_QW; ++i) m[i] = fmaxf(m[i], fmaxf(fmaxf(acc[i][0], acc[i][1]), fmaxf(acc[i][2], acc[i][3])));
          }
        }
      }
      while (pl < np) {
        if (!FEW || (pl & wmask) == grp) finish(pl);
        ++pl;
      }
    };
    if (few)  // (uniform over the workgroup: every wave meets the same barriers)
      walk(std::true_type{});
    else
      walk(std::false_type{});
    __syncthreads();
    // one owner per cell: the query's LQ terms in ascending token order
    for (int t = tid; t < np * nql; t += CBPQ_THREADS) {
      const int ql = t / np, pc = t - ql * np;
      const float* tt = T + pc * tstride + ql * p.FQ * 16;
      float acc = tt[0];
      for (int i = 1; i < p.LQ; ++i) acc = p.pool ? fmaxf(acc, tt[i]) : acc + tt[i];
      p.S[(long long)(q0 + ql) * p.ld + pl0 + pc] = acc;
    }
  }
}

}  // namespace dprhot
