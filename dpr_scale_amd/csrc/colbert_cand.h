// colbert_cand.h -- MaxSim over candidate lists: the score of colbert.h for a different, ragged list of passages
// per query instead of a doc-id range shared by all queries.  One window S[nq, cols] of candidate POSITIONS:
//
//   S[n][j] = score(n, cand_doc[cand_off[n] + pos_begin + j])   where the position is below the query's count and the doc id lies in
//                                                               [0, corpus_len);  a quiet NaN ("no candidate") everywhere else
//
// Equal, bit for bit, to the cell cb_score_kernel writes for the same query rows and passage rows: the token block is the A operand of
// v_mfma_f32_16x16x32_bf16 and 16 query tokens are B, the k-steps run in ascending order from a zero accumulator, the maxima over a
// block, over a passage's blocks (ascending) and across the lane >> 4 groups are fmaxf from a start of 0, and ONE owner thread per cell
// pools the LQ terms in ascending token order.  No floating-point atomics; a cell depends on its query's and its passage's rows only --
// not on the window, the rest of the list or the other queries.
//
// Plan    grid (runs of CBC_RUNP positions of the window) x (query).  The four waves take the run's passages one at a time from an LDS
//         counter (a 180-token passage next to 20-token ones does not hold three waves up), one pass per CBC_QW query fragments: the
//         fragments of the pass stay in registers (dp <= 128; a wider dp reads them through the cache every block) and the passage's
//         token blocks go straight from global memory into the A registers, the next block's loads issued before this block's MFMAs.
//         There is no reuse across waves, so nothing is staged through LDS.  The clamped maxima go to an LDS table T[position][query
//         token]; after the run one thread per cell pools and stores.
// Bounds  a query's pair of cand_off is clamped to [0, n_cand], an end below its begin counts as the begin (an empty list); a doc id
//         outside [0, corpus_len) is never used as an index; block offsets are clamped to [0, n_blk] and an end below its begin counts
//         as the begin.  Nothing behind tok[n_blk * 16 * dp - 1], cand_doc[n_cand - 1] or dblk[corpus_len] is read whatever the lists
//         hold.  S is written at [n < nq][j < cols] only, every such cell.
#pragma once

#include "colbert.h"

namespace dprhot {

constexpr int CBC_RUNP = 32;      // candidate positions per workgroup
constexpr int CBC_QW = 4;         // query fragments per pass
constexpr int CBC_PASSES = CB_FMAX / CBC_QW;

struct CbcArgs {
  const uint16_t* tok;        // bf16 [n_blk * 16, dp]
  const long long* dblk;      // [corpus_len + 1]
  long long n_blk, corpus_len;
  int dp;
  const uint16_t* q;          // bf16 [nq, LQ, dp]
  int nq, LQ, pool;           // pool: 0 sum, 1 max
  const long long* cand_off;  // [nq + 1]
  const int* cand_doc;        // [n_cand]
  long long n_cand;
  long long pos_begin;        // first candidate position of the window
  int cols;                   // positions in the window
  float* S;                   // [nq, ld]
  long long ld;
  int FQ;                     // fragments per query
};

// the entries [lo, hi) of cand_doc that query n owns
__device__ __forceinline__ void cbc_range(const long long* cand_off, long long n_cand, int n, long long& lo, long long& hi) {
  const long long a = cand_off[n], b = cand_off[n + 1];
  lo = a < 0 ? 0 : a > n_cand ? n_cand : a;
  hi = b < 0 ? 0 : b > n_cand ? n_cand : b;
  if (hi < lo) hi = lo;
}

// KS = dp / 32 for dp <= 128 (query fragments in registers); KS = 0: any dp, query fragments read per block
template <int KS>
__global__ __launch_bounds__(256) void cbc_score_kernel(CbcArgs p) {
  extern __shared__ __align__(16) unsigned char cbc_table[];  // T [CBC_RUNP][tstride]
  __shared__ long long sb0[CBC_RUNP], sb1[CBC_RUNP];
  __shared__ int sok[CBC_RUNP];
  __shared__ int next[CBC_PASSES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int n = (int)blockIdx.y;
  const int pl0 = (int)blockIdx.x * CBC_RUNP;
  const int np = p.cols - pl0 < CBC_RUNP ? p.cols - pl0 : CBC_RUNP;
  const int ksteps = KS ? KS : p.dp / 32;
  const int tstride = p.FQ * 16 + 1;  // floats per position (+ 1: the owners' reads spread over the banks)
  float* T = reinterpret_cast<float*>(cbc_table);

  if (tid < np) {
    long long lo, hi;
    cbc_range(p.cand_off, p.n_cand, n, lo, hi);
    const long long pos = p.pos_begin + pl0 + tid;
    int ok = 0;
    long long b0 = 0, b1 = 0;
    if (pos < hi - lo) {
      const long long doc = p.cand_doc[lo + pos];
      if (doc >= 0 && doc < p.corpus_len) {
        ok = 1;
        b0 = p.dblk[doc];
        b1 = p.dblk[doc + 1];
        b0 = b0 < 0 ? 0 : b0 > p.n_blk ? p.n_blk : b0;
        b1 = b1 < 0 ? 0 : b1 > p.n_blk ? p.n_blk : b1;
        if (b1 < b0) b1 = b0;
      }
    }
    sok[tid] = ok;
    sb0[tid] = b0;
    sb1[tid] = b1;
  }
  if (tid < CBC_PASSES) next[tid] = 0;
  __syncthreads();

  for (int f0 = 0, pass = 0; f0 < p.FQ; f0 += CBC_QW, ++pass) {
    const int nfr = p.FQ - f0 < CBC_QW ? p.FQ - f0 : CBC_QW;  // this pass's fragments are slots i < nfr
    bool bok[CBC_QW];
    const uint16_t* qp[CBC_QW];
    cb_bf16x8 bq[CBC_QW][KS ? KS : 1];
#pragma unroll
    for (int i = 0; i < CBC_QW; ++i) {
      const int t = (f0 + i) * 16 + i16;
      bok[i] = i < nfr && t < p.LQ;
      qp[i] = p.q + ((long long)n * p.LQ + (bok[i] ? t : 0)) * p.dp + g4 * 8;
      if constexpr (KS > 0) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bq[i][ks] = cb_load8(qp[i] + ks * 32, bok[i]);
      }
    }
    for (;;) {
      int pl = 0;
      if (lane == 0) pl = atomicAdd(&next[pass], 1);
      pl = __builtin_amdgcn_readfirstlane(pl);
      if (pl >= np) break;
      if (!sok[pl]) continue;
      const long long b0 = sb0[pl], b1 = sb1[pl];
      float m[CBC_QW];
#pragma unroll
      for (int i = 0; i < CBC_QW; ++i) m[i] = 0.f;  // the clamp
      const uint16_t* arow = p.tok + (b0 * 16 + i16) * p.dp + g4 * 8;  // lane's row of the block, its 8 features of k-step 0
      const long long bstride = 16ll * p.dp;
      if constexpr (KS > 0) {
        cb_bf16x8 a[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = cb_load8(arow + ks * 32, b0 < b1);
        for (long long b = b0; b < b1; ++b) {
          cb_bf16x8 an[KS];
          const bool more = b + 1 < b1;
          arow += bstride;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) an[ks] = cb_load8(arow + ks * 32, more);  // the next block is in flight under the MFMAs
          cb_f32x4 acc[CBC_QW];
#pragma unroll
          for (int i = 0; i < CBC_QW; ++i) acc[i] = cb_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int i = 0; i < CBC_QW; ++i)
            if (i < nfr) {
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], bq[i][ks], acc[i], 0, 0, 0);
            }
          // lane holds tokens g4 * 4 + r of this block against query token i16 of fragment f0 + i
#pragma unroll
          for (int i = 0; i < CBC_QW; ++i) m[i] = fmaxf(m[i], fmaxf(fmaxf(acc[i][0], acc[i][1]), fmaxf(acc[i][2], acc[i][3])));
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) a[ks] = an[ks];
        }
      } else {
        for (long long b = b0; b < b1; ++b, arow += bstride) {
          cb_f32x4 acc[CBC_QW];
#pragma unroll
          for (int i = 0; i < CBC_QW; ++i) acc[i] = cb_f32x4{0.f, 0.f, 0.f, 0.f};
          for (int ks = 0; ks < ksteps; ++ks) {
            const cb_bf16x8 a = *reinterpret_cast<const cb_bf16x8*>(arow + ks * 32);
#pragma unroll
            for (int i = 0; i < CBC_QW; ++i)
              if (i < nfr) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, cb_load8(qp[i] + ks * 32, bok[i]), acc[i], 0, 0, 0);
          }
#pragma unroll
          for (int i = 0; i < CBC_QW; ++i) m[i] = fmaxf(m[i], fmaxf(fmaxf(acc[i][0], acc[i][1]), fmaxf(acc[i][2], acc[i][3])));
        }
      }
      // the passage's maxima are complete: one term per query token into the table
#pragma unroll
      for (int i = 0; i < CBC_QW; ++i) {
        if (i < nfr) {
          float v = m[i];
          v = fmaxf(v, __shfl_xor(v, 16, 64));
          v = fmaxf(v, __shfl_xor(v, 32, 64));
          if (lane < 16) T[pl * tstride + (f0 + i) * 16 + lane] = v;
        }
      }
    }
  }
  __syncthreads();
  // one owner per cell: the query's LQ terms in ascending token order; a position without a candidate is a quiet NaN
  if (tid < np) {
    float acc = __builtin_nanf("");
    if (sok[tid]) {
      const float* tt = T + tid * tstride;
      acc = tt[0];
      for (int i = 1; i < p.LQ; ++i) acc = p.pool ? fmaxf(acc, tt[i]) : acc + tt[i];
    }
    p.S[(long long)n * p.ld + pl0 + tid] = acc;
  }
}

// the selected POSITIONS of row n become doc ids: indices[n][j] = cand_doc[cand_off[n] + indices[n][j]]; -1 stays -1
__global__ __launch_bounds__(256) void cbc_map_kernel(const long long* cand_off, const int* cand_doc, long long n_cand, int nq, int k,
                                                      long long* indices) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)nq * k) return;
  const long long pos = indices[t];
  if (pos < 0) return;
  long long lo, hi;
  cbc_range(cand_off, n_cand, (int)(t / k), lo, hi);
  indices[t] = pos < hi - lo ? (long long)cand_doc[lo + pos] : -1;
}

}  // namespace dprhot
