// colbert_cen.h -- the centroid-interaction stage of the pruned ColBERT search: every candidate of
// colbert_cand.h scored approximately, each passage token replaced by its centroid, so that exact MaxSim runs on the best `ndocs` only.
//
//   T[n][c][i]     = <q[n, i], centroid_c>   fp32 [nq, C, LT], LT = 16 * ceil(LQ / 16), columns LQ .. LT are 0           (cbi_table_kernel)
//   approx(n, doc) = POOL over query tokens i < LQ of  max(0, max over c in doc's centroid list of T[n][c][i])           (cbi_score_kernel)
//
// A passage's list is the sorted, duplicate-free centroid ids of its stored tokens: doc_cen[doc_cen_off[doc] .. doc_cen_off[doc + 1]].
// A product of the table is computed as cb_score_kernel computes a token's -- the centroid block is the A operand of
// v_mfma_f32_16x16x32_bf16, 16 query tokens are B, the k-steps run in ascending order from a zero accumulator -- every maximum is an
// fmaxf from a start of 0 and ONE owner per cell pools the LQ terms in ascending token order.  So approx(n, doc) is, bit for bit, the cell
// cb_score_kernel writes for an index with the same block layout whose token rows are centroids[tok_centroid] (zero rows on padding):
// duplicates and zero rows do not change a maximum that starts at 0.  No floating-point atomics.
//
// Plan    table: grid (groups of four blocks of 16 centroids) x (query); a wave keeps its centroid block in the A registers (dp <= 128; a
//         wider dp reads it through the cache every fragment) and walks the query's fragments: one 16 x 16 store per fragment, 64
//         contiguous bytes per centroid row.
//         score: the grid of cbc_score_kernel, (runs of CBC_RUNP positions of the window) x (query), x fastest: one query's workgroups
//         are co-resident and its table (C * LT * 4 bytes) is served from each XCD's L2.  The four waves take the run's passages one at
//         a time from an LDS counter.  A wave reads 64 centroid ids of the passage in one coalesced load; a table row is cut into
//         16-byte pieces, lane = (row slot, piece), and CBI_FLY rows per lane are in flight before the first fmaxf.  The maxima over the
//         row slots are folded across the lanes once per passage and go to the LDS term table T[position][query token]; after the run
//         one thread per cell pools and stores.  A row longer than 64 pieces (LQ > 256) takes several passes over the passage's ids.
// Bounds  the candidate window is colbert_cand.h's, word for word: a pair of cand_off is clamped to [0, n_cand], a doc id outside
//         [0, corpus_len) is never used as an index and gives a quiet NaN.  A pair of doc_cen_off is clamped to [0, n_pairs], an end
//         below its begin counts as the begin; a centroid id outside [0, C) is skipped and never used as an index; an empty list scores
//         0.  Nothing behind doc_cen[n_pairs - 1], doc_cen_off[corpus_len] or T[nq * C * LT - 1] is read whatever the lists hold.  S is
//         written at [n < nq][j < cols] only, every such cell; the table kernel writes every cell of T and nothing else.
#pragma once

#include "colbert_cand.h"

namespace dprhot {

constexpr int CBI_FLY = 4;  // table rows a lane has in flight before the first fmaxf

struct CbiTableArgs {
  const uint16_t* cen;  // bf16 [C, dp]
  int C, dp;
  const uint16_t* q;    // bf16 [nq, LQ, dp]
  int nq, LQ, FQ;       // FQ: fragments per query, LT = FQ * 16
  float* T;             // [nq, C, FQ * 16]
};

// KS = dp / 32 for dp <= 128 (the centroid block in registers); KS = 0: any dp, the block read per fragment
template <int KS>
__global__ __launch_bounds__(256) void cbi_table_kernel(CbiTableArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int n = (int)blockIdx.y;
  const long long c0 = ((long long)blockIdx.x * 4 + wave) * 16;  // the wave's block of 16 centroids
  if (c0 >= p.C) return;
  const int ksteps = KS ? KS : p.dp / 32;
  const int LT = p.FQ * 16;
  const bool aok = c0 + i16 < p.C;  // a row behind the last centroid is loaded as zeros and never stored
  const uint16_t* arow = p.cen + (aok ? c0 + i16 : 0) * p.dp + g4 * 8;
  cb_bf16x8 a[KS ? KS : 1];
  if constexpr (KS > 0) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a[ks] = cb_load8(arow + ks * 32, aok);
  }
  float* out = p.T + ((long long)n * p.C + c0 + g4 * 4) * LT + i16;  // lane holds centroids c0 + g4 * 4 + r against query token i16
  for (int f = 0; f < p.FQ; ++f) {
    const int t = f * 16 + i16;
    const bool bok = t < p.LQ;  // a token behind LQ is a zero row: its column is written as 0
    const uint16_t* qp = p.q + ((long long)n * p.LQ + (bok ? t : 0)) * p.dp + g4 * 8;
    cb_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if constexpr (KS > 0) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], cb_load8(qp + ks * 32, bok), acc, 0, 0, 0);
    } else {
      for (int ks = 0; ks < ksteps; ++ks)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cb_load8(arow + ks * 32, aok), cb_load8(qp + ks * 32, bok), acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (c0 + g4 * 4 + r < p.C) out[(long long)r * LT + f * 16] = acc[r];
  }
}

struct CbiArgs {
  const long long* dcoff;     // doc_cen_off [corpus_len + 1]
  const int* dcen;            // doc_cen [n_pairs]
  long long n_pairs, corpus_len;
  int C;
  const float* T;             // [nq, C, LT]
  int nq, LQ, pool;           // pool: 0 sum, 1 max
  const long long* cand_off;  // [nq + 1]
  const int* cand_doc;        // [n_cand]
  long long n_cand;
  long long pos_begin;        // first candidate position of the window
  int cols;                   // positions in the window
  float* S;                   // [nq, ld]
  long long ld;
  int LT;                     // table columns per centroid
};

__global__ __launch_bounds__(256) void cbi_score_kernel(CbiArgs p) {
  extern __shared__ __align__(16) unsigned char cbi_terms[];  // term table [CBC_RUNP][tstride]
  __shared__ long long sc0[CBC_RUNP], sc1[CBC_RUNP];
  __shared__ int sok[CBC_RUNP];
  __shared__ int next;
  const int tid = threadIdx.x, lane = tid & 63;
  const int n = (int)blockIdx.y;
  const int pl0 = (int)blockIdx.x * CBC_RUNP;
  const int np = p.cols - pl0 < CBC_RUNP ? p.cols - pl0 : CBC_RUNP;
  const int tstride = p.LT + 1;  // floats per position (+ 1: the owners' reads spread over the banks)
  float* TT = reinterpret_cast<float*>(cbi_terms);

  if (tid < np) {
    long long lo, hi;
    cbc_range(p.cand_off, p.n_cand, n, lo, hi);
    const long long pos = p.pos_begin + pl0 + tid;
    int ok = 0;
    long long c0 = 0, c1 = 0;
    if (pos < hi - lo) {
      const long long doc = p.cand_doc[lo + pos];
      if (doc >= 0 && doc < p.corpus_len) {
        ok = 1;
        c0 = p.dcoff[doc];
        c1 = p.dcoff[doc + 1];
        c0 = c0 < 0 ? 0 : c0 > p.n_pairs ? p.n_pairs : c0;
        c1 = c1 < 0 ? 0 : c1 > p.n_pairs ? p.n_pairs : c1;
        if (c1 < c0) c1 = c0;
      }
    }
    sok[tid] = ok;
    sc0[tid] = c0;
    sc1[tid] = c1;
  }
  if (tid == 0) next = 0;
  __syncthreads();

  const float* Tn = p.T + (long long)n * p.C * p.LT;
  const int pieces = p.LT / 4;  // 16-byte pieces of a table row
  for (;;) {
    int pl = 0;
    if (lane == 0) pl = atomicAdd(&next, 1);
    pl = __builtin_amdgcn_readfirstlane(pl);
    if (pl >= np) break;
    if (!sok[pl]) continue;
    const long long c0 = sc0[pl], c1 = sc1[pl];
    for (int p0 = 0; p0 < pieces; p0 += 64) {  // one pass per 64 pieces (256 query tokens) of the row
      const int pp = pieces - p0 < 64 ? pieces - p0 : 64;  // (a multiple of 4)
      int lg = 2;                                          // lanes per row: the power of two at or above pp
      while ((1 << lg) < pp) ++lg;
      const int R = 64 >> lg;                              // rows per wave-instruction
      const int piece = lane & ((1 << lg) - 1), slot = lane >> lg;
      const bool pok = piece < pp;
      const float* col = Tn + (p0 + (pok ? piece : 0)) * 4;
      cb_f32x4 m = {0.f, 0.f, 0.f, 0.f};  // the clamp
      for (long long base = c0; base < c1; base += 64) {
        const int id = base + lane < c1 ? p.dcen[base + lane] : -1;  // 64 ids of the list, coalesced
        const int cnt = (int)(c1 - base < 64 ? c1 - base : 64);
        // Branch-free per lane: a lane without a row (an id behind the list or outside [0, C), a piece behind the row) loads row 0 of
        // its column -- inside the table, C >= 1 -- and drops it.  With more than one instruction's rows left, CBI_FLY loads leave
        // back to back before the first fmaxf (R * CBI_FLY divides 64: s0 + u * R + slot < 64); the last R rows take one load.
        int s0 = 0;
        for (; cnt - s0 > R; s0 += R * CBI_FLY) {
          int c[CBI_FLY];
          cb_f32x4 v[CBI_FLY];
          bool ok[CBI_FLY];
#pragma unroll
          for (int u = 0; u < CBI_FLY; ++u) c[u] = __shfl(id, s0 + u * R + slot, 64);
#pragma unroll
          for (int u = 0; u < CBI_FLY; ++u) {
            ok[u] = pok && c[u] >= 0 && c[u] < p.C;
            v[u] = *reinterpret_cast<const cb_f32x4*>(col + (long long)(ok[u] ? c[u] : 0) * p.LT);
          }
#pragma unroll
          for (int u = 0; u < CBI_FLY; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], ok[u] ? v[u][e] : 0.f);  // 0 is neutral: m starts at 0
          }
        }
        if (s0 < cnt) {
          const int c = __shfl(id, s0 + slot, 64);
          const bool ok = pok && c >= 0 && c < p.C;
          const cb_f32x4 v = *reinterpret_cast<const cb_f32x4*>(col + (long long)(ok ? c : 0) * p.LT);
#pragma unroll
          for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], ok ? v[e] : 0.f);
        }
      }
      // the passage's maxima are complete: fold the row slots, one term per query token into the table
      for (int o = 1 << lg; o < 64; o <<= 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], __shfl_xor(m[e], o, 64));
      }
      if (lane < pp) {
        float* tt = TT + pl * tstride + (p0 + lane) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) tt[e] = m[e];
      }
    }
  }
  __syncthreads();
  // one owner per cell: the query's LQ terms in ascending token order; a position without a candidate is a quiet NaN
  if (tid < np) {
    float acc = __builtin_nanf("");
    if (sok[tid]) {
      const float* tt = TT + tid * tstride;
      acc = tt[0];
      for (int i = 1; i < p.LQ; ++i) acc = p.pool ? fmaxf(acc, tt[i]) : acc + tt[i];
    }
    p.S[(long long)n * p.ld + pl0 + tid] = acc;
  }
}

}  // namespace dprhot
