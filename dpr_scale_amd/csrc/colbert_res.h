// colbert_res.h -- MaxSim over candidate lists of a RESIDUAL-COMPRESSED token index: the exact stage of the
// pruned search (colbert_cand.h) over rows stored as a centroid id plus NB bits per feature, the ColBERTv2 format.
//
// Index   the block layout of colbert.h (dblk, 16 rows per block); per row tok_centroid int32 [n_blk * 16] and res_code uint8
//         [n_blk * 16, rb], rb = dp * NB / 8; per index centroids bf16 [C, dp] and ONE bucket set: weights fp32 [2^NB] (cutoffs fp32
//         [2^NB - 1] for the encoder).  code(r, t) = (res_code[r][t * NB / 8] >> (NB * (t mod (8 / NB)))) & (2^NB - 1).
// Decode  tok[r][t] = 0 <= tok_centroid[r] < C ? bf16_rne(float(centroids[tok_centroid[r]][t]) + weights[code(r, t)]) : 0
//         ONE fp32 addition, then round to nearest even.  A row whose id lies outside [0, C) is an exact zero whatever its code bytes
//         hold; every code value decodes.
// Encode  code = number of j with float(tok[r][t]) - float(centroids[tok_centroid[r]][t]) > cutoffs[j] (one fp32 subtraction; a NaN
//         residual encodes as 0); a row whose id lies outside [0, C) gets zero bytes.
//
// cbr_score_kernel writes, bit for bit, the cell cbc_score_kernel writes for the decoded index: the window contract, the plan and the
// bounds are that kernel's, word for word -- grid (runs of CBC_RUNP positions) x (query), the first CBC_RUNP threads resolve positions
// into LDS, the waves take passages from an LDS counter, CBC_QW query fragments per pass in registers, the token block is the A operand
// of v_mfma_f32_16x16x32_bf16, k-steps ascending from a zero accumulator, fmaxf chain from 0, LDS term table, one owner per cell pooling
// in ascending token order, a quiet NaN where there is no candidate, no floating-point atomics.  The one difference is the A operand,
// decoded at the operand read: lane (i16, g4) at k-step ks holds features 32 ks + 8 g4 .. + 7 of row i16 -- the row's centroid id (one
// int32 per row and block), 16 bytes of that centroid row (gathered from global memory: the table is C * dp * 2 bytes and lives in
// L2 / Infinity Cache), NB code bytes, eight weight lookups in LDS, eight fp32 adds and four packed conversions to bf16.
// In flight under block b's MFMAs: the ids of block b + 2, the code bytes and the centroid pieces of block b + 1 (a centroid piece's
// address needs its id, hence the ids run one block further ahead).
// Bounds  those of cbc_score_kernel, and: a centroid id outside [0, C) is never used as an index; nothing behind
//         res_code[n_blk * 16 * rb - 1], tok_centroid[n_blk * 16 - 1] or centroids[C * dp - 1] is read whatever the index holds.
#pragma once

#include "colbert_cand.h"

namespace dprhot {

constexpr int CBR_MAX_DP = 128;     // query fragments and a block's raw operands stay in registers
constexpr int CBR_ENC_THREADS = 256;

struct CbrArgs {
  const uint8_t* code;        // [n_blk * 16, dp * NB / 8]
  const int* tcen;            // [n_blk * 16]
  const uint16_t* cen;        // bf16 [C, dp]
  int C;
  const float* weights;       // [2^NB]
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

struct CbrEncArgs {
  const uint16_t* tok;        // bf16 [n, dp]
  const int* tcen;            // [n]
  long long n;
  int dp;
  const uint16_t* cen;        // bf16 [C, dp]
  int C;
  const float* cutoffs;       // [2^NB - 1]
  uint8_t* code;              // [n, dp * NB / 8]
};

typedef __attribute__((__vector_size__(2 * sizeof(float)))) float cbr_f32x2;
typedef __attribute__((__vector_size__(2 * sizeof(__bf16)))) __bf16 cbr_bf16x2;

__device__ __forceinline__ float cbr_bf16_f32(short h) { return __uint_as_float((uint32_t)(uint16_t)h << 16); }

// the NB code bytes of eight consecutive features, little-endian: feature j of the eight is (bits >> (NB * j)) & (2^NB - 1)
template <int NB>
__device__ __forceinline__ uint32_t cbr_load_code(const uint8_t* p, bool ok) {
  if (!ok) return 0u;
  if constexpr (NB == 1) return *p;
  if constexpr (NB == 2) return *reinterpret_cast<const uint16_t*>(p);
  return *reinterpret_cast<const uint32_t*>(p);
}

// eight decoded features as the MFMA's bf16 operand: bf16_rne(centroid + weight) in pairs, zero for a row without a centroid
template <int NB>
__device__ __forceinline__ cb_bf16x8 cbr_decode8(cb_bf16x8 cen, uint32_t bits, bool ok, const float* sw) {
  union {
    cb_bf16x8 v;
    cbr_bf16x2 h[4];
  } u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cbr_f32x2 s;
    s[0] = cbr_bf16_f32(cen[2 * j]) + sw[(bits >> (NB * 2 * j)) & ((1u << NB) - 1)];
    s[1] = cbr_bf16_f32(cen[2 * j + 1]) + sw[(bits >> (NB * (2 * j + 1))) & ((1u << NB) - 1)];
    u.h[j] = __builtin_convertvector(s, cbr_bf16x2);
  }
  const cb_bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? u.v : z;
}

// KS = dp / 32 (dp <= 128): query fragments in registers
template <int NB, int KS>
__global__ __launch_bounds__(256) void cbr_score_kernel(CbrArgs p) {
  extern __shared__ __align__(16) unsigned char cbr_table[];  // T [CBC_RUNP][tstride]
  __shared__ long long sb0[CBC_RUNP], sb1[CBC_RUNP];
  __shared__ int sok[CBC_RUNP];
  __shared__ int next[CBC_PASSES];
  __shared__ float sw[1 << NB];
  constexpr int RB = KS * 32 * NB / 8;  // code bytes per row
  constexpr int DP = KS * 32;
  const int tid = threadIdx.x, lane = tid & 63;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int n = (int)blockIdx.y;
  const int pl0 = (int)blockIdx.x * CBC_RUNP;
  const int np = p.cols - pl0 < CBC_RUNP ? p.cols - pl0 : CBC_RUNP;
  const int tstride = p.FQ * 16 + 1;  // floats per position (+ 1: the owners' reads spread over the banks)
  float* T = reinterpret_cast<float*>(cbr_table);

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
  if (tid >= 64 && tid < 64 + (1 << NB)) sw[tid - 64] = p.weights ? p.weights[tid - 64] : 0.f;  // (NULL with n_blk == 0: nothing decodes)
  __syncthreads();

  for (int f0 = 0, pass = 0; f0 < p.FQ; f0 += CBC_QW, ++pass) {
    const int nfr = p.FQ - f0 < CBC_QW ? p.FQ - f0 : CBC_QW;  // this pass's fragments are slots i < nfr
    cb_bf16x8 bq[CBC_QW][KS];
#pragma unroll
    for (int i = 0; i < CBC_QW; ++i) {
      const int t = (f0 + i) * 16 + i16;
      const bool bok = i < nfr && t < p.LQ;
      const uint16_t* qp = p.q + ((long long)n * p.LQ + (bok ? t : 0)) * DP + g4 * 8;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) bq[i][ks] = cb_load8(qp + ks * 32, bok);
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
      // lane's row of the block: its id, and its NB code bytes / 16 centroid bytes of k-step 0
      const int* idp = p.tcen + b0 * 16 + i16;
      const uint8_t* crow = p.code + (b0 * 16 + i16) * RB + g4 * NB;
      const uint16_t* cbase = p.cen + g4 * 8;
      // ids: block b0 (c0) and b0 + 1 (c1); raw operands of block b0
      int c0 = b0 < b1 ? idp[0] : -1;
      int c1 = b0 + 1 < b1 ? idp[16] : -1;
      bool ok0 = c0 >= 0 && c0 < p.C;
      uint32_t bits[KS];
      cb_bf16x8 cp[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        bits[ks] = cbr_load_code<NB>(crow + ks * 4 * NB, ok0);
        cp[ks] = cb_load8(cbase + (long long)(ok0 ? c0 : 0) * DP + ks * 32, ok0);
      }
      for (long long b = b0; b < b1; ++b) {
        // in flight under this block's MFMAs: the ids of block b + 2, the code bytes and centroid pieces of block b + 1
        idp += 16;
        crow += 16 * RB;
        const int c2 = b + 2 < b1 ? idp[16] : -1;
        const bool ok1 = c1 >= 0 && c1 < p.C;  // (c1 is -1 behind the passage's last block)
        uint32_t bitsn[KS];
        cb_bf16x8 cpn[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          bitsn[ks] = cbr_load_code<NB>(crow + ks * 4 * NB, ok1);
          cpn[ks] = cb_load8(cbase + (long long)(ok1 ? c1 : 0) * DP + ks * 32, ok1);
        }
        cb_bf16x8 a[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = cbr_decode8<NB>(cp[ks], bits[ks], ok0, sw);
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
        for (int ks = 0; ks < KS; ++ks) {
          bits[ks] = bitsn[ks];
          cp[ks] = cpn[ks];
        }
        ok0 = ok1;
        c1 = c2;
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

// one thread per (row, 8 features): 16 bytes of the token row, 16 bytes of the centroid row, NB bytes out; writes every byte of
// code [n, dp * NB / 8] and nothing else
template <int NB>
__global__ __launch_bounds__(CBR_ENC_THREADS) void cbr_encode_kernel(CbrEncArgs p) {
  const int ppr = p.dp / 8;  // 8-feature pieces per row
  const long long pieces = p.n * ppr;
  float cut[(1 << NB) - 1];
#pragma unroll
  for (int j = 0; j < (1 << NB) - 1; ++j) cut[j] = p.cutoffs[j];
  for (long long t = (long long)blockIdx.x * CBR_ENC_THREADS + threadIdx.x; t < pieces; t += (long long)gridDim.x * CBR_ENC_THREADS) {
    const long long r = t / ppr;
    const int c = p.tcen[r];
    uint32_t bits = 0;
    if (c >= 0 && c < p.C) {
      const int f = (int)(t - r * ppr) * 8;
      const cb_bf16x8 x = *reinterpret_cast<const cb_bf16x8*>(p.tok + t * 8);
      const cb_bf16x8 y = *reinterpret_cast<const cb_bf16x8*>(p.cen + (long long)c * p.dp + f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float res = cbr_bf16_f32(x[j]) - cbr_bf16_f32(y[j]);
        uint32_t code = 0;
#pragma unroll
        for (int i = 0; i < (1 << NB) - 1; ++i) code += res > cut[i] ? 1u : 0u;
        bits |= code << (NB * j);
      }
    }
    if constexpr (NB == 1) p.code[t] = (uint8_t)bits;
    if constexpr (NB == 2) reinterpret_cast<uint16_t*>(p.code)[t] = (uint16_t)bits;
    if constexpr (NB == 4) reinterpret_cast<uint32_t*>(p.code)[t] = bits;
  }
}

}  // namespace dprhot
