// maxsim.h -- late-interaction (MaxSim) expert scoring of ColBERT / COIL / CITADEL without the token-level score tensor
// (dpr_scale/task/citadel_task.py:155-238 of the reference).
//
//   S[q, y] = POOL_{i, kq} MAX_{j, kd} <Q[q, i], C[ctx, j]> * [id_q(q, i, kq) == id_c(ctx, j, kd)] * w_q(q, i, kq) * w_c(ctx, j, kd)
//
// Operands are bf16 token rows, zero-padded on the host to a multiple of 32 features (dp).  "Row" = one query token (q, i), flattened
// r = q * LQ + i; "row slot" = (r, kq), flattened r * KQ + kq; "context slot" = (j, kd), flattened j * KD + kd (the reference's view).
// In-batch: y runs over all Nc contexts, ctx = y.  Pairwise (M > 0): query q meets only its own contexts, y < M, ctx = q * M + y.
//
// Launches
//   ms_fwd_kernel   the token GEMM on v_mfma_f32_16x16x32_bf16, a running (max, argmax) per row slot in the epilogue; writes the
//                   [Ny, Nq*LQ*KQ] value / argmax tables (and the raw dot product at the argmax when weights are present)
//   ms_pool_kernel  one wave per (q, y): sum or max over the query's row slots, -inf at masked contexts
//   ms_score_kernel forward only, pairwise: both of the above in one launch, no tables (one workgroup per (q, y); see its comment)
//   ms_dq_kernel    backward, one wave per row: gathers the selected context rows in a fixed (kq, y) order; dW_q
//   ms_dc_kernel    backward, one workgroup per (context, 64-feature slice): wave w owns context tokens j = w (mod 4) and adds the
//                   selected query rows into an LDS accumulator in increasing row-slot order; dW_c
// No fp32 atomics anywhere: every output element has one owner that adds in a fixed order, so two runs are bit-identical.
// Ties: the first maximal context slot wins (strict > within a lane, lower index on equal values across lanes), as torch.max(dim).
// NaN propagates as in torch.max: a NaN beats every number (the first NaN wins), so a NaN token gives a NaN score, never a sentinel.
// Every argmax written is a valid slot index; the backward kernels clamp the indices they read all the same.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dprhot {

constexpr int MS_BM = 64;        // rows per forward workgroup (4 waves x 16)
constexpr int MS_BN = 64;        // context tokens per epilogue chunk (4 MFMA column fragments)
constexpr int MS_KMAX = 8;       // KQ, KD <= 8
constexpr int MS_DC_SLICE = 64;  // features per dC workgroup (one per lane)
constexpr int MS_DQ_CHUNK = 256; // features per dQ wave pass (4 per lane)

struct MsArgs {
  const uint16_t* q;   // bf16 [Nq * LQ, dp]
  const uint16_t* c;   // bf16 [Nc * LD, dp]
  const int* qid;      // [Nq * LQ * KQ] or null
  const int* cid;      // [Nc * LD * KD] or null
  const float* qw;     // [Nq * LQ * KQ] or null
  const float* cw;     // [Nc * LD * KD] or null
  const uint8_t* mask; // [Nc] (context index) or null
  int Nq, LQ, Nc, LD, dp, KQ, KD, M, Ny, pool;  // pool: 0 sum, 1 max
  float* val;          // [Ny, Nq*LQ*KQ] max value per row slot
  int* arg;            // [Ny, Nq*LQ*KQ] argmax context slot
  float* raw;          // [Ny, Nq*LQ*KQ] <Q, C> at the argmax (weights present), else null
  int* parg;           // [Nq, Ny] argmax row slot of max pooling
  float* S;            // [Nq, Ny]
};

__device__ __forceinline__ int ms_ctx(const MsArgs& p, int q, int y) { return p.M > 0 ? q * p.M + y : y; }

// (v2, i2) beats (v1, i1): NaN beats numbers; equal values (and two NaNs) go to the lower index.  An empty candidate is
// (-inf, MS_NONE): any real slot beats it (MS_NONE is larger than every slot index).
constexpr int MS_NONE = 0x7fffffff;
__device__ __forceinline__ bool ms_better(float v2, int i2, float v1, int i1) {
  const bool n2 = __builtin_isnan(v2), n1 = __builtin_isnan(v1);
  if (n2 || n1) return n2 && (!n1 || i2 < i1);
  return v2 > v1 || (v2 == v1 && i2 < i1);
}

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short ms_bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float ms_f32x4;

__device__ __forceinline__ ms_bf16x8 ms_load8(const uint16_t* p, bool ok) {
  ms_bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? *reinterpret_cast<const ms_bf16x8*>(p) : z;
}

__device__ __forceinline__ float ms_bf(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// One workgroup: rows [r0, rend) of one query block against context ctx.  KQT >= KQ is the compile-time slot count.
template <int KQT, bool IDS, bool W>
__global__ __launch_bounds__(256) void ms_fwd_kernel(MsArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = p.Nq * p.LQ;
  int ntiles, tile, y = 0, r0, rend;
  if (p.M > 0) {
    const int tpq = (p.LQ + MS_BM - 1) / MS_BM;
    ntiles = p.Nq * tpq;
    y = (int)(blockIdx.x / (unsigned)ntiles);
    tile = (int)(blockIdx.x - (unsigned)y * ntiles);
    const int b = tile / tpq;
    r0 = b * p.LQ + (tile - b * tpq) * MS_BM;
    rend = min(r0 + MS_BM, (b + 1) * p.LQ);
  } else {
    ntiles = (R + MS_BM - 1) / MS_BM;
    y = (int)(blockIdx.x / (unsigned)ntiles);
    tile = (int)(blockIdx.x - (unsigned)y * ntiles);
    r0 = tile * MS_BM;
    rend = min(r0 + MS_BM, R);
  }
  const int ctx = p.M > 0 ? (r0 / p.LQ) * p.M + y : y;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int ra = r0 + wave * 16 + i16;  // A-operand row of this lane
  const bool ra_ok = ra < rend;
  const uint16_t* qa = p.q + (long)(ra_ok ? ra : r0) * p.dp + g4 * 8;
  const uint16_t* cbase = p.c + (long)ctx * p.LD * p.dp + g4 * 8;
  const int KD = p.KD;

  float bv[4][KQT], bs[4][KQT];
  int bi[4][KQT];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int k = 0; k < KQT; ++k) { bv[r][k] = -INFINITY; bs[r][k] = 0.f; bi[r][k] = MS_NONE; }

  for (int c0 = 0; c0 < p.LD; c0 += MS_BN) {
    ms_f32x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = ms_f32x4{0.f, 0.f, 0.f, 0.f};
    int col[4];
    bool cok[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) { col[b] = c0 + b * 16 + i16; cok[b] = col[b] < p.LD; }
    for (int k = 0; k < p.dp; k += 32) {
      const ms_bf16x8 af = ms_load8(qa + k, ra_ok);
      ms_bf16x8 bfr[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) bfr[b] = ms_load8(cbase + (long)(cok[b] ? col[b] : 0) * p.dp + k, cok[b]);
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[b], acc[b], 0, 0, 0);
    }
    // epilogue: lane holds rows wave*16 + g4*4 + r, column col[b]; columns visited in increasing (j, kd) order
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (!cok[b]) continue;
      const long cs = ((long)ctx * p.LD + col[b]) * KD;
      for (int kd = 0; kd < KD; ++kd) {
        const int idc = IDS ? p.cid[cs + kd] : 0;
        const float wc = W ? p.cw[cs + kd] : 1.f;
        const int idx = col[b] * KD + kd;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = acc[b][r];
          const int rq = min(r0 + wave * 16 + g4 * 4 + r, rend - 1);  // this lane's row (rows past the tile end are never written)
#pragma unroll
          for (int kq = 0; kq < KQT; ++kq) {
            if (kq >= p.KQ) break;
            bool match = true;
            if (IDS) match = p.qid[(long)rq * p.KQ + kq] == idc;
            // the reference's order: s * (match ? w_q * w_c : 0) -- an unmatched slot is s * 0 (0, or NaN for a NaN score)
            float f = 1.f;
            if (W) f = p.qw[(long)rq * p.KQ + kq] * wc;
            if (!match) f = 0.f;
            const float v = (IDS || W) ? s * f : s;
            if (ms_better(v, idx, bv[r][kq], bi[r][kq])) { bv[r][kq] = v; bi[r][kq] = idx; if (W) bs[r][kq] = s; }
          }
        }
      }
    }
  }
  // combine the 16 lanes that share a row (lower index on equal values), then lane i16 == 0 writes
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int kq = 0; kq < KQT; ++kq) {
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) {
        const float v2 = __shfl_xor(bv[r][kq], off, 64);
        const int i2 = __shfl_xor(bi[r][kq], off, 64);
        const float s2 = __shfl_xor(bs[r][kq], off, 64);
        if (ms_better(v2, i2, bv[r][kq], bi[r][kq])) { bv[r][kq] = v2; bi[r][kq] = i2; bs[r][kq] = s2; }
      }
    }
  if (i16 == 0) {
    const long RK = (long)R * p.KQ;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + wave * 16 + g4 * 4 + r;
      if (row >= rend) continue;
#pragma unroll
      for (int kq = 0; kq < KQT; ++kq) {
        if (kq >= p.KQ) break;
        const long o = (long)y * RK + (long)row * p.KQ + kq;
        p.val[o] = bv[r][kq];
        p.arg[o] = bi[r][kq] == MS_NONE ? 0 : bi[r][kq];  // (only reachable when every slot is -inf)
        if (W && p.raw) p.raw[o] = bs[r][kq];
      }
    }
  }
}

// One wave per (q, y): pool over the LQ * KQ row slots of query q (fixed lane order + fixed xor tree: deterministic).
__global__ __launch_bounds__(256) void ms_pool_kernel(MsArgs p) {
  const int lane = threadIdx.x & 63;
  const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= (long)p.Nq * p.Ny) return;
  const int q = (int)(pair / p.Ny), y = (int)(pair - (long)q * p.Ny);
  const int n = p.LQ * p.KQ;
  const long base = (long)y * p.Nq * n + (long)q * n;
  float acc = p.pool ? -INFINITY : 0.f;
  int ai = MS_NONE;
  for (int s = lane; s < n; s += 64) {
    const float v = p.val[base + s];
    if (p.pool) {
      if (ms_better(v, s, acc, ai)) { acc = v; ai = s; }
    } else {
      acc += v;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float v2 = __shfl_xor(acc, off, 64);
    if (p.pool) {
      const int i2 = __shfl_xor(ai, off, 64);
      if (ms_better(v2, i2, acc, ai)) { acc = v2; ai = i2; }
    } else {
      acc += v2;
    }
  }
  if (lane == 0) {
    const int ctx = ms_ctx(p, q, y);
    p.S[pair] = (p.mask && p.mask[ctx]) ? -INFINITY : acc;
    if (p.pool) p.parg[pair] = q * n + (ai == MS_NONE ? 0 : ai);
  }
}

// Score only (inference: reranking aligned pairs): ms_fwd_kernel + ms_pool_kernel in pairwise mode as ONE launch with no tables.
// One workgroup per (q, y), blockIdx.x = ctx = q * M + y.  The query's rows go in tiles of 16 * nrf tokens, nrf = 1 (LQ <= 16),
// 2 (LQ <= 32) or 4 MFMA row fragments; wave w works on fragment w % nrf and column group w / nrf, and the 4 / nrf column groups take
// alternate 64-token chunks of the passage -- so four waves stay busy at a rerank query's 32 tokens.  ms_better is a total order, so
// its maximum does not depend on how the columns are split.  Each wave leaves its row slots' (max, argmax) in LDS, one plane per
// column group (argmax planes exist only where there is more than one group: they settle equal values, +0 against -0, as the
// tables' lowest-index rule does).  After one barrier wave 0 merges the planes and pools the n = LQ * KQ slots in ms_pool_kernel's
// order -- lane l takes slots l, l + 64, ... in increasing order, then the xor tree 32 .. 1 -- so the fp32 sum is the same to the bit.
constexpr int MS_SC_SLOTS = 512 * MS_KMAX;     // LQ <= 512 (DPRHOT_MAXSIM_MAX_LEN): 4096 row slots, the 16 KiB value table
constexpr int MS_SC_SPLIT = 32 * MS_KMAX * 2;  // LQ <= 32: at most 4 planes x 16 tokens x 8 = 2 planes x 32 tokens x 8 slots

template <int KQT, bool IDS, bool W>
__global__ __launch_bounds__(256) void ms_score_kernel(MsArgs p) {
  __shared__ float tab[MS_SC_SLOTS];
  __shared__ int tix[MS_SC_SPLIT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ctx = (int)blockIdx.x;
  const int q = ctx / p.M;
  const int LQ = p.LQ, KD = p.KD, n = LQ * p.KQ;
  const int nrf = LQ <= 16 ? 1 : LQ <= 32 ? 2 : 4;
  const int ncg = 4 / nrf;
  const int frag = wave % nrf, cg = wave / nrf;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int qr0 = q * LQ;  // first global row of this query
  const uint16_t* cbase = p.c + (long)ctx * p.LD * p.dp + g4 * 8;

  for (int t0 = 0; t0 < LQ; t0 += 16 * nrf) {
    const int f0 = t0 + frag * 16;  // first query token of this wave's fragment
    if (f0 >= LQ) continue;         // (wave-uniform; the barrier is outside the loop)
    const int ia = f0 + i16;        // A-operand token of this lane
    const bool ra_ok = ia < LQ;
    const uint16_t* qa = p.q + (long)(qr0 + (ra_ok ? ia : f0)) * p.dp + g4 * 8;

    float bv[4][KQT];
    int bi[4][KQT];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int k = 0; k < KQT; ++k) { bv[r][k] = -INFINITY; bi[r][k] = MS_NONE; }

    for (int c0 = cg * MS_BN; c0 < p.LD; c0 += ncg * MS_BN) {
      ms_f32x4 acc[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = ms_f32x4{0.f, 0.f, 0.f, 0.f};
      int col[4];
      bool cok[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) { col[b] = c0 + b * 16 + i16; cok[b] = col[b] < p.LD; }
      for (int k = 0; k < p.dp; k += 32) {
        const ms_bf16x8 af = ms_load8(qa + k, ra_ok);
        ms_bf16x8 bfr[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) bfr[b] = ms_load8(cbase + (long)(cok[b] ? col[b] : 0) * p.dp + k, cok[b]);
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[b], acc[b], 0, 0, 0);
      }
      // epilogue as in ms_fwd_kernel: lane holds tokens f0 + g4*4 + r, column col[b]
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (!cok[b]) continue;
        const long cs = ((long)ctx * p.LD + col[b]) * KD;
        for (int kd = 0; kd < KD; ++kd) {
          const int idc = IDS ? p.cid[cs + kd] : 0;
          const float wc = W ? p.cw[cs + kd] : 1.f;
          const int idx = col[b] * KD + kd;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float s = acc[b][r];
            const long rq = qr0 + min(f0 + g4 * 4 + r, LQ - 1);  // (tokens past the query's end are never written)
#pragma unroll
            for (int kq = 0; kq < KQT; ++kq) {
              if (kq >= p.KQ) break;
              bool match = true;
              if (IDS) match = p.qid[rq * p.KQ + kq] == idc;
              float f = 1.f;
              if (W) f = p.qw[rq * p.KQ + kq] * wc;
              if (!match) f = 0.f;
              const float v = (IDS || W) ? s * f : s;
              if (ms_better(v, idx, bv[r][kq], bi[r][kq])) { bv[r][kq] = v; bi[r][kq] = idx; }
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int kq = 0; kq < KQT; ++kq) {
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
          const float v2 = __shfl_xor(bv[r][kq], off, 64);
          const int i2 = __shfl_xor(bi[r][kq], off, 64);
          if (ms_better(v2, i2, bv[r][kq], bi[r][kq])) { bv[r][kq] = v2; bi[r][kq] = i2; }
        }
      }
    if (i16 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = f0 + g4 * 4 + r;
        if (i >= LQ) continue;
#pragma unroll
        for (int kq = 0; kq < KQT; ++kq) {
          if (kq >= p.KQ) break;
          const int o = cg * n + i * p.KQ + kq;  // ncg > 1 only with LQ <= 32: ncg * n <= MS_SC_SPLIT
          tab[o] = bv[r][kq];
          if (ncg > 1) tix[o] = bi[r][kq];
        }
      }
    }
  }
  __syncthreads();
  if (wave != 0) return;
  float acc = p.pool ? -INFINITY : 0.f;
  int ai = MS_NONE;
  for (int s = lane; s < n; s += 64) {
    float v = tab[s];
    if (ncg > 1) {
      int vi = tix[s];
      for (int g = 1; g < ncg; ++g) {
        const float v2 = tab[g * n + s];
        const int i2 = tix[g * n + s];
        if (ms_better(v2, i2, v, vi)) { v = v2; vi = i2; }
      }
    }
    if (p.pool) {
      if (ms_better(v, s, acc, ai)) { acc = v; ai = s; }
    } else {
      acc += v;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float v2 = __shfl_xor(acc, off, 64);
    if (p.pool) {
      const int i2 = __shfl_xor(ai, off, 64);
      if (ms_better(v2, i2, acc, ai)) { acc = v2; ai = i2; }
    } else {
      acc += v2;
    }
  }
  if (lane == 0) p.S[ctx] = (p.mask && p.mask[ctx]) ? -INFINITY : acc;
}

struct MsBwd {
  const float* dS;   // [Nq, Ny]
  float* dq;         // fp32 [Nq * LQ, dp] or null
  float* dc;         // fp32 [Nc * LD, dp] or null
  float* dwq;        // [Nq * LQ * KQ] or null
  float* dwc;        // [Nc * LD * KD] or null
};

// Gradient of S[q, y] reaching row slot rs (global) through the argmax: 0 at masked contexts, and under max pooling everywhere but
// at the pooled row slot.  `cm` is the match indicator times (w_q * w_c) -- the factor the forward multiplied the dot product by.
__device__ __forceinline__ float ms_grad(const MsArgs& p, const MsBwd& g, int q, int y, int rs) {
  const int ctx = ms_ctx(p, q, y);
  if (p.mask && p.mask[ctx]) return 0.f;
  const long o = (long)q * p.Ny + y;
  if (p.pool && p.parg[o] != rs) return 0.f;
  return g.dS[o];
}

// One wave per row r = (q, i), one 256-feature chunk per blockIdx.y; the (kq, y) order of the sum is fixed.
template <bool IDS, bool W>
__global__ __launch_bounds__(256) void ms_dq_kernel(MsArgs p, MsBwd g) {
  const int lane = threadIdx.x & 63;
  const int r = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= p.Nq * p.LQ) return;
  const int q = r / p.LQ;
  const int f0 = (int)blockIdx.y * MS_DQ_CHUNK + lane * 4;
  const bool fok = f0 < p.dp;
  const long RK = (long)p.Nq * p.LQ * p.KQ;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int kq = 0; kq < p.KQ; ++kq) {
    const int rs = r * p.KQ + kq;
    const int idq = IDS ? p.qid[rs] : 0;
    const float wq = W ? p.qw[rs] : 1.f;
    float dw = 0.f;
    for (int y0 = 0; y0 < p.Ny; y0 += 64) {
      const int y = y0 + lane;
      float cf = 0.f;
      int row = 0;  // context token row (ctx * LD + j) of this lane's y
      if (y < p.Ny) {
        const int ctx = ms_ctx(p, q, y);
        const int a = min(max(p.arg[(long)y * RK + rs], 0), p.LD * p.KD - 1);
        const int j = a / p.KD;
        row = ctx * p.LD + j;
        const float gr = ms_grad(p, g, q, y, rs);
        const long cs = (long)row * p.KD + (a - j * p.KD);
        const bool match = !IDS || p.cid[cs] == idq;
        const float wc = W ? p.cw[cs] : 1.f;
        if (match) {
          cf = W ? gr * (wq * wc) : gr;
          if (W) dw += gr * p.raw[(long)y * RK + rs] * wc;
        }
      }
      if (g.dq) {  // (the shuffles run on every lane: a lane outside the feature range still holds its y's entry)
        const int n = min(64, p.Ny - y0);
        for (int t0 = 0; t0 < n; t0 += 8) {
          float c8[8];
          uint2 v8[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int t = min(t0 + u, n - 1);
            c8[u] = t0 + u < n ? __shfl(cf, t, 64) : 0.f;
            const int rw = __shfl(row, t, 64);
            v8[u] = fok ? *reinterpret_cast<const uint2*>(p.c + (long)rw * p.dp + f0) : make_uint2(0u, 0u);
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (c8[u] == 0.f) continue;
            acc[0] += c8[u] * ms_bf((uint16_t)(v8[u].x & 0xffff));
            acc[1] += c8[u] * ms_bf((uint16_t)(v8[u].x >> 16));
            acc[2] += c8[u] * ms_bf((uint16_t)(v8[u].y & 0xffff));
            acc[3] += c8[u] * ms_bf((uint16_t)(v8[u].y >> 16));
          }
        }
      }
    }
    if (W && g.dwq && blockIdx.y == 0) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) dw += __shfl_xor(dw, off, 64);
      if (lane == 0) g.dwq[rs] = dw;
    }
  }
  if (g.dq && fok) *reinterpret_cast<float4*>(g.dq + (long)r * p.dp + f0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// One workgroup per (context, 64-feature slice).  Dynamic LDS: LD * 64 fp32 accumulator (+ LD * KD fp32 for dW_c).
template <bool IDS, bool W>
__global__ __launch_bounds__(256) void ms_dc_kernel(MsArgs p, MsBwd g) {
  extern __shared__ float ms_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ctx = (int)blockIdx.x;
  const int f = (int)blockIdx.y * MS_DC_SLICE + lane;
  const bool fok = f < p.dp;
  const bool do_dw = W && g.dwc && blockIdx.y == 0;
  float* acc = ms_lds;
  float* dwl = ms_lds + (long)p.LD * MS_DC_SLICE;
  for (int e = tid; e < p.LD * MS_DC_SLICE; e += 256) acc[e] = 0.f;
  if (do_dw)
    for (int e = tid; e < p.LD * p.KD; e += 256) dwl[e] = 0.f;
  __syncthreads();
  const int n = p.LQ * p.KQ;  // row slots per query
  const long RK = (long)p.Nq * n;
  int y, rs_beg, rs_end;
  if (p.M > 0) {
    const int b = ctx / p.M;
    y = ctx - b * p.M;
    rs_beg = b * n;
    rs_end = rs_beg + n;
  } else {
    y = ctx;
    rs_beg = 0;
    rs_end = (int)RK;
  }
  for (int s0 = rs_beg; s0 < rs_end; s0 += 64) {
    const int rs = s0 + lane;
    bool hit = false;
    float cf = 0.f, dwv = 0.f;
    int j = 0, slot = 0;
    if (rs < rs_end) {
      const int a = min(max(p.arg[(long)y * RK + rs], 0), p.LD * p.KD - 1);
      j = a / p.KD;
      slot = a;
      if ((j & 3) == wave) {
        const int q = rs / n;
        const float gr = ms_grad(p, g, q, y, rs);
        const long cs = (long)ctx * p.LD * p.KD + a;
        const bool match = !IDS || p.cid[cs] == p.qid[rs];
        if (match && gr != 0.f) {
          hit = true;
          const float wq = W ? p.qw[rs] : 1.f;
          cf = W ? gr * (wq * p.cw[cs]) : gr;
          if (W) dwv = gr * p.raw[(long)y * RK + rs] * wq;
        }
      }
    }
    uint64_t m = __ballot(hit);
    while (m) {  // up to 8 hits per round: their row loads are in flight together
      int t8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (m) {
          t8[u] = __builtin_ctzll(m);
          m &= m - 1;
        } else {
          t8[u] = -1;
        }
      }
      uint16_t v8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int rw = __shfl(rs, t8[u] < 0 ? 0 : t8[u], 64) / p.KQ;
        v8[u] = (fok && t8[u] >= 0) ? p.q[(long)rw * p.dp + f] : (uint16_t)0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (t8[u] < 0) break;
        const float c = __shfl(cf, t8[u], 64);
        const int jj = __shfl(j, t8[u], 64);
        acc[jj * MS_DC_SLICE + lane] += c * ms_bf(v8[u]);
        if (do_dw) {
          const float dv = __shfl(dwv, t8[u], 64);
          const int sl = __shfl(slot, t8[u], 64);
          if (lane == 0) dwl[sl] += dv;
        }
      }
    }
  }
  __syncthreads();
  if (g.dc)
    for (int jr = wave; jr < p.LD; jr += 4)
      if (fok) g.dc[((long)ctx * p.LD + jr) * p.dp + f] = acc[jr * MS_DC_SLICE + lane];
  if (do_dw)
    for (int e = tid; e < p.LD * p.KD; e += 256) g.dwc[(long)ctx * p.LD * p.KD + e] = dwl[e];
}

}  // namespace dprhot
