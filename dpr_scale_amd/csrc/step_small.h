// step_small.h -- the second (and last) launch of a whole training step at the latency-bound BASELINE shapes
// (B <= 32 queries per rank, Nc <= 1152 gathered contexts, d % 16 == 0: cfg1, cfg2, cfg4 per rank).
//
// dpr_task.py:209-212 (softmax cross-entropy) and the autograd backward of :98-105 (dQ = G C, dC = G^T Q) in ONE
// kernel.  At these sizes every launch costs a kernel boundary plus one dependent trip to memory (~3.7 us), whatever it
// computes, so the step is the number of dependent launches.  The row softmax needs complete rows and the backward GEMMs
// need complete columns of G, which is why they were two launches; here each workgroup owns 64 columns of d, recomputes
// the (tiny: <= 32 x 512) softmax from the partial-logit slabs of the sim launch -- 128 KiB of L2 reads per workgroup at
// cfg2 -- keeps G in LDS and feeds both GEMMs from that one image:
//     dQ[:, n0:n0+64]      = G   x C[:, n0:n0+64]     A = G row-major = k-major fragments (ds_read_b128)
//     dC_part[:, n0:n0+64] = G^T x Q[:, n0:n0+64]     A = the SAME image read through ds_read_b64_tr_b16
// d/16 workgroups of 1024 threads (48 at d = 768), no atomics, fixed summation orders (bit-reproducible); workgroup 0
// also writes loss / logsumexp / G / logits.  What in-kernel stamps showed for a 256-thread version (cfg2, 5.4 us inside
// the kernel): 1.7 us pulling the 128 KiB of slabs + operand tiles through one CU's L1 (64 B/clk), 1.8 us of softmax
// ALU at 32 scores per thread, 0.9 + 0.7 us in two latency-bound MFMA loops -- hence 1024 threads (8 scores each), the
// dQ contraction split over 8 wave pairs and one 16-row block of dC per wave.
#pragma once
#include "gemm_bf16.h"
#include "rowwise.h"

// stamps of the timing build (scratch/step_small_stamps.hip; nothing in the library): slot i of workgroup 0 as before, and the same
// instant in slot i - 8 of the stamping workgroup's own row (the lead does extra stores, an ordinary workgroup does not)
#define SS_TM(i) do { DPRHOT_TM(i); DPRHOT_TMB(0, (i) - 8); } while (0)

namespace dprhot {

constexpr int SS_ROWS = 32;     // query rows of one row block (rows beyond B are zero)
constexpr int SS_MAXB = 64;     // query rows of the launch: two row blocks at most
constexpr int SS_MAXNC = 1152;  // G image + C tile + dQ partials must fit the 160 KiB of LDS
// TW = columns of d per workgroup (16 in the library); the C / Q tile images have row stride TW + 8 elements

struct StepSmallArgs {
  const float* slabs;  // [splits][B][Nc] partial logits (mask and 1/T applied: -inf at masked columns)
  int splits;
  size_t slab_stride;
  int B, Nc, d;
  const int64_t* y;
  int64_t y_offset;
  float grad_scale;
  const uint16_t* Qb;  // [B][d]  bf16 (written by the sim launch)
  const uint16_t* Cb;  // [Nc][d] bf16
  float h_scale;
  const float* d_scale;
  float* dQ;           // [B][d]
  float* dC;           // [Nc][d]
  float* S_out;        // optional [B][Nc]
  float* row_loss;     // optional [B]
  float* row_lse;      // optional [B]
  float* loss_sum;     // [1]
  uint16_t* G;         // optional [B][Nc]
  int stamp_period, stamp_row;  // > 0: dC[m][0] = loss numerator for m % stamp_period == stamp_row (EpiScaleF32)
  float loss_scale = 1.0f;
};

inline size_t step_small_lds(int Nc, int TW) {
  const int ncp = (Nc + 31) / 32 * 32, ts = TW + 8;
  return (size_t)SS_ROWS * (ncp + 8) * 2 + (size_t)ncp * ts * 2 + (size_t)SS_ROWS * ts * 2 + SS_MAXB * sizeof(float) +
         (size_t)8 * SS_ROWS * TW * sizeof(float);  // + the dQ partial sums of the 8 K slices
}

template <int CTRL>
__device__ __forceinline__ float ss_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
// reductions over 8 consecutive lanes (aligned): xor 1, xor 2 inside the quad, then the two quads of the half row
__device__ __forceinline__ float ss_max8(float v) {
  v = fmaxf(v, ss_dpp<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, ss_dpp<0x4E>(v));   // quad_perm [2,3,0,1]
  return fmaxf(v, ss_dpp<0x141>(v));  // row_half_mirror
}
__device__ __forceinline__ float ss_sum8(float v) {
  v += ss_dpp<0xB1>(v);
  v += ss_dpp<0x4E>(v);
  return v + ss_dpp<0x141>(v);
}

__device__ __forceinline__ bf16x8 ss_tr_frag(const uint16_t* T, int stride, int k0, int c0, int lane) {
  // fragment of an [k][col] image for 16 columns c0.. and the 32 k values k0..: see load_frag (gemm_bf16.h)
  const int i = lane & 15, g = lane >> 4;
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const uint16_t* p = T + (k0 + g * 8 + (i >> 2)) * stride + c0 + (i & 3) * 4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(p));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(p + 4 * stride));
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// CPT: 8-value chunks of a row per thread (32 threads per row): Nc <= 256 * CPT.  TW: columns of d per workgroup.
// NS: partial-logit slabs read (>= p.splits; the sim launch writes 1 slab above 512 columns, up to 4 below).
// NRB: row blocks of 32 (1: B <= 32, the body runs once, straight-line as before; 2: B <= 64, unrolled twice).
template <int CPT, int TW, int NS, int NRB = 1>
__global__ __launch_bounds__(1024) void step_small_kernel(StepSmallArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint16_t ss_smem[];
  constexpr int TS = TW + 8;          // tile image row stride (elements)
  constexpr int TC = TW / 8;          // 16-byte chunks per tile row
  constexpr int CU = (256 * CPT * TC + 1023) / 1024;  // C-tile chunks per thread
  constexpr int NF = TW / 16;         // 16-column fragments of the tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // workgroup -> column tile: linear ids are dealt round-robin to the 8 XCDs; give each XCD a CONTIGUOUS run of tiles, so
  // that the 4 neighbouring 16-column tiles that share every 128-byte line of C / Q rows meet in one L2 (PMC: 3.5 MB of
  // HBM traffic per launch at cfg2 with the identity mapping against 1.5 MB algorithmic)
  const int nwg = gridDim.x;
  const int tile = (nwg % 8 == 0) ? (blockIdx.x % 8) * (nwg / 8) + blockIdx.x / 8 : blockIdx.x;
  const int n0 = tile * TW;
  const int Nc = p.Nc, cpr = Nc >> 3;
  const int ncp = (Nc + 31) / 32 * 32, gs = ncp + 8;
  uint16_t* const Gs = ss_smem;                       // [32][gs]   G, row-major
  uint16_t* const Cs = Gs + SS_ROWS * gs;             // [ncp][TS]  C[:, n0:n0+TW]
  uint16_t* const Qs = Cs + ncp * TS;                 // [32][TS]   Q[:, n0:n0+TW]
  float* const s_rl = reinterpret_cast<float*>(Qs + SS_ROWS * TS);  // [SS_MAXB] row losses of all row blocks
  float* const red = s_rl + SS_MAXB;                  // [8][32][TW] dQ partial sums

  // Row blocks of 32 (round 3: B <= 64 -- the per-GPU batch of the DRAGON / NQ recipes -- takes two turns through the body below with
  // the C tile resident and the dC accumulators kept in registers; a third launch plus a G round trip through HBM cost more than
  // the second softmax: 5 + ~2.5 us against ~11).  The first block's loads are all issued back to back with the C tile's.
  const int lrow = tid >> 5, tr = tid & 31;
  const float dsc = p.d_scale ? *p.d_scale : 1.0f;
  const bool lead = tile == 0;
  const float sc = p.h_scale * dsc;
  const int i = lane & 15, g = lane >> 4;
  f32x4 dcacc[CPT][NF];
#pragma unroll
  for (int it = 0; it < CPT; ++it)
#pragma unroll
    for (int b = 0; b < NF; ++b) dcacc[it][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb) {
  // ---- all global reads of the block, back to back (nothing is used before the last one is issued) ----
  SS_TM(8);
  const int row = rb * SS_ROWS + lrow;
  const bool active = row < p.B;
  const int64_t yraw = active ? p.y[row] : (int64_t)-1;
  uint4 qreg = make_uint4(0u, 0u, 0u, 0u);
  if (active && tr < TC) qreg = *reinterpret_cast<const uint4*>(p.Qb + (size_t)row * p.d + n0 + tr * 8);
  uint4 creg[CU];  // the C tile: loaded and parked in LDS by the first block only
  if (rb == 0) {
#pragma unroll
    for (int u = 0; u < CU; ++u) {
      const int q = tid + u * 1024, j = q / TC, cc = q % TC;
      creg[u] = make_uint4(0u, 0u, 0u, 0u);
      if (j < Nc) creg[u] = *reinterpret_cast<const uint4*>(p.Cb + (size_t)j * p.d + n0 + cc * 8);
    }
  }
  // partial-logit slabs (at most NS): every load is issued unconditionally on a valid address (absent slabs re-read
  // slab 0 and are dropped by a select at the add) -- a loop over p.splits would wait for one slab before asking for
  // the next: dependent trips to L2 instead of one
  float4 sa[CPT][NS], sb[CPT][NS];
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int chunk = tr + k * 32;
    const bool ok = active && chunk < cpr;
    const float* src = p.slabs + (ok ? (size_t)row * Nc + (size_t)chunk * 8 : (size_t)0);
#pragma unroll
    for (int z = 0; z < NS; ++z) {
      const float* sz = src + (z < p.splits ? (size_t)z * p.slab_stride : (size_t)0);
      sa[k][z] = *reinterpret_cast<const float4*>(sz);
      sb[k][z] = *reinterpret_cast<const float4*>(sz + 4);
    }
  }

  // ---- operand tiles -> LDS ----
  SS_TM(9);
  if (rb > 0) __syncthreads();  // the previous block's readers of Gs / Qs / red are done
  if (tr < TC) *reinterpret_cast<uint4*>(Qs + lrow * TS + tr * 8) = qreg;
  if (rb == 0) {
#pragma unroll
    for (int u = 0; u < CU; ++u) {
      const int q = tid + u * 1024, j = q / TC, cc = q % TC;
      if (j < ncp) *reinterpret_cast<uint4*>(Cs + j * TS + cc * 8) = creg[u];
    }
  }

  // ---- row softmax (32 lanes per row: DPP over 16, one lane exchange across the two halves), loss, G ----
  SS_TM(10);
  float v[CPT][8];
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    float4 a = sa[k][0], b = sb[k][0];
#pragma unroll
    for (int z = 1; z < NS; ++z) {
      const bool on = z < p.splits;
      a.x += on ? sa[k][z].x : 0.f; a.y += on ? sa[k][z].y : 0.f; a.z += on ? sa[k][z].z : 0.f; a.w += on ? sa[k][z].w : 0.f;
      b.x += on ? sb[k][z].x : 0.f; b.y += on ? sb[k][z].y : 0.f; b.z += on ? sb[k][z].z : 0.f; b.w += on ? sb[k][z].w : 0.f;
    }
    const bool ok = active && (tr + k * 32) < cpr;
    v[k][0] = ok ? a.x : -INFINITY; v[k][1] = ok ? a.y : -INFINITY; v[k][2] = ok ? a.z : -INFINITY; v[k][3] = ok ? a.w : -INFINITY;
    v[k][4] = ok ? b.x : -INFINITY; v[k][5] = ok ? b.y : -INFINITY; v[k][6] = ok ? b.z : -INFINITY; v[k][7] = ok ? b.w : -INFINITY;
  }
  SS_TM(11);
  const int yi = active ? (int)(yraw + p.y_offset) : -1;
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < CPT; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, v[k][e]);
  m = dprhot_row16_max(m);
  m = fmaxf(m, __shfl_xor(m, 16));
  float sm = 0.f, gold = 0.f;  // exactly one lane of the row holds the gold column
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int c0 = (tr + k * 32) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (yi == c0 + e) gold = v[k][e];
  }
  // every workgroup repeats this softmax, so its ALU time is on the critical path of the whole launch: ONE exponential
  // per score -- e = exp(v - max) feeds the row sum and, scaled by 1 / sum, the probabilities
  float ex[CPT][8];
  const bool dead = m == -INFINITY;  // a row with every column masked (the reference yields NaN there as well)
#pragma unroll
  for (int k = 0; k < CPT; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ex[k][e] = dead ? 0.f : __expf(v[k][e] - m);
      sm += ex[k][e];
    }
  sm = dprhot_row16_sum(sm);
  gold = dprhot_row16_sum(gold);
  sm += __shfl_xor(sm, 16);
  gold += __shfl_xor(gold, 16);
  const float lse = m + logf(sm);
  const float inv_sm = 1.0f / sm;  // sm = 0 (dead row): inf * 0 = NaN, like exp(v - lse) with lse = NaN
  if (tr == 0) {
    const float l = active ? lse - gold : 0.f;
    s_rl[rb * SS_ROWS + lrow] = l;
    if (lead && active) {
      if (p.row_lse) p.row_lse[row] = lse;
      if (p.row_loss) p.row_loss[row] = l;
    }
  }
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int chunk = tr + k * 32;
    if (chunk * 8 < ncp) {
      uint4 gv = make_uint4(0u, 0u, 0u, 0u);
      if (active && chunk < cpr) {
        const int c0 = chunk * 8;
        float gg[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float pr = ex[k][e] * inv_sm;
          if (c0 + e == yi) pr -= 1.0f;
          gg[e] = pr * p.grad_scale;
        }
        gv = make_uint4(pk_bf16(gg[0], gg[1]), pk_bf16(gg[2], gg[3]), pk_bf16(gg[4], gg[5]), pk_bf16(gg[6], gg[7]));
        if (lead) {
          if (p.G != nullptr) *reinterpret_cast<uint4*>(p.G + (size_t)row * Nc + c0) = gv;
          if (p.S_out != nullptr) {
            float* dst = p.S_out + (size_t)row * Nc + c0;
            *reinterpret_cast<float4*>(dst) = make_float4(v[k][0], v[k][1], v[k][2], v[k][3]);
            *reinterpret_cast<float4*>(dst + 4) = make_float4(v[k][4], v[k][5], v[k][6], v[k][7]);
          }
        }
      }
      *reinterpret_cast<uint4*>(Gs + lrow * gs + chunk * 8) = gv;
    }
  }
  SS_TM(12);
  __syncthreads();
  SS_TM(13);
  if constexpr (NRB == 1) {  // one block: the loss is complete here, summed under the GEMMs
    if (lead && tid == 0) {
      double tot = 0.0;
      for (int r = 0; r < p.B; ++r) tot += (double)s_rl[r];
      p.loss_sum[0] = (float)tot * p.loss_scale;
      s_rl[0] = (float)tot * p.loss_scale;  // (row losses are no longer needed) for the stamp below, read after the next barrier
    }
  }

  // ---- dQ[rows of the block, n0:n0+TW] = G[32, Nc] x C[Nc, TW]: wave w -> rows (w & 1) * 16.., K slice w >> 1 of 8; partial sums
  //      through LDS, added in slice order ----
  {
    const int wm = wave & 1, ks = wave >> 1;
    f32x4 acc[NF];
#pragma unroll
    for (int b = 0; b < NF; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < CPT; ++t) {  // ncp / 32 <= 8 * CPT K steps of 32
      const int kk = ks + t * 8;
      if (kk * 32 < ncp) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(Gs + (wm * 16 + i) * gs + kk * 32 + g * 8);
#pragma unroll
        for (int b = 0; b < NF; ++b) {
          const bf16x8 bfr = ss_tr_frag(Cs, TS, kk * 32, b * 16, lane);
          acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc[b], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < NF; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(ks * SS_ROWS + wm * 16 + g * 4 + r) * TW + b * 16 + i] = acc[b][r];
  }
  __syncthreads();
  // ---- dC_part[0:Nc, n0:n0+TW] += G^T[Nc, 32] x Q[32, TW]: one 16-row block of contexts per wave and round ----
  SS_TM(14);
  {
    bf16x8 bq[NF];
#pragma unroll
    for (int b = 0; b < NF; ++b) bq[b] = ss_tr_frag(Qs, TS, 0, b * 16, lane);
    if constexpr (NRB == 1) {  // one block: every 16-row block of contexts is stored as soon as it is multiplied
      const bool stamp = lead && p.stamp_period > 0;  // column 0 of d belongs to workgroup 0
      float* out = p.dC + (size_t)(wave * 16 + g * 4) * p.d + n0 + i;
      const size_t step = (size_t)256 * p.d;
#pragma unroll
      for (int it = 0; it < CPT; ++it) {  // Nc <= 256 * CPT rows, 256 per round of the sixteen waves
        const int j0 = wave * 16 + it * 256;
        if (j0 < Nc) {
          const bf16x8 af = ss_tr_frag(Gs, gs, 0, j0, lane);  // A(m = context j0 + i, k = query row) = G[k][m]
          f32x4 acc[NF];
#pragma unroll
          for (int b = 0; b < NF; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bq[b], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          float* o = out;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (j0 + g * 4 + r < Nc) {
#pragma unroll
              for (int b = 0; b < NF; ++b) {
                float vv = acc[b][r] * sc;
                if (b == 0 && i == 0 && stamp && (j0 + g * 4 + r) % p.stamp_period == p.stamp_row) vv = s_rl[0];
                o[b * 16] = vv;
              }
            }
            o += p.d;
          }
        }
        out += step;
      }
    } else {
#pragma unroll
      for (int it = 0; it < CPT; ++it) {
        const int j0 = wave * 16 + it * 256;
        if (j0 < Nc) {
          const bf16x8 af = ss_tr_frag(Gs, gs, 0, j0, lane);
#pragma unroll
          for (int b = 0; b < NF; ++b) dcacc[it][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bq[b], dcacc[it][b], 0, 0, 0);
        }
      }
    }
  }
  // dQ of the block: add the 8 K slices in order
  for (int e = tid; e < SS_ROWS * TW; e += 1024) {
    const int r = e / TW, ccol = e - r * TW;
    if (rb * SS_ROWS + r < p.B) {
      float s = red[e];
#pragma unroll
      for (int k = 1; k < 8; ++k) s += red[k * SS_ROWS * TW + e];
      p.dQ[(size_t)(rb * SS_ROWS + r) * p.d + n0 + ccol] = s * sc;
    }
  }
  }  // row blocks

  if constexpr (NRB > 1) {
  __syncthreads();  // every block's row losses are in s_rl (and red is free)
  if (lead && tid == 0) {
    double tot = 0.0;
    for (int r = 0; r < p.B; ++r) tot += (double)s_rl[r];
    p.loss_sum[0] = (float)tot * p.loss_scale;
    red[0] = (float)tot * p.loss_scale;  // for the stamp below
  }
  {
    const bool stamp = lead && p.stamp_period > 0;  // column 0 of d belongs to workgroup 0
    float lsum = 0.f;
    if (stamp) {  // workgroup-uniform
      __syncthreads();
      lsum = red[0];
    }
    float* out = p.dC + (size_t)(wave * 16 + g * 4) * p.d + n0 + i;
    const size_t step = (size_t)256 * p.d;
#pragma unroll
    for (int it = 0; it < CPT; ++it) {
      const int j0 = wave * 16 + it * 256;
      if (j0 < Nc) {
        float* o = out;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (j0 + g * 4 + r < Nc) {
#pragma unroll
            for (int b = 0; b < NF; ++b) {
              float vv = dcacc[it][b][r] * sc;
              if (b == 0 && i == 0 && stamp && (j0 + g * 4 + r) % p.stamp_period == p.stamp_row) vv = lsum;
              o[b * 16] = vv;
            }
          }
          o += p.d;
        }
      }
      out += step;
    }
  }
  }  // NRB > 1
  SS_TM(15);
}

// ---- the same launch split by role (option small_step_roles; B <= 32, Nc <= 768) ------------------------------------------------
// dQ of rows 0-15 never touches the softmax of rows 16-31, dC needs neither the C tile nor the dQ slice buffer, and 48 workgroups
// leave 208 CUs idle: one grid, blockIdx.x picks the role.
//   dC role, d / 16 blocks (first to start):        slabs + Q tile, the full softmax, G image, ONE barrier, dC product and stores.
//   dQ role, one block per (16-row half, QTW columns): its 16 rows of the slabs (waves 0-7: 32 lanes per row, as ever) while waves
//                                                   8-15 fetch the C tile; G half image, dQ product in 8 K slices, slice sum, store.
//   who writes loss / logsumexp / G / logits:       step_small_kernel_roles (forms 1, 2): the dC workgroup of tile 0, the lead, as in
//                                                   step_small_kernel -- and it ended the launch 0.36 us behind the other 47.
//                                                   step_small_kernel_out (form 3): output workgroups of the same grid that have
//                                                   no product to do -- a loss block and two row-store blocks (ss_role_loss,
//                                                   ss_role_rows); every dC workgroup is a plain one.
// No role waits on memory in front of its operand loads: the device-side scale, used behind the products only, is the LAST load of a
// role's batch (tests/test_step_fronts.py reads that off the assembly).
// Every value is formed by the arithmetic instructions of step_small_kernel in their order -- the softmax below is its text without
// the selects, compares, address arithmetic and LDS lane exchanges that change no value -- so the outputs are the same bits, and
// step_small_kernel, which is left exactly as it was, is the reference they are compared with (tests/test_small_step_roles.py,
// tests/test_small_step_out.py, tests/test_small_step_lean.py, tests/test_small_step_split_gpu.py).
inline size_t step_roles_lds(int Nc, int QTW) {
  const int ncp = (Nc + 31) / 32 * 32, gs = ncp + 8;
  const size_t dc = (size_t)SS_ROWS * gs * 2 + (size_t)SS_ROWS * 24 * 2 + SS_MAXB * sizeof(float);
  const size_t dq = (size_t)16 * gs * 2 + (size_t)ncp * (QTW + 8) * 2 + (size_t)8 * 16 * QTW * sizeof(float);
  const size_t out = SS_ROWS * sizeof(float);  // the output role keeps the row losses only (never the largest of the three)
  const size_t m = dc > dq ? dc : dq;
  return m > out ? m : out;
}

// The row softmax of step_small_kernel for the thread's 8 * CPT scores of `row` (32 lanes per row): slabs added in slab order, one
// exponential per score, G (bf16) into row `lrow` of the LDS image.  Returns the row loss (lane tr == 0 uses it).
// MODE (compile-time) takes whole parts of the text out for the blocks of form 3 that nobody reads an image from: SS_SM_ROWS drops the
// LDS store of G and the two per-row stores and nothing else (the values are formed all the same for the global stores); SS_SM_LOSS
// stops at the row loss.  What remains forms its values exactly as the full text does.
// Every workgroup of the launch repeats this text on four SIMDs, so its VALU instructions ARE the launch's critical path.  It forms
// every value with the arithmetic instructions of step_small_kernel, in their order, and spends nothing else ("the lean
// row softmax"):
//   NS is the number of slabs, by contract with the launcher (NS == max(splits, 1)): no run-time `z < p.splits` select at the add.
//   FULL (B == 32 and Nc == 256 * CPT, compile-time): every row and every chunk is there -- no -inf select, no guard, no zero fill.
//   A dead row takes one select on the subtrahend (exp(-inf - 0) = +0, what the select on the result gave), not one per score.
//   The gold column is the element dg = yi - c0 of the thread's chunk, a compare against a constant per element.
//   The two 16-lane halves of a row meet through v_permlane16_swap, not through LDS (ss_pair16).

// x of lanes l and l ^ 16, side by side in every lane.  v_permlane16_swap with D = S = x exchanges the odd 16-lane rows of D with the
// even rows of S: afterwards r[0] = x[l & ~16] and r[1] = x[l | 16] in EVERY lane l.  Here a query row is 32 lanes (tr = tid & 31:
// lanes 0-31 of a wave are row 2w, lanes 32-63 row 2w + 1), so lanes tr and tr ^ 16 -- the two DPP rows of ONE query row -- meet, and
// the two query rows of the wave never mix.  Lanes 0-15 / 32-47 combine (own, other) as __shfl_xor(x, 16) had them, lanes 16-31 /
// 48-63 (other, own): max and a two-term sum are commutative, so all 32 lanes of the row hold the bits they held before.  (The one
// non-commutative case of v_max_f32 is max(+0, -0): the sign of a zero row maximum reaches no output -- exp(+-0) = 1, and
// lse = m + log(sum) with sum >= 1 has log(sum) >= +0, which absorbs it.)
__device__ __forceinline__ void ss_pair16(float x, float& even, float& odd) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  even = __uint_as_float(r[0]);
  odd = __uint_as_float(r[1]);
}

// The row maximum over the 32 lanes of a query row, as ONE asm statement: four DPP row rotations (8, 4, 2, 1) inside each 16-lane half,
// then the two halves through v_permlane16_swap.  dprhot_row16_max + ss_pair16 + fmaxf form the same values, but fmaxf on a DPP or
// swap result makes hipcc put a canonicalising v_max_f32 x, x, x (and a v_mov_b32_dpp) in front of every v_max_f32: 17 vector
// instructions where 7 do (profiles/valu_issue_probe.txt: 9.9 against 3.0 cycles per SIMD and rotation step at four waves per SIMD).
// The canonicalisation only quiets a signalling NaN, and x is never any NaN here: the thread's maximum starts from -inf, and
// v_max3_f32 returns a number when one operand is one.  v_max_f32 of two numbers is their maximum whichever operand comes first (the
// DPP operand has to be src0); its one order-dependent case is max(+0, -0), see ss_pair16.
// Wait states (inside the string, the hazard recognizer does not look into it): a DPP read and a v_permlane read each need two behind
// the VALU write of their operand -- s_nop 1 in front of every rotation (the first covers the instruction that formed x) and of the swap.
// NOT covered: a VALU write of EXEC (v_cmpx) needs five wait states before a DPP read, and an SGPR written by v_readlane /
// v_readfirstlane is no operand here -- the kernels of this file have no v_cmpx; do not call this directly behind one.
// The no-NaN argument holds for any NS: with NS >= 2 the scores are sums (an arithmetic result is never a signalling NaN), and with
// NS == 1 they are the words the sim launch stored, arithmetic results as well; hipcc canonicalises such loaded words in front of
// v_max3_f32 itself.  A caller that feeds this softmax slabs from elsewhere has to check that again.
__device__ __forceinline__ float ss_row32_max(float x) {
  float t;
  asm("s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_mov_b32 %1, %0\n\t"
      "s_nop 1\n\t"
      "v_permlane16_swap_b32 %0, %1\n\t"  // %0 = x of the row's lanes 0-15, %1 = of its lanes 16-31, in every lane (ss_pair16)
      "v_max_f32 %0, %0, %1"
      : "+v"(x), "=&v"(t));
  return x;
}

typedef float ss_f32x2 __attribute__((ext_vector_type(2)));

constexpr int SS_SM_IMAGE = 0;  // dC / dQ roles: G into the LDS image; `lead` (forms 1, 2) also stores every output
constexpr int SS_SM_LOSS = 1;   // loss block (form 3): logsumexp and row loss only -- no G arithmetic, no G or logits store, no image
constexpr int SS_SM_ROWS = 2;   // row-store blocks (form 3): G and the logits to memory only -- no image, no logsumexp / row-loss store
// Issue cycles ("the priced row softmax"; prices: profiles/valu_issue_probe.txt).  At four waves per SIMD a packed fp32
// instruction costs what any other vector instruction does (3.0 cycles per SIMD) and forms two values, so the element-wise parts
// -- slab sums, v - m0, * log2(e), e * (1 / sum) and * grad_scale -- are written on two-element vectors: v_pk_add_f32 / v_pk_mul_f32 /
// v_pk_fma_f32 are the same IEEE operation on each half, in the order of the scalar text.  The row maximum is ss_row32_max.  The probability is
// fma(e, 1 / sum, addend) with addend -1 at the gold element (the contracted `e * inv - 1` of step_small_kernel) and -0 elsewhere:
// e * inv is +0 or greater, or NaN, and x + (-0) = x for each of those, so the fma rounds the product as the multiplication did --
// the select acts on eight constants, ahead of the slabs' arrival, and not on eight pairs of results behind the division.
template <int CPT, int NS, bool FULL, int MODE = SS_SM_IMAGE>
__device__ __forceinline__ float ss_row_softmax(const StepSmallArgs& p, float4 (&sa)[CPT][NS], float4 (&sb)[CPT][NS], int row, bool active,
                                                int64_t yraw, int tr, bool lead, uint16_t* Gs_row, int ncp) {
  const int Nc = FULL ? 256 * CPT : p.Nc, cpr = Nc >> 3;
  const int yi = FULL || active ? (int)(yraw + p.y_offset) : -1;
  unsigned dg[CPT];  // the gold column is element dg of the thread's chunk k (dg < 8 in one lane of the row and nowhere else; yi = -1 matches nothing)
  ss_f32x2 addend[CPT][4];
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    dg[k] = (unsigned)yi - (unsigned)((tr + k * 32) * 8);
    if constexpr (MODE != SS_SM_LOSS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) addend[k][j] = ss_f32x2{dg[k] == (unsigned)(2 * j) ? -1.0f : -0.0f, dg[k] == (unsigned)(2 * j + 1) ? -1.0f : -0.0f};
      // (an empty statement that ties the addends to the chunk of the first slab: the label arrives ahead of the slabs, and the
      // selects are to issue while the SIMD waits for them, not among the sums or behind the division where hipcc would sink them.
      // Not where the slabs in flight and the addends together would not fit the 128 registers of a 1024-thread workgroup -- three
      // chunks of four slabs: there the addends are formed where hipcc likes, with nothing spilled)
      if constexpr (CPT * (NS + 1) * 8 <= 96)
        asm("" : "+v"(addend[k][0]), "+v"(addend[k][1]), "+v"(addend[k][2]), "+v"(addend[k][3]), "+v"(sa[k][0].x), "+v"(sa[k][0].y),
            "+v"(sa[k][0].z), "+v"(sa[k][0].w), "+v"(sb[k][0].x), "+v"(sb[k][0].y), "+v"(sb[k][0].z), "+v"(sb[k][0].w));
    }
  }
  ss_f32x2 v[CPT][4];  // elements 2 j, 2 j + 1 of chunk k
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    v[k][0] = ss_f32x2{sa[k][0].x, sa[k][0].y}; v[k][1] = ss_f32x2{sa[k][0].z, sa[k][0].w};
    v[k][2] = ss_f32x2{sb[k][0].x, sb[k][0].y}; v[k][3] = ss_f32x2{sb[k][0].z, sb[k][0].w};
#pragma unroll
    for (int z = 1; z < NS; ++z) {  // slab order 0, 1, 2, 3
      v[k][0] += ss_f32x2{sa[k][z].x, sa[k][z].y}; v[k][1] += ss_f32x2{sa[k][z].z, sa[k][z].w};
      v[k][2] += ss_f32x2{sb[k][z].x, sb[k][z].y}; v[k][3] += ss_f32x2{sb[k][z].z, sb[k][z].w};
    }
    if constexpr (!FULL) {
      const bool ok = active && (tr + k * 32) < cpr;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[k][j] = ss_f32x2{ok ? v[k][j][0] : -INFINITY, ok ? v[k][j][1] : -INFINITY};
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < CPT; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, v[k][e >> 1][e & 1]);
  m = ss_row32_max(m);
  float gold = 0.f;  // exactly one lane of the row holds the gold column
#pragma unroll
  for (int k = 0; k < CPT; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (dg[k] == (unsigned)e) gold = v[k][e >> 1][e & 1];
  float ex[CPT][8];
  const bool dead = m == -INFINITY;  // a row with every column masked (the reference yields NaN there as well)
  const float m0 = dead ? 0.f : m;   // every score of a dead row is -inf: exp(-inf - 0) = +0
  const ss_f32x2 m2 = {m0, m0}, log2e = {0x1.715476p+0f, 0x1.715476p+0f};  // __expf(x) = exp2(log2(e) * x), the constant of the HIP header
#pragma unroll
  for (int k = 0; k < CPT; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const ss_f32x2 t = log2e * (v[k][j] - m2);
      ex[k][2 * j] = __builtin_amdgcn_exp2f(t[0]);
      ex[k][2 * j + 1] = __builtin_amdgcn_exp2f(t[1]);
    }
  float sm = 0.f + ex[0][0];  // (as step_small_kernel has it; starting from ex[0][0] is exact and measured no gain: scratch/negative/README.md)
#pragma unroll
  for (int k = 0; k < CPT; ++k)
#pragma unroll
    for (int e = (k == 0 ? 1 : 0); e < 8; ++e) sm += ex[k][e];
  sm = dprhot_row16_sum(sm);
  gold = dprhot_row16_sum(gold);
  float even, odd;
  ss_pair16(sm, even, odd);
  sm = even + odd;
  ss_pair16(gold, even, odd);
  gold = even + odd;
  const float lse = m + logf(sm);
  const float inv_sm = 1.0f / sm;  // sm = 0 (dead row): inf * 0 = NaN, like exp(v - lse) with lse = NaN
  const float l = FULL || active ? lse - gold : 0.f;
  if constexpr (MODE != SS_SM_ROWS) {
    if (tr == 0 && lead && (FULL || active)) {
      if (p.row_lse) p.row_lse[row] = lse;
      if (p.row_loss) p.row_loss[row] = l;
    }
  }
  if constexpr (MODE != SS_SM_LOSS) {  // (compiled out, not masked: the loss needs no probability)
  const ss_f32x2 inv2 = {inv_sm, inv_sm}, gs2 = {p.grad_scale, p.grad_scale};
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int chunk = tr + k * 32;
    if (FULL || chunk * 8 < ncp) {
      uint4 gv = make_uint4(0u, 0u, 0u, 0u);
      if (FULL || (active && chunk < cpr)) {
        const int c0 = chunk * 8;
        uint32_t gw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const ss_f32x2 pr = __builtin_elementwise_fma(ss_f32x2{ex[k][2 * j], ex[k][2 * j + 1]}, inv2, addend[k][j]);
          const ss_f32x2 gg = pr * gs2;
          gw[j] = pk_bf16(gg[0], gg[1]);
        }
        gv = make_uint4(gw[0], gw[1], gw[2], gw[3]);
        if (lead) {
          if (p.G != nullptr) *reinterpret_cast<uint4*>(p.G + (size_t)row * Nc + c0) = gv;
          if (p.S_out != nullptr) {
            float* dst = p.S_out + (size_t)row * Nc + c0;
            *reinterpret_cast<float4*>(dst) = make_float4(v[k][0][0], v[k][0][1], v[k][1][0], v[k][1][1]);
            *reinterpret_cast<float4*>(dst + 4) = make_float4(v[k][2][0], v[k][2][1], v[k][3][0], v[k][3][1]);
          }
        }
      }
      if constexpr (MODE == SS_SM_IMAGE) *reinterpret_cast<uint4*>(Gs_row + chunk * 8) = gv;
    }
  }
  }
  return l;
}

// the thread's chunks of all NS slabs, issued back to back: slab z is one base plus z uniform strides
template <int CPT, int NS, bool FULL>
__device__ __forceinline__ void ss_load_slabs(const StepSmallArgs& p, float4 (&sa)[CPT][NS], float4 (&sb)[CPT][NS], int row, bool active, int tr) {
  const int Nc = FULL ? 256 * CPT : p.Nc, cpr = Nc >> 3;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int chunk = tr + k * 32;
    const bool ok = FULL || (active && chunk < cpr);  // (an absent chunk re-reads the first one and is dropped by the softmax)
    const float* src = p.slabs + (ok ? (size_t)row * Nc + (size_t)chunk * 8 : (size_t)0);
#pragma unroll
    for (int z = 0; z < NS; ++z) {
      const float* sz = src + (size_t)z * p.slab_stride;
      sa[k][z] = *reinterpret_cast<const float4*>(sz);
      sb[k][z] = *reinterpret_cast<const float4*>(sz + 4);
    }
  }
}

// ---- the role bodies (step_small_kernel_roles and step_small_kernel_out call the same text) ----

// dC role: dC_part[0:Nc, n0:n0+16] = G^T x Q[:, n0:n0+16] for column tile `tile`.  LEAD: the workgroup of tile 0 also writes the
// loss / logsumexp / G / logits and, in the stamping launch of the packed step, the loss into its column 0 of dC (forms 1, 2);
// false: no workgroup of this role does (form 3).
// FULL (every role): B == 32 and Nc == 256 * CPT, known at compile time -- see ss_row_softmax.
template <int CPT, int NS, bool LEAD, bool FULL>
__device__ __forceinline__ void ss_role_dc(const StepSmallArgs& p, uint16_t* Gs, int tile) {  // Gs: [32][gs]  G, row-major
  constexpr int TW = 16, TS = TW + 8, TC = TW / 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Nc = FULL ? 256 * CPT : p.Nc, B = FULL ? SS_ROWS : p.B;
  const int ncp = (Nc + 31) / 32 * 32, gs = ncp + 8;
  DPRHOT_TMB(1, 0);
  const int lrow = tid >> 5, tr = tid & 31;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = tile * TW;
  const bool lead = LEAD && tile == 0;
  uint16_t* const Qs = Gs + SS_ROWS * gs;                           // [32][TS]  Q[:, n0:n0+16]
  float* const s_rl = reinterpret_cast<float*>(Qs + SS_ROWS * TS);  // [32] row losses
  const int row = lrow;
  const bool active = FULL || row < B;
  const int64_t yraw = active ? p.y[row] : (int64_t)-1;
  uint4 qreg = make_uint4(0u, 0u, 0u, 0u);
  if (active && tr < TC) qreg = *reinterpret_cast<const uint4*>(p.Qb + (size_t)row * p.d + n0 + tr * 8);
  float4 sa[CPT][NS], sb[CPT][NS];
  ss_load_slabs<CPT, NS, FULL>(p, sa, sb, row, active, tr);
  // The device-side scale is used behind the product only.  Read at the top under `p.d_scale ? ... : 1.0f` it was a load and a wait
  // of its own -- a whole trip to memory -- in front of every load above; here it is ONE unconditional load (of a slab word where
  // there is no scale, dropped by the select at the use), the last of the batch, and nothing in front of the barrier waits for it.
  const float dsv = *(p.d_scale ? p.d_scale : p.slabs);
  DPRHOT_TMB(1, 1);
  if (tr < TC) *reinterpret_cast<uint4*>(Qs + lrow * TS + tr * 8) = qreg;
  const float l = ss_row_softmax<CPT, NS, FULL>(p, sa, sb, row, active, yraw, tr, lead, Gs + lrow * gs, ncp);
  if constexpr (LEAD) {
    if (tr == 0) s_rl[lrow] = l;
  }
  DPRHOT_TMB(1, 2);
  __syncthreads();
  DPRHOT_TMB(1, 3);
  const bool stamp = lead && p.stamp_period > 0;  // column 0 of d belongs to the lead
  if (lead) {                                     // workgroup-uniform
    if (tid == 0) {
      double tot = 0.0;
      for (int r = 0; r < B; ++r) tot += (double)s_rl[r];
      p.loss_sum[0] = (float)tot * p.loss_scale;
      s_rl[0] = (float)tot * p.loss_scale;  // (row losses are no longer needed) for the stamp below
    }
    if (stamp) __syncthreads();  // only the stamping launch of the packed step pays this second barrier
  }
  const float sc = p.h_scale * (p.d_scale ? dsv : 1.0f);
  const bf16x8 bq = ss_tr_frag(Qs, TS, 0, 0, lane);
  float* out = p.dC + (size_t)(wave * 16 + g * 4) * p.d + n0 + i;
  const size_t step = (size_t)256 * p.d;
#pragma unroll
  for (int it = 0; it < CPT; ++it) {  // Nc <= 256 * CPT rows, 256 per round of the sixteen waves
    const int j0 = wave * 16 + it * 256;
    if (j0 < Nc) {
      const bf16x8 af = ss_tr_frag(Gs, gs, 0, j0, lane);  // A(m = context j0 + i, k = query row) = G[k][m]
      const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bq, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      float* o = out;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (j0 + g * 4 + r < Nc) {
          float vv = acc[r] * sc;
          if (i == 0 && stamp && (j0 + g * 4 + r) % p.stamp_period == p.stamp_row) vv = s_rl[0];
          o[0] = vv;
        }
        o += p.d;
      }
    }
    out += step;
  }
  DPRHOT_TMB(1, 4);
}

// dQ role: dQ[r0:r0+16, n0:n0+QTW] = G[r0:r0+16, :] x C[:, n0:n0+QTW] for column tile qt and 16-row half `half`
template <int CPT, int NS, int QTW, bool FULL>
__device__ __forceinline__ void ss_role_dq(const StepSmallArgs& p, uint16_t* Gs, int qt, int half) {  // Gs: [16][gs]  G, row-major
  constexpr int QTS = QTW + 8, QTC = QTW / 8, NF = QTW / 16;
  constexpr int CUQ = (256 * CPT * QTC + 511) / 512;  // C-tile chunks per thread of waves 8-15
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Nc = FULL ? 256 * CPT : p.Nc, B = FULL ? SS_ROWS : p.B;
  const int ncp = (Nc + 31) / 32 * 32, gs = ncp + 8;
  DPRHOT_TMB(2, 0);
  const int lrow = tid >> 5, tr = tid & 31;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = qt * QTW, r0 = half * 16;
  if (r0 >= B) return;  // (fewer rows than one half: nothing of dQ is this block's to write)
  uint16_t* const Cs = Gs + 16 * gs;                             // [ncp][QTS]  C[:, n0:n0+QTW]
  float* const red = reinterpret_cast<float*>(Cs + ncp * QTS);   // [8][16][QTW] dQ partial sums
  float dsv = 1.0f;  // the device-side scale, as in ss_role_dc: the last load of the batch (the slice sum is threads 0 .. 16 QTW - 1 <= 511)
  if (tid < 512) {  // waves 0-7: the softmax of the half's 16 rows
    const int row = r0 + lrow;
    const bool active = FULL || row < B;
    const int64_t yraw = active ? p.y[row] : (int64_t)-1;
    float4 sa[CPT][NS], sb[CPT][NS];
    ss_load_slabs<CPT, NS, FULL>(p, sa, sb, row, active, tr);
    dsv = *(p.d_scale ? p.d_scale : p.slabs);
    DPRHOT_TMB(2, 1);
    (void)ss_row_softmax<CPT, NS, FULL>(p, sa, sb, row, active, yraw, tr, false, Gs + lrow * gs, ncp);
  } else {  // waves 8-15: the C tile
    const int t2 = tid - 512;
    uint4 creg[CUQ];
#pragma unroll
    for (int c = 0; c < CUQ; ++c) {
      const int q = t2 + c * 512, j = q / QTC, cc = q % QTC;
      creg[c] = make_uint4(0u, 0u, 0u, 0u);
      if (j < Nc) creg[c] = *reinterpret_cast<const uint4*>(p.Cb + (size_t)j * p.d + n0 + cc * 8);
    }
#pragma unroll
    for (int c = 0; c < CUQ; ++c) {
      const int q = t2 + c * 512, j = q / QTC, cc = q % QTC;
      if (j < ncp) *reinterpret_cast<uint4*>(Cs + j * QTS + cc * 8) = creg[c];
    }
  }
  DPRHOT_TMB(2, 2);
  __syncthreads();
  DPRHOT_TMB(2, 3);
  {
    // K slice ks of 8 (kk = ks + 8 t, ascending t); QTW = 32: the wave pair of a slice takes one 16-column fragment each
    const int ks = NF == 2 ? wave >> 1 : wave, b = NF == 2 ? wave & 1 : 0;
    if (ks < 8) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < CPT; ++t) {
        const int kk = ks + t * 8;
        if (kk * 32 < ncp) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(Gs + i * gs + kk * 32 + g * 8);
          const bf16x8 bfr = ss_tr_frag(Cs, QTS, kk * 32, b * 16, lane);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(ks * 16 + g * 4 + r) * QTW + b * 16 + i] = acc[r];
    }
  }
  __syncthreads();
  DPRHOT_TMB(2, 4);
  if (tid < 16 * QTW) {  // add the 8 K slices in order
    const float sc = p.h_scale * (p.d_scale ? dsv : 1.0f);
    const int e = tid, r = e / QTW, ccol = e - r * QTW;
    if (r0 + r < B) {
      float s = red[e];
#pragma unroll
      for (int k = 1; k < 8; ++k) s += red[k * 16 * QTW + e];
      p.dQ[(size_t)(r0 + r) * p.d + n0 + ccol] = s * sc;
    }
  }
  DPRHOT_TMB(2, 5);
}

// The output roles (form 3): what the lead did besides its dC tile, and nothing else.  No Q tile, no C tile, no product, and no G
// image in LDS.  One workgroup did all of it at first and ended the launch (2.40 us against 2.28 for the last dC workgroup): the
// full softmax with every store on four waves per SIMD, then a barrier, then the loss.  But the loss needs every row's statistics
// and neither G nor the logits, and the per-row outputs need no barrier and split by rows -- so they are two roles:
//   loss block (one):       the softmax of all 32 rows up to the row loss (SS_SM_LOSS), logsumexp and row loss stored, ONE barrier,
//                           the sum.
//   row-store blocks (two): one 16-row half each on waves 0-7, as in the dQ role; G and the logits stored (SS_SM_ROWS), no barrier.
// Each forms its values with the shared softmax text: the same bits as the lead's.
template <int CPT, int NS, bool FULL>
__device__ __forceinline__ void ss_role_loss(const StepSmallArgs& p, float* s_rl) {  // s_rl: [32] row losses
  const int tid = threadIdx.x, lane = tid & 63;
  DPRHOT_TMB(3, 0);
  const int Nc = FULL ? 256 * CPT : p.Nc, B = FULL ? SS_ROWS : p.B;
  const int ncp = (Nc + 31) / 32 * 32;
  const int lrow = tid >> 5, tr = tid & 31;
  const int row = lrow;
  const bool active = FULL || row < B;
  const int64_t yraw = p.y[active ? row : 0];  // (unconditional, on a valid address: the softmax drops the label of an absent row)
  float4 sa[CPT][NS], sb[CPT][NS];
  ss_load_slabs<CPT, NS, FULL>(p, sa, sb, row, active, tr);
  DPRHOT_TMB(3, 1);
  const float l = ss_row_softmax<CPT, NS, FULL, SS_SM_LOSS>(p, sa, sb, row, active, yraw, tr, true, nullptr, ncp);
  if (tr == 0) s_rl[lrow] = l;
  DPRHOT_TMB(3, 2);
  __syncthreads();
  DPRHOT_TMB(3, 3);
  if (tid < 64) {  // wave 0
    // The loss: double accumulator, rows 0 .. B-1 in ascending order, as the lead's walk over s_rl added them -- but that walk was B
    // dependent trips to LDS (read, convert, add, next address).  ONE read, lane r holding row r and widening it (exact), then the
    // lane reads -- none depends on the sum, and the guard r < B is a select, not a branch (32 scalar branches in a row cost 0.5 us)
    // -- and the same B additions in the same order out of registers.  A row beyond B contributes a +0.0 that changes no bit: the
    // sum starts at +0.0 and an addition in round-to-nearest never yields -0.0 from there.
    const double mine = (double)s_rl[lane & (SS_ROWS - 1)];
    const int mlo = __double2loint(mine), mhi = __double2hiint(mine);
    double x[SS_ROWS];
#pragma unroll
    for (int r = 0; r < SS_ROWS; ++r) {
      const double xr = __hiloint2double(__builtin_amdgcn_readlane(mhi, r), __builtin_amdgcn_readlane(mlo, r));
      x[r] = r < B ? xr : 0.0;
    }
    double tot = 0.0;
#pragma unroll
    for (int r = 0; r < SS_ROWS; ++r) tot += x[r];
    if (tid == 0) p.loss_sum[0] = (float)tot * p.loss_scale;
  }
  DPRHOT_TMB(3, 4);
}

// row-store block of 16-row half `half`: G and the logits of its rows, nothing else
template <int CPT, int NS, bool FULL>
__device__ __forceinline__ void ss_role_rows(const StepSmallArgs& p, int half) {
  const int tid = threadIdx.x;
  DPRHOT_TMB(0, 0);
  const int Nc = FULL ? 256 * CPT : p.Nc, B = FULL ? SS_ROWS : p.B;
  const int ncp = (Nc + 31) / 32 * 32;
  const int lrow = tid >> 5, tr = tid & 31;
  const int r0 = half * 16;
  // waves 8-15 have no row; a half without a row and a step that asks for neither output have nothing to store (no barrier below)
  if (tid >= 512 || r0 >= B || (p.G == nullptr && p.S_out == nullptr)) return;
  const int row = r0 + lrow;
  const bool active = FULL || row < B;
  const int64_t yraw = p.y[active ? row : 0];  // (as in ss_role_loss)
  float4 sa[CPT][NS], sb[CPT][NS];
  ss_load_slabs<CPT, NS, FULL>(p, sa, sb, row, active, tr);
  DPRHOT_TMB(0, 1);
  (void)ss_row_softmax<CPT, NS, FULL, SS_SM_ROWS>(p, sa, sb, row, active, yraw, tr, true, nullptr, ncp);
  DPRHOT_TMB(0, 2);
}

// CPT, NS: as in step_small_kernel (CPT <= 3).  QTW: columns of d per dQ workgroup (16 or 32; d % QTW == 0).
// Grid: d / 16 dC blocks, then 2 * d / QTW dQ blocks.
template <int CPT, int NS, int QTW, bool FULL>
__device__ __forceinline__ void ss_roles_block(const StepSmallArgs& p, uint16_t* smem) {
  const int ndc = p.d / 16;  // dC blocks
  if ((int)blockIdx.x < ndc) {
    // the XCD-aware tile mapping of step_small_kernel (linear ids are dealt round-robin to the 8 XCDs)
    const int tile = (ndc % 8 == 0) ? ((int)blockIdx.x % 8) * (ndc / 8) + (int)blockIdx.x / 8 : (int)blockIdx.x;
    ss_role_dc<CPT, NS, true, FULL>(p, smem, tile);
    return;
  }
  const int u = (int)blockIdx.x - ndc, nqt = p.d / QTW;
  // both halves of a tile, and the tiles that share the 128-byte lines of C rows, in the XCD of the dC blocks of the same columns
  int qt, half;
  if (ndc % 8 == 0 && nqt % 8 == 0) {
    const int per = nqt / 8;
    qt = (u % 8) * per + (u / 8) % per;
    half = (u / 8) / per;
  } else {
    qt = u % nqt;
    half = u / nqt;
  }
  ss_role_dq<CPT, NS, QTW, FULL>(p, smem, qt, half);
}
// FULL is chosen HERE, from the arguments the role bodies index with, by one workgroup-uniform scalar branch: a kernel cannot be
// launched with a flag that its B and Nc do not bear out, and the launcher keeps one instantiation per (CPT, NS, QTW).
template <int CPT, int NS, int QTW>
__global__ __launch_bounds__(1024) void step_small_kernel_roles(StepSmallArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint16_t ss_smem[];
  if (p.B == SS_ROWS && p.Nc == 256 * CPT) ss_roles_block<CPT, NS, QTW, true>(p, ss_smem);
  else ss_roles_block<CPT, NS, QTW, false>(p, ss_smem);
}

// Form 3.  Grid: the loss block, the two row-store blocks, then d / 16 dC blocks, then 2 * d / QTW dQ blocks (SS_OUT_BLOCKS = 3 in
// front of the products).
// The output blocks are the physical blocks 0-2.  Workgroups are handed out in index order, and the roles kernel's stamps show what
// a late index costs: its dQ blocks, behind the 48 dC blocks, take their first stamp 0.2-0.3 us after block 0 does.  The loss block
// carries a full 32-row softmax and then a barrier and the loss, so it has to be the first to start, not behind 96 others; being
// in front costs every other block three places in the queue and nothing else (99 of 256 CUs are taken).  They land in XCDs 0-2.
// Block index b -> XCD is b % 8, so the tile mappings below are computed from the physical index b: the blocks of one role are a
// run of consecutive indices [first, first + n), those of XCD b % 8 among them are 8 apart, so (b - first) / 8 counts them, and with
// n / 8 blocks per XCD, XCD x owns the same contiguous run of column tiles in both roles -- the neighbouring tiles of one 128-byte
// line of Q / C rows still meet in one L2 -- and every tile has exactly one owner.
constexpr int SS_OUT_BLOCKS = 3;
template <int CPT, int NS, int QTW, bool FULL>
__device__ __forceinline__ void ss_out_block(const StepSmallArgs& p, uint16_t* smem) {
  const int b = (int)blockIdx.x;
  if (b == 0) {
    ss_role_loss<CPT, NS, FULL>(p, reinterpret_cast<float*>(smem));
    return;
  }
  if (b < SS_OUT_BLOCKS) {
    ss_role_rows<CPT, NS, FULL>(p, b - 1);
    return;
  }
  const int ndc = p.d / 16, nqt = p.d / QTW;
  if (b < SS_OUT_BLOCKS + ndc) {
    const int v = b - SS_OUT_BLOCKS;
    const int tile = (ndc % 8 == 0) ? (b % 8) * (ndc / 8) + v / 8 : v;
    ss_role_dc<CPT, NS, false, FULL>(p, smem, tile);
    return;
  }
  const int u = b - SS_OUT_BLOCKS - ndc;
  int qt, half;
  if (ndc % 8 == 0 && nqt % 8 == 0) {  // u / 8 counts the dQ blocks of XCD b % 8: per tiles, both halves of each
    const int per = nqt / 8;
    qt = (b % 8) * per + (u / 8) % per;
    half = (u / 8) / per;
  } else {
    qt = u % nqt;
    half = u / nqt;
  }
  ss_role_dq<CPT, NS, QTW, FULL>(p, smem, qt, half);
}
template <int CPT, int NS, int QTW>
__global__ __launch_bounds__(1024) void step_small_kernel_out(StepSmallArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint16_t ss_smem[];
  if (p.B == SS_ROWS && p.Nc == 256 * CPT) ss_out_block<CPT, NS, QTW, true>(p, ss_smem);  // (FULL: see step_small_kernel_roles)
  else ss_out_block<CPT, NS, QTW, false>(p, ss_smem);
}

}  // namespace dprhot
