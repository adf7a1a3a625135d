// spar.h -- SPAR retrieval: the weighted score of two resident indexes for a whole grid of weights,
//
//   s[w][i][j] = fmaf(lam[w], acc2[i][j], acc1[i][j]),   acc1 = <Q1[i], C1[j]> over d1,   acc2 = <Q2[i], C2[j]> over d2
//
// ONE fp32 fma per score.  The reference (spar_retrieval.py:153-182) concatenates the two corpora and multiplies the weight into the
// query half: a second copy of both indexes, and on bf16 operands a weight rounded into 8 bits of significand.  Here the two
// contractions run back to back into two accumulator sets and the weight meets the fp32 partial score in the epilogue: every further
// weight costs an epilogue and no GEMM work.
//
// Tile    128 x 128 (queries x passages), 256 threads = 2 x 2 waves of 64 x 64, v_mfma_f32_16x16x32_bf16: 4 x 4 blocks per wave and
//         product, 2 x 64 accumulator registers per lane.  K steps of 64 (d1, d2 are multiples of 32: the last step of a product may be
//         half, its missing 16-byte chunks are staged as zeros), one LDS image per operand ([128 rows][64 k], 16-byte chunk c of row r at
//         c ^ ((r >> 1) & 7): the 16 rows of a fragment read land on distinct banks), the next step's global loads in registers while
//         the current one is multiplied.  Rows behind nq / cols are read from the last valid row (no read out of bounds) and never leave.
// Order   acc1 and acc2 sum their K steps in ascending k, 32 deep per MFMA: a cell's bits depend on its two query rows, its two passage
//         rows and lam[w] only -- not on the tile, the chunk, the epilogue or the other weights.
// Store   S [W * nq, ld] fp32, row w * nq + i, columns 0 .. cols; nothing else is written.
// Filter  the EpiFilter contract (gemm_bf16.h) for the W * nq state rows: a score leaves the tile only if it ranks ahead of its row's
//         current k-th entry (score desc, passage id asc; id -1 = unfilled slot, loses to everything; NaN never qualifies), appended to
//         the row's candidate list through atomicAdd on cnt[row]: at most `cols` entries per row and launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_bf16.h"  // bf16x8, f32x4

namespace dprhot {

constexpr int SP_B = 128, SP_BK = 64, SP_IMG = SP_B * SP_BK;  // tile edge, K step, elements of one operand image (16 KiB)
constexpr int SP_MAXW = 32;                                   // weights per launch

struct SparArgs {
  const uint16_t* Q1;  // bf16 [nq, d1]
  const uint16_t* Q2;  // bf16 [nq, d2]
  const uint16_t* C1;  // bf16 [cols, d1]: row 0 is the chunk's first passage
  const uint16_t* C2;  // bf16 [cols, d2]
  int nq, cols, d1, d2;
  int W;
  float lam[SP_MAXW];
  // store epilogue
  float* S;  // [W * nq, ld]
  long long ld;
  // filter epilogue
  const float* kth_val;    // state values [W * nq, k]
  const int64_t* kth_idx;  // state ids    [W * nq, k]
  int k;
  long long col_offset;  // passage id of column 0
  int* cnt;              // [W * nq]
  float* cand_v;         // [W * nq, ldc]
  int* cand_j;           // [W * nq, ldc]
  long long ldc;
};

// acc += A[m0 .. m0 + 128) x B[n0 .. n0 + 128)^T over K; rows at or behind M / N are read from row M - 1 / N - 1
__device__ __forceinline__ void sp_product(const uint16_t* __restrict__ A, int M, int m0, const uint16_t* __restrict__ B, int N, int n0, int K,
                                           f32x4 (&acc)[4][4], uint16_t* As, uint16_t* Bs, int tid, int lane, int wm, int wn) {
  const int i = lane & 15, g = lane >> 4;
  const uint16_t* ga[4];
  const uint16_t* gb[4];
  int kc[4], so[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // piece e of 1024: row e >> 3, 16-byte chunk e & 7
    const int e = tid + j * 256, row = e >> 3, c = e & 7;
    kc[j] = c * 8;
    so[j] = row * SP_BK + ((c ^ ((row >> 1) & 7)) << 3);
    ga[j] = A + (size_t)min(m0 + row, M - 1) * K + c * 8;
    gb[j] = B + (size_t)min(n0 + row, N - 1) * K + c * 8;
  }
  const int nt = (K + SP_BK - 1) / SP_BK;
  uint4 ra[4], rb[4];
  auto fetch = [&](int t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = t * SP_BK + kc[j] < K;  // (the half step behind a K of 32 mod 64)
      ra[j] = ok ? *reinterpret_cast<const uint4*>(ga[j] + t * SP_BK) : uint4{0u, 0u, 0u, 0u};
      rb[j] = ok ? *reinterpret_cast<const uint4*>(gb[j] + t * SP_BK) : uint4{0u, 0u, 0u, 0u};
    }
  };
  fetch(0);
  for (int t = 0; t < nt; ++t) {
    __syncthreads();  // everybody is done reading the images of the step before
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<uint4*>(As + so[j]) = ra[j];
      *reinterpret_cast<uint4*>(Bs + so[j]) = rb[j];
    }
    __syncthreads();
    if (t + 1 < nt) fetch(t + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int row = wm * 64 + a * 16 + i;
        af[a] = *reinterpret_cast<const bf16x8*>(As + row * SP_BK + (((kk * 4 + g) ^ ((row >> 1) & 7)) << 3));
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int row = wn * 64 + b * 16 + i;
        bfr[b] = *reinterpret_cast<const bf16x8*>(Bs + row * SP_BK + (((kk * 4 + g) ^ ((row >> 1) & 7)) << 3));
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
    }
  }
}

// the score of the contract: one fma, the same instruction in both epilogues
__device__ __forceinline__ float sp_score(float lam, float a2, float a1) { return __builtin_fmaf(lam, a2, a1); }

template <bool FILTER>
__global__ __launch_bounds__(256) void spar_kernel(SparArgs p) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[2 * SP_IMG];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = (int)blockIdx.y * SP_B, n0 = (int)blockIdx.x * SP_B;
  const int i = lane & 15, g = lane >> 4;

  f32x4 acc1[4][4], acc2[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      acc1[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc2[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  sp_product(p.Q1, p.nq, m0, p.C1, p.cols, n0, p.d1, acc1, smem, smem + SP_IMG, tid, lane, wm, wn);
  sp_product(p.Q2, p.nq, m0, p.C2, p.cols, n0, p.d2, acc2, smem, smem + SP_IMG, tid, lane, wm, wn);

  const int mw_ = m0 + wm * 64 + g * 4, nw_ = n0 + wn * 64 + i;  // this lane's cells: rows mw + a * 16 + r, columns nw + b * 16
#pragma unroll 1
  for (int w = 0; w < p.W; ++w) {
    const float lam = p.lam[w];
    const size_t row0 = (size_t)w * p.nq;
    if constexpr (!FILTER) {
      const int mw = mw_, nw = nw_;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = mw + a * 16 + r;
          if (m >= p.nq) continue;
          float* o = p.S + (row0 + m) * (size_t)p.ld;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int n = nw + b * 16;
            if (n < p.cols) o[n] = sp_score(lam, acc2[a][b][r], acc1[a][b][r]);
          }
        }
    } else {
      // the branch-free screen of EpiFilter first: once the thresholds have risen almost no tile holds a score that reaches its
      // row's k-th best
      // (the lane's origin behind an opaque copy per weight: the 16 row addresses and the 20 bounds masks are formed where they
      //  are used instead of being carried around the weight loop in registers the accumulators need)
      int mw = mw_, nw = nw_;
      asm volatile("" : "+v"(mw), "+v"(nw));
      float tv[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) tv[a][r] = p.kth_val[(row0 + min(mw + a * 16 + r, p.nq - 1)) * (size_t)p.k + p.k - 1];
      bool any = false;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int b = 0; b < 4; ++b) any |= sp_score(lam, acc2[a][b][r], acc1[a][b][r]) >= tv[a][r];
      if (!any) continue;
      // the same weight behind an opaque copy: the scores are formed again (same fma, same bits) instead of 256 of them being kept
      // in registers across the screen
      float lam_again = lam;
      asm volatile("" : "+v"(lam_again));
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = mw + a * 16 + r;
          if (m >= p.nq) continue;
          const size_t row = row0 + m;
          const float t = tv[a][r];
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int n = nw + b * 16;
            const float v = sp_score(lam_again, acc2[a][b][r], acc1[a][b][r]);
            if (!(n < p.cols && v >= t)) continue;  // (a NaN compares false)
            bool take = v > t;
            if (!take) {  // exact tie with the k-th best -> lower passage id wins (-1: slot unfilled)
              const long long ti = p.kth_idx[row * (size_t)p.k + p.k - 1];
              take = ti < 0 || p.col_offset + n < ti;
            }
            if (take) {
              const int pos = atomicAdd(&p.cnt[row], 1);
              if ((unsigned)pos >= (unsigned)p.ldc) continue;  // a row's list holds ldc entries: a stale counter never stores outside it
              p.cand_v[row * (size_t)p.ldc + pos] = v;
              p.cand_j[row * (size_t)p.ldc + pos] = n;
            }
          }
        }
    }
  }
}

}  // namespace dprhot
