// dense_fp8.h -- the fp8 dense index: passage rows as OCP e4m3fn codes with one power-of-two scale per row,
//
//   s[i][j] = (acc[i][j] * sq[i]) * sc[j],   acc[i][j] = sum_t value(qc[i][t]) * value(cc[j][t])   (fp32 in the MFMA unit, t ascending)
//
// Format  codes uint8 [n, dp], dp = round_up(d, 32), features behind d are code 0x00; scale fp32 [n].  amax = f * 2^p (1 <= f < 2):
//         e = p - 8 + (f > 1.75), clamped to [-64, 64], scale = 2^e -- the smallest power of two with amax <= 448 * scale, read off the
//         float's bits.  code = e4m3fn(x / scale): the division is exact, rounding is to nearest even, +-448 is the largest magnitude
//         (reached by saturation only where e was clamped).  amax == 0: scale 1.  A non-finite element: scale NaN, codes 0x00.
// Tile    dfp8_kernel is the tile of spar.h on bytes: 128 x 128 (queries x passages), 256 threads = 2 x 2 waves of 64 x 64 (at most 32
//         queries: 32 x 128, waves of 16 x 64, a quarter of the MFMAs -- the search streams the codes once and is bound by that),
//         v_mfma_f32_16x16x32_fp8_fp8 (8 code bytes per lane and step: lane l holds row l & 15, features 8 (l >> 4) .. + 8), 4 x 4 blocks
//         per wave, 64 accumulator registers per lane.  K steps of 128 features (dp is a multiple of 32: the 16-byte chunks of a last
//         step behind dp are staged as zeros), one LDS image per operand ([128 rows][128 bytes] = 16 KiB, 16-byte chunk c of row r at
//         c ^ ((r >> 1) & 7): the 8-byte reads of half a wave cover all 64 banks once), the next step's global loads in registers while
//         the current one is multiplied.  Rows behind nq / cols are read from the last valid row and never leave the tile.
// Order   a cell's bits depend on its two code rows and its two scales only -- not on the tile, the chunk, the id range or the epilogue.
// Store   S [nq, ld] fp32, columns 0 .. cols; nothing else is written.
// Filter  the EpiFilter contract (gemm_bf16.h): a score leaves the tile only if it ranks ahead of its row's current k-th entry (score
//         desc, passage id asc; id -1 = unfilled slot; NaN never qualifies), appended to the row's candidate list through atomicAdd on
//         cnt[row]: at most `cols` entries per row and launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_bf16.h"  // f32x4

namespace dprhot {

constexpr int F8_B = 128, F8_BK = 128;                          // tile edge, K step (features = bytes)
constexpr int F8_TM_SHORT = 32;                                 // query rows of the short tile
constexpr int F8_EMIN = -64, F8_EMAX = 64;                     // the clamp of a row's scale exponent

// ---- encode --------------------------------------------------------------------------------------------------------------------------
// e4m3fn(y), y finite: round to nearest even, saturate at +-448
__device__ __forceinline__ uint32_t f8_code(float y) {
  const uint32_t u = __float_as_uint(y), sign = (u >> 24) & 0x80u, a = u & 0x7FFFFFFFu;
  uint32_t c;
  if (a < 0x3C800000u) {  // |y| < 2^-6: the subnormal grid, steps of 2^-9 (8 steps reach the smallest normal, code 0x08)
    c = (uint32_t)__float2int_rn(__uint_as_float(a) * 512.f);
  } else {
    c = ((a + 0x7FFFFu + ((a >> 20) & 1u)) >> 20) - ((127u - 7u) << 3);  // 3 bits of significand, ties to even; exponent bias 127 -> 7
    c = c > 0x7Eu ? 0x7Eu : c;                                            // 0x7E = 448; 0x7F is NaN
  }
  return sign | c;
}

template <bool BF16>
__device__ __forceinline__ void f8_load16(const void* __restrict__ row, int t0, int d, float (&v)[16]) {
  if constexpr (BF16) {
    const uint16_t* x = static_cast<const uint16_t*>(row);
    if (t0 + 16 <= d && ((reinterpret_cast<uintptr_t>(x + t0) & 15u) == 0)) {
      const uint4 a = *reinterpret_cast<const uint4*>(x + t0), b = *reinterpret_cast<const uint4*>(x + t0 + 8);
      const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[2 * j] = __uint_as_float(w[j] << 16);
        v[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = t0 + j < d ? __uint_as_float((uint32_t)x[t0 + j] << 16) : 0.f;
    }
  } else {
    const float* x = static_cast<const float*>(row);
    if (t0 + 16 <= d && ((reinterpret_cast<uintptr_t>(x + t0) & 15u) == 0)) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(x + t0 + 4 * j);
        v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = t0 + j < d ? x[t0 + j] : 0.f;
    }
  }
}

// One wave per row: pass 1 reduces amax (and "any element non-finite") across the wave, pass 2 writes the codes as 16-byte stores, the
// zero padding behind d included.  rows [n, d] fp32 or bf16, codes [n, dp], scale [n].
template <bool BF16>
__global__ __launch_bounds__(256) void fp8_encode_kernel(const void* __restrict__ rows, long long n, int d, int dp, uint8_t* __restrict__ codes,
                                                         float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const void* row = static_cast<const char*>(rows) + (size_t)r * d * (BF16 ? 2 : 4);
  float v[16];
  float amax = 0.f;
  bool bad = false;
  for (int t0 = lane * 16; t0 < d; t0 += 1024) {
    f8_load16<BF16>(row, t0, d, v);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      bad |= !(__builtin_fabsf(v[j]) < __builtin_inff());  // NaN or +-inf
      amax = __builtin_fmaxf(amax, __builtin_fabsf(v[j]));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = __builtin_fmaxf(amax, __shfl_xor(amax, o, 64));
  bad = __any(bad);
  // amax = f * 2^p: e = p - 8 + (f > 1.75), from the bits (a subnormal amax reads p = -127: clamped like every p < -56)
  const uint32_t ab = __float_as_uint(amax);
  int e = (int)(ab >> 23) - 127 - 8 + ((ab & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  e = e < F8_EMIN ? F8_EMIN : e > F8_EMAX ? F8_EMAX : e;
  if (amax == 0.f) e = 0;
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e: the division is an exact multiplication
  if (lane == 0) scale[r] = bad ? __builtin_nanf("") : __uint_as_float((uint32_t)(127 + e) << 23);
  uint8_t* out = codes + (size_t)r * dp;
  for (int t0 = lane * 16; t0 < dp; t0 += 1024) {  // (dp % 16 == 0: whole 16-byte pieces)
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (!bad && t0 < d) {
      f8_load16<BF16>(row, t0, d, v);
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j >> 2] |= f8_code(v[j] * inv) << (8 * (j & 3));
    }
    *reinterpret_cast<uint4*>(out + t0) = uint4{w[0], w[1], w[2], w[3]};
  }
}

// ---- search --------------------------------------------------------------------------------------------------------------------------
struct Dfp8Args {
  const uint8_t* Qc;  // codes [nq, dp]
  const float* qs;    // [nq]
  const uint8_t* Cc;  // codes [cols, dp]: row 0 is the chunk's first passage
  const float* cs;    // [cols]
  int nq, cols, dp;
  // store epilogue
  float* S;  // [nq, ld]
  long long ld;
  // filter epilogue
  const float* kth_val;    // state values [nq, k]
  const int64_t* kth_idx;  // state ids    [nq, k]
  int k;
  long long col_offset;  // passage id of column 0
  int* cnt;              // [nq]
  float* cand_v;         // [nq, ldc]
  int* cand_j;           // [nq, ldc]
  long long ldc;
};

// the score of the contract: two fp32 multiplies, the same instructions in both epilogues
__device__ __forceinline__ float f8_score(float acc, float sq, float sc) { return (acc * sq) * sc; }

// TM: query rows of the tile, 128 or 32 (F8_TM_SHORT: the tile of a search with at most 32 queries, which streams the codes once and
// would spend three quarters of its MFMAs on rows behind nq otherwise); the wave grid stays 2 x 2, a wave holds TM / 32 x 4 blocks.
template <bool FILTER, int TM>
__global__ __launch_bounds__(256) void dfp8_kernel(Dfp8Args p) {
  constexpr int NA = TM / 32;  // 16-row blocks per wave = 16-byte pieces of the query image per thread
  __shared__ __attribute__((aligned(16))) uint8_t smem[(TM + F8_B) * F8_BK];
  uint8_t* As = smem;
  uint8_t* Bs = smem + TM * F8_BK;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = (int)blockIdx.y * TM, n0 = (int)blockIdx.x * F8_B;
  const int i = lane & 15, g = lane >> 4;
  const int K = p.dp;

  f32x4 acc[NA][4];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const uint8_t* ga[4];  // (the first NA are used)
  const uint8_t* gb[4];
  int kc[4], so[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // piece e of an image: row e >> 3, 16-byte chunk e & 7 (the query image has TM * 8 pieces)
    const int e = tid + j * 256, row = e >> 3, c = e & 7;
    kc[j] = c * 16;
    so[j] = row * F8_BK + ((c ^ ((row >> 1) & 7)) << 4);
    if (j < NA) ga[j] = p.Qc + (size_t)min(m0 + row, p.nq - 1) * K + c * 16;
    gb[j] = p.Cc + (size_t)min(n0 + row, p.cols - 1) * K + c * 16;
  }
  const int nt = (K + F8_BK - 1) / F8_BK;
  uint4 ra[4], rb[4];
  auto fetch = [&](int t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = t * F8_BK + kc[j] < K;  // (the chunks behind a dp of 32, 64 or 96 mod 128)
      if (j < NA) ra[j] = ok ? *reinterpret_cast<const uint4*>(ga[j] + t * F8_BK) : uint4{0u, 0u, 0u, 0u};
      rb[j] = ok ? *reinterpret_cast<const uint4*>(gb[j] + t * F8_BK) : uint4{0u, 0u, 0u, 0u};
    }
  };
  fetch(0);
  for (int t = 0; t < nt; ++t) {
    __syncthreads();  // everybody is done reading the images of the step before
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < NA) *reinterpret_cast<uint4*>(As + so[j]) = ra[j];
      *reinterpret_cast<uint4*>(Bs + so[j]) = rb[j];
    }
    __syncthreads();
    if (t + 1 < nt) fetch(t + 1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {  // features kk * 32 + 8 g .. + 8 of the step: chunk kk * 2 + (g >> 1), its half g & 1
      long af[NA], bfr[4];
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int row = wm * (TM / 2) + a * 16 + i;
        af[a] = *reinterpret_cast<const long*>(As + row * F8_BK + (((kk * 2 + (g >> 1)) ^ ((row >> 1) & 7)) << 4) + ((g & 1) << 3));
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int row = wn * 64 + b * 16 + i;
        bfr[b] = *reinterpret_cast<const long*>(Bs + row * F8_BK + (((kk * 2 + (g >> 1)) ^ ((row >> 1) & 7)) << 4) + ((g & 1) << 3));
      }
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(af[a], bfr[b], acc[a][b], 0, 0, 0);
    }
  }

  // this lane's cells: rows mw + a * 16 + r, columns nw + b * 16
  const int mw = m0 + wm * (TM / 2) + g * 4, nw = n0 + wn * 64 + i;
  float sc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) sc[b] = p.cs[min(nw + b * 16, p.cols - 1)];
  if constexpr (!FILTER) {
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mw + a * 16 + r;
        if (m >= p.nq) continue;
        const float sq = p.qs[m];
        float* o = p.S + (size_t)m * (size_t)p.ld;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int n = nw + b * 16;
          if (n < p.cols) o[n] = f8_score(acc[a][b][r], sq, sc[b]);
        }
      }
  } else {
    // the branch-free screen of EpiFilter first: once the thresholds have risen almost no tile holds a score that reaches its row's
    // k-th best
    float tv[NA][4], sq[NA][4];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = min(mw + a * 16 + r, p.nq - 1);
        tv[a][r] = p.kth_val[(size_t)m * (size_t)p.k + p.k - 1];
        sq[a][r] = p.qs[m];
      }
    bool any = false;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int b = 0; b < 4; ++b) any |= f8_score(acc[a][b][r], sq[a][r], sc[b]) >= tv[a][r];
    if (!any) return;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mw + a * 16 + r;
        if (m >= p.nq) continue;
        const size_t row = (size_t)m;
        const float t = tv[a][r];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int n = nw + b * 16;
          const float v = f8_score(acc[a][b][r], sq[a][r], sc[b]);
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

}  // namespace dprhot
