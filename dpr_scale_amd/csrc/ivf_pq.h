// ivf_pq.h -- product-quantised postings for the inverted index of csrc/ivf.h.
//
// Index   postings sorted by (expert, doc) as in ivf.h, but a posting's row is code uint8 [P, m] -- one 8-bit code per subspace of DSUB
//         features, m = dp / DSUB -- and one codebook cb bf16 [m, 256, DSUB] serves the whole index:
//             decode(p)[j * DSUB + t] = cb[j, code[p, j], t]
// Score   ivf_pq_score_kernel is ivf_score_kernel (same ownership, same order of additions, same flush) with ONE change: the B
//         fragment of a posting is assembled from its code bytes and the codebook instead of being loaded from pv.  Lane (i16, g4) at
//         K step k holds features k + 8 g4 .. + 7 = 8 / DSUB whole sub-vectors, so it reads 8 / DSUB code bytes (one 1-, 2- or 4-byte
//         load) and as many DSUB-wide codebook rows (16-, 8- or 4-byte LDS reads).  The MFMA operands are then bit for bit those of
//         the dense kernel over decode(p), and so is every score.
//         The codebook (dp * 512 bytes) is staged in LDS once per workgroup by all four waves; the workgroup barrier behind that load
//         comes BEFORE the return of the waves past the end of the chunk (the dense kernel has no barrier and returns at the top).
// Encode  pq_encode_kernel: code[r, j] = argmin over c = 0 .. 255 of D(c) = sum over t = 0 .. DSUB - 1 (in that order) of
//         (x_t - cb_t)^2, every subtract, multiply and add rounded on its own in fp32 (nothing contracted into an fma), strict <
//         (the lowest index wins a tie, a NaN distance never wins, a row of NaNs gets code 0).  One block column per subspace with its
//         256 centroids widened into LDS; one thread owns one output byte; exactly n * m bytes are written.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf.h"

namespace dprhot {

struct IvfPqArgs {
  const uint8_t* code;   // uint8 [P, dp / DSUB]
  const uint16_t* cb;    // bf16 [dp / DSUB, 256, DSUB]
  const int* pd;         // [P]
  const long long* eoff; // [V + 1]
  int V;
  const uint16_t* ev;    // bf16 [Eq, dp]
  const int* eq;         // [Eq]
  const int* bexp;       // [nb]
  const int* boff;       // [nb + 1]
  int nb, nq;
  long long D0;          // first doc id of the chunk
  int cols;              // doc ids in the chunk
  float* S;              // [nq, ld]
  long long ld;
};

typedef __attribute__((__vector_size__(2 * sizeof(int)))) int ivf_i32x2;
typedef __attribute__((__vector_size__(4 * sizeof(int)))) int ivf_i32x4;

// the 8 bf16 features of sub-vectors j0 .. j0 + 8 / DSUB - 1 of the posting whose code row starts at `code`; cb: the codebook in LDS
template <int DSUB>
__device__ __forceinline__ ivf_bf16x8 ivf_pq_frag(const uint8_t* code, const uint16_t* cb, int j0, bool ok) {
  ivf_i32x4 w = {0, 0, 0, 0};
  if constexpr (DSUB == 8) {
    const unsigned c = code[j0];
    w = reinterpret_cast<const ivf_i32x4*>(cb)[j0 * 256 + c];
  } else if constexpr (DSUB == 4) {
    const unsigned c = *reinterpret_cast<const uint16_t*>(code + j0);
    const ivf_i32x2 lo = reinterpret_cast<const ivf_i32x2*>(cb)[j0 * 256 + (c & 255u)];
    const ivf_i32x2 hi = reinterpret_cast<const ivf_i32x2*>(cb)[(j0 + 1) * 256 + (c >> 8)];
    w = ivf_i32x4{lo[0], lo[1], hi[0], hi[1]};
  } else {
    static_assert(DSUB == 2, "sub-vectors of 2, 4 or 8 features");
    const unsigned c = *reinterpret_cast<const uint32_t*>(code + j0);
    const int* q = reinterpret_cast<const int*>(cb) + j0 * 256;
    w = ivf_i32x4{q[c & 255u], q[256 + ((c >> 8) & 255u)], q[512 + ((c >> 16) & 255u)], q[768 + (c >> 24)]};
  }
  const ivf_i32x4 z = {0, 0, 0, 0};
  return (ivf_bf16x8)(ok ? w : z);
}

template <int DSUB, int DP>
__global__ __launch_bounds__(64 * IVF_WAVES) void ivf_pq_score_kernel(IvfPqArgs p) {
  constexpr int MSUB = DP / DSUB;  // code bytes per posting
  __shared__ int M[IVF_WAVES][IVF_ROWS * IVF_T];
  __shared__ __attribute__((aligned(16))) uint16_t CB[DP * 256];
  // every wave of the workgroup takes part in the codebook load, also one that has no doc range of its own
  for (int i = threadIdx.x; i < DP * 32; i += 64 * IVF_WAVES)
    reinterpret_cast<ivf_i32x4*>(CB)[i] = reinterpret_cast<const ivf_i32x4*>(p.cb)[i];
  __syncthreads();  // (the only workgroup barrier; behind it the waves are independent as in ivf_score_kernel)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long t0 = ((long long)blockIdx.x * IVF_WAVES + wave) * IVF_T;
  if (t0 >= p.cols) return;
  int* m = M[wave];
  for (int i = lane; i < IVF_ROWS * IVF_T; i += 64) m[i] = 0;
  const long long t1 = t0 + IVF_T < p.cols ? t0 + IVF_T : (long long)p.cols;
  const int d0 = (int)(p.D0 + t0), d1 = (int)(p.D0 + t1);
  const int i16 = lane & 15, g4 = lane >> 4;
  ivf_phase();

  for (int b0 = 0; b0 < p.nb; b0 += 64) {
    // 1. this lane's expert: its postings with d0 <= doc < d1 are [s, s + cnt)
    long long s = 0;
    int cnt = 0;
    if (b0 + lane < p.nb) {
      const int x = p.bexp[b0 + lane];
      if (x >= 0 && x < p.V) {
        const long long hi = p.eoff[x + 1];
        long long a = p.eoff[x], b = hi;
        while (a < b) {
          const long long mid = (a + b) >> 1;
          if (p.pd[mid] < d0) a = mid + 1; else b = mid;
        }
        s = a;
        long long w = 1;  // every posting before a is < d1
        while (a + w <= hi && p.pd[a + w - 1] < d1) { a += w; w <<= 1; }
        b = a + w < hi ? a + w : hi;
        while (a < b) {
          const long long mid = (a + b) >> 1;
          if (p.pd[mid] < d1) a = mid + 1; else b = mid;
        }
        cnt = (int)(a - s);
      }
    }
    unsigned long long live = __ballot(cnt > 0);
    while (live) {
      const int l = __ffsll((long long)live) - 1;
      live &= live - 1;
      const long long ps = __shfl(s, l, 64);
      const int pc = __shfl(cnt, l, 64);
      const int e0 = p.boff[b0 + l], e1 = p.boff[b0 + l + 1];
      for (int eg = e0; eg < e1; eg += IVF_ROWS) {
        const int ne = e1 - eg < IVF_ROWS ? e1 - eg : IVF_ROWS;
        const bool ra_ok = i16 < ne;
        const uint16_t* qa = p.ev + (long long)(eg + (ra_ok ? i16 : 0)) * DP + g4 * 8;
        const ivf_bf16x8 af0 = ivf_load8(qa, ra_ok);
        // 2. products, clamp, segmented max into M
        for (int c0 = 0; c0 < pc; c0 += 64) {
          ivf_f32x4 acc[4];
          int col[4];
          bool cok[4];
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            acc[b] = ivf_f32x4{0.f, 0.f, 0.f, 0.f};
            col[b] = c0 + b * 16 + i16;
            cok[b] = col[b] < pc;
          }
#pragma unroll
          for (int k = 0; k < DP; k += 32) {
            const ivf_bf16x8 af = k == 0 ? af0 : ivf_load8(qa + k, ra_ok);
            ivf_bf16x8 bfr[4];
#pragma unroll
            for (int b = 0; b < 4; ++b)
              bfr[b] = ivf_pq_frag<DSUB>(p.code + (ps + (cok[b] ? col[b] : 0)) * MSUB, CB, (k + g4 * 8) / DSUB, cok[b]);
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[b], acc[b], 0, 0, 0);
          }
          // lane holds entries g4 * 4 + r of posting col[b]
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            if (!cok[b]) continue;
            const int dl = p.pd[ps + col[b]] - d0;
            if ((unsigned)dl >= (unsigned)IVF_T) continue;  // (unreachable for a sorted index)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float v = acc[b][r];
              if (v > 0.f) atomicMax(&m[(g4 * 4 + r) * IVF_T + dl], __float_as_int(v));  // integer max in LDS
            }
          }
        }
        ivf_phase();
        // 3. the first posting of every doc's run adds the doc's column of M into S, entries in order
        for (int c = lane; c < pc; c += 64) {
          const int doc = p.pd[ps + c];
          if (c > 0 && p.pd[ps + c - 1] == doc) continue;
          const int dl = doc - d0;
          if ((unsigned)dl >= (unsigned)IVF_T) continue;
          for (int r = 0; r < ne; ++r) {
            const int bits = m[r * IVF_T + dl];
            if (bits == 0) continue;
            m[r * IVF_T + dl] = 0;
            const int q = p.eq[eg + r];
            if ((unsigned)q >= (unsigned)p.nq) continue;
            float* cell = p.S + (long long)q * p.ld + (doc - p.D0);
            *cell = *cell + __int_as_float(bits);
          }
        }
        ivf_phase();
      }
    }
  }
}

struct PqEncodeArgs {
  const uint16_t* vec;   // bf16 [n, dp]
  long long n;
  int dp;
  const uint16_t* cb;    // bf16 [dp / DSUB, 256, DSUB]
  uint8_t* codes;        // uint8 [n, dp / DSUB]
};

constexpr int PQ_ENC_THREADS = 256;

template <int DSUB>
__global__ __launch_bounds__(PQ_ENC_THREADS) void pq_encode_kernel(PqEncodeArgs p) {
#pragma clang fp contract(off)  // D(c) is defined with separately rounded operations
  __shared__ float C[256 * DSUB];
  const int j = blockIdx.y, msub = p.dp / DSUB;
  for (int i = threadIdx.x; i < 256 * DSUB; i += PQ_ENC_THREADS)
    C[i] = __uint_as_float((uint32_t)p.cb[(long long)j * 256 * DSUB + i] << 16);
  __syncthreads();
  for (long long r = (long long)blockIdx.x * PQ_ENC_THREADS + threadIdx.x; r < p.n; r += (long long)gridDim.x * PQ_ENC_THREADS) {
    const uint16_t* row = p.vec + r * p.dp + j * DSUB;
    float x[DSUB];
#pragma unroll
    for (int t = 0; t < DSUB; ++t) x[t] = __uint_as_float((uint32_t)row[t] << 16);
    float best = __builtin_inff();
    int code = 0;
    for (int c = 0; c < 256; ++c) {
      float D = 0.f;
#pragma unroll
      for (int t = 0; t < DSUB; ++t) {
        const float diff = __fsub_rn(x[t], C[c * DSUB + t]);
        const float sq = __fmul_rn(diff, diff);
        D = t == 0 ? sq : __fadd_rn(D, sq);
      }
      if (D < best) {
        best = D;
        code = c;
      }
    }
    p.codes[r * msub + j] = (uint8_t)code;
  }
}

}  // namespace dprhot
