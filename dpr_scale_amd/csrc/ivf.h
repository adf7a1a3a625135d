// ivf.h -- inverted-index scoring of CITADEL / COIL retrieval: the expert part of
//
//   score(n, doc) = sum over entries (e, u) of query n of  max(0, max over postings (doc, v) of expert e of <u, v>)
//
// added into one chunk S[nq, cols] of the score matrix (doc ids D0 .. D0 + cols).  The [nq, corpus_len] matrix never exists, nor do the
// token-level products.
//
// Index   postings sorted by (expert, doc): pv bf16 [P, dp] (dp = d padded with zeros to a multiple of 32), pd int32 [P] doc ids,
//         eoff int64 [V + 1] offsets by expert id.
// Batch   entries sorted by (expert, query, slot): ev bf16 [Eq, dp], eq int32 [Eq] query rows; bexp int32 [nb] the distinct experts of
//         the batch in ascending order, boff int32 [nb + 1] their entry ranges.
//
// Plan    ONE WAVE owns IVF_T consecutive doc ids for all queries (a workgroup is four independent waves; no workgroup barrier).
//   1. 64 batch experts at a time, one per lane: the postings of the expert inside the wave's doc range by binary search on the sorted
//      doc ids (lower bound of the first id in the whole list, then a galloping search for the end, which is a few postings away).
//   2. The non-empty (expert, range) pairs are walked in ascending expert order.  16 entries x 64 postings per step on
//      v_mfma_f32_16x16x32_bf16 (d = 32 is one instruction per 16 x 16 block); the epilogue clamps at 0 and folds every product into
//      an LDS table M[16 entries][IVF_T docs] with an INTEGER max on the bit pattern (non-negative floats order as integers; a max does
//      not depend on the order of its operands) -- the segmented max over a doc's run of postings, wherever the run is cut.
//   3. Flush: the lane that holds the first posting of a doc's run owns that doc for this step; it adds M[r][doc] for r = 0 .. 15 in
//      entry order into S[query(r), doc] with plain loads and stores and clears the table cells it read.
// Every cell S[n, doc] therefore receives its contributions one at a time in the order (expert ascending, the query's entries as
// listed), by one lane at a time: no floating-point atomics, two runs are bit-identical, and the result does not depend on the chunk,
// on the other queries of the batch (a zero contribution is skipped, never added) or on how the index was sharded on disk.
// A unit's work is bounded by the doc range, not by an expert: a hot expert's list is cut into as many pieces as there are waves.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dprhot {

constexpr int IVF_T = 128;      // doc ids per wave
constexpr int IVF_WAVES = 4;    // independent waves per workgroup
constexpr int IVF_ROWS = 16;    // entries per MFMA step

struct IvfArgs {
  const uint16_t* pv;    // bf16 [P, dp]
  const int* pd;         // [P]
  const long long* eoff; // [V + 1]
  int V, dp;
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

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short ivf_bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float ivf_f32x4;

__device__ __forceinline__ ivf_bf16x8 ivf_load8(const uint16_t* p, bool ok) {
  ivf_bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? *reinterpret_cast<const ivf_bf16x8*>(p) : z;
}

// wave-level ordering point between the phases of a step: LDS and global accesses of the wave issued before it have completed
__device__ __forceinline__ void ivf_phase() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(64 * IVF_WAVES) void ivf_score_kernel(IvfArgs p) {
  __shared__ int M[IVF_WAVES][IVF_ROWS * IVF_T];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long t0 = ((long long)blockIdx.x * IVF_WAVES + wave) * IVF_T;
  if (t0 >= p.cols) return;  // (no workgroup barrier anywhere in this kernel)
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
        const uint16_t* qa = p.ev + (long long)(eg + (ra_ok ? i16 : 0)) * p.dp + g4 * 8;
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
          for (int k = 0; k < p.dp; k += 32) {
            const ivf_bf16x8 af = k == 0 ? af0 : ivf_load8(qa + k, ra_ok);
            ivf_bf16x8 bfr[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) bfr[b] = ivf_load8(p.pv + (ps + (cok[b] ? col[b] : 0)) * p.dp + g4 * 8 + k, cok[b]);
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

}  // namespace dprhot
