// ivf_pack.h -- from encoder outputs to index postings and query batches ("Building postings and query batches"):
// the per-token loops of the reference's citadel_eval_task.py:43-70 (index writer) and citadel_retrieval_task.py:104-125 (query side).
//
// Both sides do one thing to a repr dict (expert_repr [B, L, d], expert_ids / expert_weights [B, L, K], attention_mask [B, L]): a slot
// (b, t, k) is KEPT when att[b, t] > 0 and its weight passes the side's test; the kept slots are emitted in (b, t, k) order, each with
// its expert id, its sequence's row id, its weight and the vector weight * expert_repr[b, t].
//
// Compaction  ONE WAVE owns one sequence.
//   ivf_count_kernel   the wave walks the L K slots 64 at a time and adds up the population counts of the ballots of kept lanes.
//   ivf_scan_kernel    one workgroup turns the B counts into offsets (integer sums).
//   ivf_emit_kernel    the same walk; a kept lane's record index is base + (kept lanes below it in the ballot), base running over the
//                      steps from the sequence's offset: the order is exact by construction.  No atomics.
// Gather      one thread per output element: the record's token row times its weight, one fp32 multiply, then the rounding chain
//             prod_round -> (fp16) -> fp32 | bf16, every step to nearest even, as torch does on the host; padding columns are zeros.
// Every output element has one owner: two runs are bit-identical.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dprhot {

constexpr int IVFP_WAVES = 4;  // sequences per workgroup (independent waves, no workgroup barrier)
constexpr int IVFP_FP32 = 0, IVFP_BF16 = 1, IVFP_FP16 = 2;

struct IvfCompactArgs {
  const int* ids;        // [B, L, K]
  const float* w;        // [B, L, K] or NULL (all 1)
  const uint8_t* att;    // [B, L]
  const int* row_ids;    // [B]
  int B, L, K;
  int test_weight;
  float min_weight;
  int* seq_off;          // [B + 1]
  int* out_expert;       // [capacity] each
  int* out_row;
  int* out_slot;
  float* out_weight;
  long long capacity;
};

// slot s = t K + k of sequence b (s < L K)
__device__ __forceinline__ bool ivf_keep(const IvfCompactArgs& p, int b, int s, float* weight) {
  const int t = s / p.K;
  const float w = p.w != nullptr ? p.w[(long long)b * p.L * p.K + s] : 1.0f;
  *weight = w;
  return p.att[(long long)b * p.L + t] > 0 && (p.test_weight == 0 || w > p.min_weight);  // (a NaN weight fails the comparison)
}

__global__ __launch_bounds__(64 * IVFP_WAVES) void ivf_count_kernel(IvfCompactArgs p) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * IVFP_WAVES + (threadIdx.x >> 6);
  if (b >= p.B) return;  // (wave-uniform; no workgroup barrier in this kernel)
  const int LK = p.L * p.K;
  int cnt = 0;
  for (int s0 = 0; s0 < LK; s0 += 64) {
    const int s = s0 + lane;
    float w;
    const bool keep = s < LK && ivf_keep(p, b, s, &w);
    cnt += __popcll(__ballot(keep));
  }
  if (lane == 0) p.seq_off[b + 1] = cnt;
}

// seq_off[1 .. B] holds the counts; afterwards seq_off[b] = sum of the counts before b.  Every thread owns one contiguous piece.
__global__ __launch_bounds__(256) void ivf_scan_kernel(int* seq_off, int B) {
  __shared__ int part[256];
  const int tid = threadIdx.x;
  const int per = (B + 255) / 256;
  const int lo = tid * per < B ? tid * per : B;
  const int hi = lo + per < B ? lo + per : B;
  int s = 0;
  for (int i = lo; i < hi; ++i) s += seq_off[i + 1];
  part[tid] = s;
  __syncthreads();
  int base = 0;
  for (int j = 0; j < tid; ++j) base += part[j];
  if (tid == 0) seq_off[0] = 0;
  for (int i = lo; i < hi; ++i) {
    base += seq_off[i + 1];
    seq_off[i + 1] = base;
  }
}

__global__ __launch_bounds__(64 * IVFP_WAVES) void ivf_emit_kernel(IvfCompactArgs p) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * IVFP_WAVES + (threadIdx.x >> 6);
  if (b >= p.B) return;
  const int LK = p.L * p.K;
  const int row = p.row_ids[b];
  long long base = p.seq_off[b];
  for (int s0 = 0; s0 < LK; s0 += 64) {
    const int s = s0 + lane;
    float w = 0.f;
    const bool keep = s < LK && ivf_keep(p, b, s, &w);
    const unsigned long long kept = __ballot(keep);
    const long long r = base + __popcll(kept & ((1ull << lane) - 1ull));
    if (keep && r < p.capacity) {
      const int flat = b * LK + s;  // (B L K < 2^31)
      p.out_expert[r] = p.ids[flat];
      p.out_row[r] = row;
      p.out_slot[r] = flat;
      p.out_weight[r] = w;
    }
    base += __popcll(kept);
  }
}

struct IvfGatherArgs {
  const float* x;         // [n_rows, d], row stride x_ld
  long long x_ld, n_rows;
  const float* w;         // [n_rows K] or NULL (all 1)
  const int* slot;        // [n]
  const long long* perm;  // [n] or NULL
  long long n;
  int d, K, prod_round, entry_round;
  void* out;              // [n, out_ld] fp32 or bf16
  long long out_ld;
};

// fp32 -> bf16 -> fp32, round to nearest even (the bits torch's cast gives; a NaN becomes the quiet NaN 0x7fc0)
__device__ __forceinline__ float ivf_rne_bf16(float v) {
  unsigned u = __float_as_uint(v);
  u = v != v ? 0x7fc00000u : (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
  return __uint_as_float(u);
}

__device__ __forceinline__ float ivf_rne_fp16(float v) { return __half2float(__float2half_rn(v)); }

template <int OUT>
__global__ __launch_bounds__(256) void ivf_gather_kernel(IvfGatherArgs p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.n * p.out_ld) return;
  const long long i = idx / p.out_ld;
  const int c = (int)(idx - i * p.out_ld);
  float v = 0.f;
  if (c < p.d) {
    const long long r = p.perm != nullptr ? p.perm[i] : i;
    if (r >= 0 && r < p.n) {
      const int s = p.slot[r];
      const long long row = s / p.K;
      if (s >= 0 && row < p.n_rows) {
        const float w = p.w != nullptr ? p.w[s] : 1.0f;
        v = __fmul_rn(w, p.x[row * p.x_ld + c]);  // one fp32 multiply; nothing to contract it with
        if (p.prod_round == IVFP_BF16) v = ivf_rne_bf16(v);
        if (p.prod_round == IVFP_FP16 || p.entry_round != 0) v = ivf_rne_fp16(v);
      }
    }
  }
  if (OUT == IVFP_BF16)
    static_cast<uint16_t*>(p.out)[idx] = (uint16_t)(__float_as_uint(ivf_rne_bf16(v)) >> 16);
  else
    static_cast<float*>(p.out)[idx] = v;
}

}  // namespace dprhot
