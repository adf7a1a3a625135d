// router_head.h -- the CITADEL / SPLADE encoder head behind the MLM logits (reference: dpr_scale/models/citadel_models/
// citadel_model.py:46-82, splade_model.py:26-32), forward and backward, without any [B, T, V] temporary (gfx950, wave64).
//   x[b,t,v] = logits[b, t + skip, v]   m[b,t] = mask[b, t + skip] != 0   f = m ? log(1 + relu(x)) : 0
//   rh_row_kernel  one workgroup per token row, the row in registers: row logsumexp (saved for the backward and for rh_col_kernel) and
//                  the k routing rounds (block argmax, value descending then vocabulary index ascending)
//   rh_col_kernel  one thread per (sequence, vocabulary column), tokens in order: max_t f with its first token, sum_t softmax, and the
//                  routing count of the column (integer LDS histogram of the sequence's expert ids)
//   rh_bwd_sparse_kernel  dlogits without a softmax gradient: no reduction, the logits are read only where a gradient lands
//   rh_bwd_row_kernel     dlogits with the softmax gradient: one workgroup per token row, one block reduction (sum_u p g_soft)
// Every output element has one owner that adds in a fixed order; there is no floating-point atomic.  Rows are addressed by element
// strides and read with element-sized loads: no alignment beyond the element's own is assumed.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "rowwise.h"

namespace dprhot {

constexpr int RH_THREADS = 1024;  // rh_row_kernel / rh_bwd_row_kernel: 16 waves, a row of 30522 is 30 values per thread
constexpr int RH_WAVES = RH_THREADS / 64;
constexpr int RH_KMAX = 8;
constexpr int RH_COLS = 256;      // columns per workgroup of the column-owned kernels
constexpr int RH_BWD_ROWS = 16;   // token rows per workgroup of rh_bwd_sparse_kernel
enum { RH_BF16 = 0, RH_FP16 = 1, RH_FP32 = 2 };  // the dtype codes of the gradient-bucket legs (dprhot_grad_pack)

struct RhArgs {
  const void* x;        // logits [B, T1, V], element strides sb / st, unit column stride
  const uint8_t* mask;  // [B, T1]
  int B, T1, T, V, skip, k, want_soft;
  long long sb, st;
  // forward outputs (dtype of the logits unless noted)
  void* repr;     // [B, V]
  int* arg;       // [B, V] int32
  void* w;        // [B, T, k]
  int* ids;       // [B, T, k] int32
  void* rmask;    // [B, V]
  void* ssum;     // [B, V]
  float* lse;     // [B, T] fp32 (workspace)
  // backward
  const float* g_repr;  // [B, V] or NULL
  const float* g_w;     // [B, T, k] or NULL
  const float* g_soft;  // [B, V] or NULL
  void* dx;             // [B, T1, V] contiguous
};

template <int DT>
__device__ __forceinline__ float rh_ld(const void* p, long long i) {
  if constexpr (DT == RH_FP32) return ((const float*)p)[i];
  else if constexpr (DT == RH_BF16) return __uint_as_float((uint32_t)((const uint16_t*)p)[i] << 16);
  else return (float)((const _Float16*)p)[i];
}
template <int DT>
__device__ __forceinline__ void rh_st(void* p, long long i, float v) {
  if constexpr (DT == RH_FP32) ((float*)p)[i] = v;
  else if constexpr (DT == RH_BF16) ((uint16_t*)p)[i] = (uint16_t)(pk_bf16(v, 0.f) & 0xffffu);
  else ((_Float16*)p)[i] = (_Float16)v;
}

// f of an unmasked token: the log of the fp32-rounded 1 + x (citadel_model.py:55), 0 for x <= 0 and for a NaN logit
__device__ __forceinline__ float rh_f(float x) { return x > 0.f ? logf(1.0f + x) : 0.f; }
// its derivative (0 at x <= 0 and at NaN; 0 at +inf)
__device__ __forceinline__ float rh_df(float x) { return x > 0.f ? 1.0f / (1.0f + x) : 0.f; }

// block reductions over RH_THREADS threads: wave reduction, then the 16 wave results combined in wave order by every thread
__device__ __forceinline__ float rh_block_max(float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int i = 1; i < RH_WAVES; ++i) r = fmaxf(r, sh[i]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float rh_block_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int i = 1; i < RH_WAVES; ++i) r += sh[i];
  __syncthreads();
  return r;
}
// (value descending, index ascending): is (f, i) ahead of (g, j)?
__device__ __forceinline__ bool rh_ahead(float f, int i, float g, int j) { return f > g || (f == g && i < j); }

// NPT > 0: the row lives in NPT registers per thread (V <= NPT * RH_THREADS).  NPT == 0: any V, every pass re-reads the row (L2).
template <int DT, int NPT>
__global__ __launch_bounds__(RH_THREADS) void rh_row_kernel(RhArgs a) {
  __shared__ float sh[RH_WAVES];
  __shared__ float shf[RH_WAVES];
  __shared__ int shi[RH_WAVES];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int b = row / a.T, t = row - b * a.T;
  const long long base = (long long)b * a.sb + (long long)(t + a.skip) * a.st;
  const bool live = a.mask[(long long)b * a.T1 + t + a.skip] != 0;
  const int V = a.V;
  constexpr int UNR = NPT ? NPT : 1;  // the register-resident row is walked fully unrolled, the re-read one not at all
  const int nit = NPT ? NPT : (V + RH_THREADS - 1) / RH_THREADS;
  float xv[NPT ? NPT : 1];
  if constexpr (NPT > 0) {
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int v = tid + i * RH_THREADS;
      xv[i] = v < V ? rh_ld<DT>(a.x, base + v) : -INFINITY;
    }
  }
  auto val = [&](int i, int v) -> float {
    if constexpr (NPT > 0) return xv[i];
    else return v < V ? rh_ld<DT>(a.x, base + v) : -INFINITY;
  };
  if (a.want_soft) {  // padded tokens count as well (citadel_model.py:71)
    float mx = -INFINITY;
#pragma unroll UNR
    for (int i = 0; i < nit; ++i) mx = fmaxf(mx, val(i, tid + i * RH_THREADS));
    mx = rh_block_max(mx, sh);
    float s = 0.f;
#pragma unroll UNR
    for (int i = 0; i < nit; ++i) s += expf(val(i, tid + i * RH_THREADS) - mx);
    s = rh_block_sum(s, sh);
    if (tid == 0) a.lse[row] = mx + logf(s);
  }
  const int k = a.k;
  if (k == 0) return;
  const long long o = (long long)row * k;
  if (!live) {  // every f is 0: the first k columns, weight 0
    if (tid < k) {
      a.ids[o + tid] = tid;
      rh_st<DT>(a.w, o + tid, 0.f);
    }
    return;
  }
  if constexpr (NPT > 0) {
#pragma unroll
    for (int i = 0; i < NPT; ++i) xv[i] = rh_f(xv[i]);
  }
  float pf = INFINITY;  // the previous round's winner: this round takes what comes strictly behind it
  int pi = -1;
  for (int j = 0; j < k; ++j) {
    float bf = -1.f;
    int bi = 0x7fffffff;
#pragma unroll UNR
    for (int i = 0; i < nit; ++i) {
      const int v = tid + i * RH_THREADS;
      float f;
      if constexpr (NPT > 0) f = xv[i];
      else f = rh_f(val(i, v));
      const bool cand = v < V && (f < pf || (f == pf && v > pi));
      if (cand && rh_ahead(f, v, bf, bi)) { bf = f; bi = v; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float of = __shfl_xor(bf, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (rh_ahead(of, oi, bf, bi)) { bf = of; bi = oi; }
    }
    if ((tid & 63) == 0) { shf[tid >> 6] = bf; shi[tid >> 6] = bi; }
    __syncthreads();
    bf = shf[0];
    bi = shi[0];
#pragma unroll
    for (int i = 1; i < RH_WAVES; ++i)
      if (rh_ahead(shf[i], shi[i], bf, bi)) { bf = shf[i]; bi = shi[i]; }
    __syncthreads();
    if (tid == 0) {  // V >= k: a candidate exists in every round, bi is a column of the row
      a.ids[o + j] = bi;
      rh_st<DT>(a.w, o + j, bf);
    }
    pf = bf;
    pi = bi;
  }
}

template <int DT>
__global__ __launch_bounds__(RH_COLS) void rh_col_kernel(RhArgs a) {
  __shared__ int cnt[RH_COLS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int c0 = blockIdx.x * RH_COLS, v = c0 + tid;
  const int T = a.T, k = a.k;
  if (k > 0) {
    cnt[tid] = 0;
    __syncthreads();
    const long long o = (long long)b * T * k;
    for (int i = tid; i < T * k; i += RH_COLS) {
      const int id = a.ids[o + i];
      if (id >= c0 && id < c0 + RH_COLS && rh_ld<DT>(a.w, o + i) > 0.f) atomicAdd(&cnt[id - c0], 1);  // integer: order-free
    }
    __syncthreads();
  }
  if (v >= a.V) return;
  const uint8_t* __restrict__ mrow = a.mask + (long long)b * a.T1 + a.skip;
  const float* __restrict__ lse = a.lse + (long long)b * T;
  const long long base = (long long)b * a.sb + (long long)a.skip * a.st + v;
  const bool soft = a.want_soft != 0;
  float best = -1.f, sp = 0.f;  // f >= 0: token 0 always takes the lead, a later token only with a strictly larger f
  int arg = 0;
  int t = 0;
  for (; t + 4 <= T; t += 4) {
    float x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = rh_ld<DT>(a.x, base + (long long)(t + u) * a.st);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float f = mrow[t + u] ? rh_f(x[u]) : 0.f;
      if (f > best) { best = f; arg = t + u; }
      if (soft) sp += expf(x[u] - lse[t + u]);
    }
  }
  for (; t < T; ++t) {
    const float x = rh_ld<DT>(a.x, base + (long long)t * a.st);
    const float f = mrow[t] ? rh_f(x) : 0.f;
    if (f > best) { best = f; arg = t; }
    if (soft) sp += expf(x - lse[t]);
  }
  const long long o = (long long)b * a.V + v;
  rh_st<DT>(a.repr, o, best);
  a.arg[o] = arg;
  if (k > 0) rh_st<DT>(a.rmask, o, (float)cnt[tid]);
  if (soft) rh_st<DT>(a.ssum, o, sp);
}

// dlogits from g_repr and / or g_w alone: a thread owns a column over RH_BWD_ROWS rows of dlogits; the logits are read only where a
// gradient lands (one token per column for g_repr, k columns per token for g_w).  grid (ceil(V / RH_COLS), ceil(T1 / RH_BWD_ROWS), B).
template <int DT>
__global__ __launch_bounds__(RH_COLS) void rh_bwd_sparse_kernel(RhArgs a) {
  const int b = blockIdx.z, v = blockIdx.x * RH_COLS + threadIdx.x;
  if (v >= a.V) return;
  const int k = a.g_w ? a.k : 0;
  const long long ov = (long long)b * a.V + v;
  const float gr = a.g_repr ? a.g_repr[ov] : 0.f;
  const int arg = a.g_repr ? a.arg[ov] : -1;
  const int r0 = blockIdx.y * RH_BWD_ROWS;
  const int r1 = min(r0 + RH_BWD_ROWS, a.T1);
  for (int r = r0; r < r1; ++r) {
    const int t = r - a.skip;
    float out = 0.f;
    if (t >= 0 && a.mask[(long long)b * a.T1 + r] != 0) {
      float wsum = 0.f;
      bool hit = t == arg;
      const long long o = ((long long)b * a.T + t) * k;
      for (int j = 0; j < k; ++j)
        if (a.ids[o + j] == v) { wsum += a.g_w[o + j]; hit = true; }
      if (hit) {
        const float df = rh_df(rh_ld<DT>(a.x, (long long)b * a.sb + (long long)r * a.st + v));
        out = (t == arg ? gr * df : 0.f) + wsum * df;
      }
    }
    rh_st<DT>(a.dx, ((long long)b * a.T1 + r) * a.V + v, out);
  }
}

// dlogits with the softmax gradient: one workgroup per row of dlogits (skipped rows are zeroed), grid B * T1.  The register-resident
// form is built up to NPT = 4 only: at 32 values per thread next to g_soft, argmax and g_repr it spills under the 128 registers of a
// 1024-thread workgroup, so wide rows take NPT = 0 and read the row a second time (it was read microseconds ago: L2 / MALL).
template <int DT, int NPT>
__global__ __launch_bounds__(RH_THREADS) void rh_bwd_row_kernel(RhArgs a) {
  __shared__ float sh[RH_WAVES];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int b = row / a.T1, r = row - b * a.T1;
  const int t = r - a.skip, V = a.V;
  const long long orow = (long long)row * V;
  constexpr int UNR = NPT ? NPT : 1;  // the register-resident row is walked fully unrolled, the re-read one not at all
  const int nit = NPT ? NPT : (V + RH_THREADS - 1) / RH_THREADS;
  if (t < 0) {
    for (int i = 0; i < nit; ++i) {
      const int v = tid + i * RH_THREADS;
      if (v < V) rh_st<DT>(a.dx, orow + v, 0.f);
    }
    return;
  }
  const long long base = (long long)b * a.sb + (long long)r * a.st;
  const bool live = a.mask[(long long)b * a.T1 + r] != 0;
  const float lse = a.lse[(long long)b * a.T + t];
  const float* __restrict__ gs = a.g_soft + (long long)b * V;
  float xv[NPT ? NPT : 1];
  if constexpr (NPT > 0) {
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int v = tid + i * RH_THREADS;
      xv[i] = v < V ? rh_ld<DT>(a.x, base + v) : -INFINITY;
    }
  }
  auto val = [&](int i, int v) -> float {
    if constexpr (NPT > 0) return xv[i];
    else return v < V ? rh_ld<DT>(a.x, base + v) : -INFINITY;
  };
  float dot = 0.f;
#pragma unroll UNR
  for (int i = 0; i < nit; ++i) {
    const int v = tid + i * RH_THREADS;
    if (v < V) dot += expf(val(i, v) - lse) * gs[v];
  }
  dot = rh_block_sum(dot, sh);
  const int k = a.g_w ? a.k : 0;
  const long long ok = ((long long)b * a.T + t) * k;
  int id[RH_KMAX];
  float gw[RH_KMAX];
#pragma unroll
  for (int j = 0; j < RH_KMAX; ++j) {
    id[j] = j < k ? a.ids[ok + j] : -1;
    gw[j] = j < k ? a.g_w[ok + j] : 0.f;
  }
#pragma unroll UNR
  for (int i = 0; i < nit; ++i) {
    const int v = tid + i * RH_THREADS;
    if (v >= V) continue;
    const float x = val(i, v);
    float sparse = 0.f;
    if (live) {
      const float df = rh_df(x);
      float wsum = 0.f;
#pragma unroll
      for (int j = 0; j < RH_KMAX; ++j) wsum += id[j] == v ? gw[j] : 0.f;
      const float gr = (a.g_repr && a.arg[(long long)b * V + v] == t) ? a.g_repr[(long long)b * V + v] : 0.f;
      sparse = gr * df + wsum * df;
    }
    rh_st<DT>(a.dx, orow + v, sparse + expf(x - lse) * (gs[v] - dot));
  }
}

}  // namespace dprhot
