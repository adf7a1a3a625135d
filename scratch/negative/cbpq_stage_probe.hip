// cbpq_stage_probe.hip -- form (a) of DESIGN.md section 12.1 against the kernel that ships (form (b)), stand-alone.
//
// Form (a): the codes are decoded WHILE THE TILE IS STAGED -- every 16-byte piece of a decoded row is assembled once per workgroup
// (code bytes from global memory, codebook rows from LDS) and written into cb_score_kernel's padded bf16 tile; the inner loop is the
// dense kernel's.  Same workgroup (8 waves, 32 query fragments, one pass), same codebook in LDS, same term table, same owner: the only
// difference to cbpq_score_kernel is where the decode happens.  Both kernels score the same synthetic index (uniform random codes, a
// random bf16 codebook, passages of 1 .. 12 blocks) with 32 x 32 queries; S must agree byte for byte; times by device events.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../dpr_scale_amd/csrc cbpq_stage_probe.hip -o cbpq_stage_probe && ./cbpq_stage_probe
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "colbert_pq.h"

using namespace dprhot;

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      std::printf("%s: %s\n", #x, hipGetErrorString(e_));                      \
      std::exit(1);                                                            \
    }                                                                          \
  } while (0)

template <int DSUB, int KS>
__global__ __launch_bounds__(CBPQ_THREADS) void cbpq_stage_kernel(CbPqArgs p) {
  constexpr int DP = KS * 32, MSUB = DP / DSUB, CPR = KS * 4, ROWB = DP * 2 + 16;
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ long long off[CB_RUNP + 1];
  uint16_t* CBK = reinterpret_cast<uint16_t*>(lds);
  unsigned char* tile = lds + DP * 512;  // [TB][16] rows of ROWB bytes
  const int tstride = p.QPW * p.FQ * 16 + 1;
  float* T = reinterpret_cast<float*>(tile + CB_TILE_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g4 = lane >> 4;
  for (int i = tid; i < DP * 32; i += CBPQ_THREADS) reinterpret_cast<ivf_i32x4*>(CBK)[i] = reinterpret_cast<const ivf_i32x4*>(p.cb)[i];
  const int q0 = (int)blockIdx.y * p.QPW;
  const int nql = p.nq - q0 < p.QPW ? p.nq - q0 : p.QPW;
  const int F = nql * p.FQ;
  const int nfr = F - wave > 0 ? (F - wave + CBPQ_WAVES - 1) / CBPQ_WAVES : 0;
  int fr[CB_QW];
  cb_bf16x8 bq[CB_QW][KS];
  float m[CB_QW];
#pragma unroll
  for (int i = 0; i < CB_QW; ++i) {
    fr[i] = i * CBPQ_WAVES + wave;
    const bool fok = fr[i] < F;
    const int ql = fok ? fr[i] / p.FQ : 0;
    const int t = (fok ? fr[i] - ql * p.FQ : 0) * 16 + i16;
    const bool bok = fok && t < p.LQ;
    const uint16_t* qp = p.q + ((long long)(q0 + ql) * p.LQ + (bok ? t : 0)) * DP + g4 * 8;
    m[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bq[i][ks] = cb_load8(qp + ks * 32, bok);
  }
  const int nruns = (p.cols + CB_RUNP - 1) / CB_RUNP;
  const int run0 = (int)blockIdx.x * p.RPW, run1 = run0 + p.RPW < nruns ? run0 + p.RPW : nruns;
  for (int run = run0; run < run1; ++run) {
    const int pl0 = run * CB_RUNP;
    const int np = p.cols - pl0 < CB_RUNP ? p.cols - pl0 : CB_RUNP;
    if (tid <= np) {
      long long v = p.dblk[p.D0 + pl0 + tid];
      off[tid] = v < 0 ? 0 : v > p.n_blk ? p.n_blk : v;
    }
    __syncthreads();
    if (tid == 0)
      for (int i = 1; i <= np; ++i)
        if (off[i] < off[i - 1]) off[i] = off[i - 1];
    __syncthreads();
    const long long b0 = off[0], b1 = off[np];
    auto finish = [&](int pl) {
#pragma unroll
      for (int i = 0; i < CB_QW; ++i)
        if (i < nfr) {
          float v = m[i];
          v = fmaxf(v, __shfl_xor(v, 16, 64));
          v = fmaxf(v, __shfl_xor(v, 32, 64));
          if (lane < 16) T[pl * tstride + fr[i] * 16 + lane] = v;
          m[i] = 0.f;
        }
    };
    int pl = 0;
    long long nxt = off[1];
    for (long long t0 = b0; t0 < b1; t0 += p.TB) {
      const int nb = (int)(b1 - t0 < p.TB ? b1 - t0 : p.TB);
      __syncthreads();
      for (int c = tid; c < nb * 16 * CPR; c += CBPQ_THREADS) {  // decode while staging: one 16-byte piece of a decoded row per step
        const int r = c / CPR, k = c - r * CPR;
        const bool rok = (r & 15) < (int)p.rows[t0 + (r >> 4)];
        *reinterpret_cast<cb_bf16x8*>(tile + r * ROWB + k * 16) = ivf_pq_frag<DSUB>(p.code + (t0 * 16 + r) * MSUB, CBK, k * 8 / DSUB, rok);
      }
      __syncthreads();
      if (nfr > 0)
        for (int bl = 0; bl < nb; ++bl) {
          while (t0 + bl >= nxt) {
            finish(pl);
            ++pl;
            nxt = off[pl + 1];
          }
          const unsigned char* arow = tile + (bl * 16 + i16) * ROWB + g4 * 16;
          cb_bf16x8 a[KS];
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) a[ks] = *reinterpret_cast<const cb_bf16x8*>(arow + ks * 64);
          cb_f32x4 acc[CB_QW];
#pragma unroll
          for (int i = 0; i < CB_QW; ++i) {
            acc[i] = cb_f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < nfr) {
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], bq[i][ks], acc[i], 0, 0, 0);
            }
          }
#pragma unroll
          for (int i = 0; i < CB_QW; ++i) m[i] = fmaxf(m[i], fmaxf(fmaxf(acc[i][0], acc[i][1]), fmaxf(acc[i][2], acc[i][3])));
        }
    }
    while (pl < np) {
      finish(pl);
      ++pl;
    }
    __syncthreads();
    for (int t = tid; t < np * nql; t += CBPQ_THREADS) {
      const int ql = t / np, pc = t - ql * np;
      const float* tt = T + pc * tstride + ql * p.FQ * 16;
      float acc = tt[0];
      for (int i = 1; i < p.LQ; ++i) acc = p.pool ? fmaxf(acc, tt[i]) : acc + tt[i];
      p.S[(long long)(q0 + ql) * p.ld + pl0 + pc] = acc;
    }
  }
}

static uint32_t rng = 12345u;
static uint32_t next() {
  rng = rng * 1664525u + 1013904223u;
  return rng >> 8;
}

template <int DSUB>
static int run(int docs) {
  constexpr int KS = 4, DP = 128, MSUB = DP / DSUB, NQ = 32, LQ = 32, COLS = 65536;
  std::vector<long long> dblk(docs + 1, 0);
  for (int i = 0; i < docs; ++i) dblk[i + 1] = dblk[i] + 1 + next() % 12;
  const long long n_blk = dblk[docs];
  std::vector<uint8_t> code((size_t)n_blk * 16 * MSUB), rows(n_blk);
  for (auto& c : code) c = (uint8_t)next();
  for (auto& r : rows) r = (uint8_t)(1 + next() % 16);
  std::vector<uint16_t> cb((size_t)DP * 256), q((size_t)NQ * LQ * DP);
  auto bf = [] { return (uint16_t)(0x3c00u + (next() & 0x81ffu)); };  // +-(2^-7 .. 2^-6): finite, both signs
  for (auto& v : cb) v = bf();
  for (auto& v : q) v = bf();
  uint8_t *dcode, *drows;
  uint16_t *dcb, *dq;
  long long* ddblk;
  float *S1, *S2;
  CK(hipMalloc(&dcode, code.size()));
  CK(hipMalloc(&drows, rows.size()));
  CK(hipMalloc(&dcb, cb.size() * 2));
  CK(hipMalloc(&dq, q.size() * 2));
  CK(hipMalloc(&ddblk, dblk.size() * 8));
  CK(hipMalloc(&S1, (size_t)NQ * docs * 4));
  CK(hipMalloc(&S2, (size_t)NQ * docs * 4));
  CK(hipMemcpy(dcode, code.data(), code.size(), hipMemcpyHostToDevice));
  CK(hipMemcpy(drows, rows.data(), rows.size(), hipMemcpyHostToDevice));
  CK(hipMemcpy(dcb, cb.data(), cb.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(dq, q.data(), q.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(ddblk, dblk.data(), dblk.size() * 8, hipMemcpyHostToDevice));
  const int FQ = LQ / 16, QPW = CBPQ_FPP / FQ, gy = (NQ + QPW - 1) / QPW;
  const size_t table = (size_t)CB_RUNP * (QPW * FQ * 16 + 1) * 4;
  const size_t lds_b = (size_t)DP * 512 + CBPQ_TILE_BYTES + CBPQ_TILE_BLOCKS + table, lds_a = (size_t)DP * 512 + CB_TILE_BYTES + table;
  const int TB_b = std::min(CBPQ_TILE_BYTES / (16 * MSUB), CBPQ_TILE_BLOCKS), TB_a = CB_TILE_BYTES / (16 * (DP * 2 + 16));
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(cbpq_score_kernel<DSUB, KS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(cbpq_stage_kernel<DSUB, KS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a));
  auto pass = [&](bool stage, float* S) {
    for (long long j0 = 0; j0 < docs; j0 += COLS) {
      const int cols = (int)std::min<long long>(COLS, docs - j0);
      const long long wgs = (long long)((cols + CB_RUNP - 1) / CB_RUNP) * gy;
      const int RPW = (int)std::max<long long>(1, std::min<long long>(CBPQ_MAX_RPW, wgs / 1024));
      CbPqArgs a{dcode, drows, dcb, ddblk, n_blk, dq, NQ, LQ, 0, j0, cols, S + j0, (long long)docs, FQ, QPW, stage ? TB_a : TB_b, RPW};
      const dim3 grid((unsigned)(((cols + CB_RUNP - 1) / CB_RUNP + RPW - 1) / RPW), (unsigned)gy);
      if (stage)
        hipLaunchKernelGGL((cbpq_stage_kernel<DSUB, KS>), grid, dim3(CBPQ_THREADS), lds_a, 0, a);
      else
        hipLaunchKernelGGL((cbpq_score_kernel<DSUB, KS>), grid, dim3(CBPQ_THREADS), lds_b, 0, a);
    }
  };
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<float> tb, ta;
  for (int it = 0; it < 12; ++it)
    for (int stage = 0; stage < 2; ++stage) {  // the two forms alternate
      CK(hipEventRecord(e0));
      pass(stage, stage ? S2 : S1);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      CK(hipGetLastError());
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (it >= 2) (stage ? ta : tb).push_back(ms);
    }
  std::vector<float> h1((size_t)NQ * docs), h2(h1.size());
  CK(hipMemcpy(h1.data(), S1, h1.size() * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(h2.data(), S2, h2.size() * 4, hipMemcpyDeviceToHost));
  const bool same = std::memcmp(h1.data(), h2.data(), h1.size() * 4) == 0;
  std::sort(tb.begin(), tb.end());
  std::sort(ta.begin(), ta.end());
  std::printf("{\"probe\": \"cbpq_stage\", \"dsub\": %d, \"docs\": %d, \"n_blk\": %lld, \"S_equal\": %s, \"form_b_ms\": [%.3f, %.3f, %.3f], "
              "\"form_a_ms\": [%.3f, %.3f, %.3f]}\n",
              DSUB, docs, n_blk, same ? "true" : "false", tb[0], tb[tb.size() / 2], tb.back(), ta[0], ta[ta.size() / 2], ta.back());
  hipFree(dcode), hipFree(drows), hipFree(dcb), hipFree(dq), hipFree(ddblk), hipFree(S1), hipFree(S2);
  return same ? 0 : 1;
}

int main() {
  int rc = 0;
  rc |= run<8>(100000);
  rc |= run<4>(100000);
  rc |= run<2>(100000);
  return rc;
}
