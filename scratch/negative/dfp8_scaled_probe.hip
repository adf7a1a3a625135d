// A/B of the two fp8 MFMA forms under the tile of csrc/dense_fp8.h, store epilogue, one process, arms alternating:
//
//   arm 0  v_mfma_f32_16x16x32_fp8_fp8           4 per block pair and 128-deep K step, 8 code bytes per lane each (the shipped form)
//   arm 1  v_mfma_scale_f32_16x16x128_f8f6f4     1 per block pair and K step, 32 code bytes per lane, both scale operands 127 (= 1.0)
//
// The scaled form takes features 32 (l >> 4) .. + 32 of the step from lane l (two 16-byte chunks of the image: two ds_read_b128 per
// block and step instead of four ds_read_b64).  Both arms are first held against a host computation on integer-grid codes, where every
// sum is exact whatever the order: that check is what pins the scaled form's operand map.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I ../../dpr_scale_amd/csrc dfp8_scaled_probe.hip -o dfp8_scaled_probe && ./dfp8_scaled_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "dense_fp8.h"

using namespace dprhot;

typedef int i32x8 __attribute__((ext_vector_type(8)));

#define CHECK(x)                                                                         \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                            \
      exit(2);                                                                           \
    }                                                                                    \
  } while (0)

// dfp8_kernel<false, TM> with the MFMA form as a template parameter; everything else as in dense_fp8.h
template <int TM, bool SCALED>
__global__ __launch_bounds__(256) void probe_kernel(Dfp8Args p) {
  constexpr int NA = TM / 32;
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
  const uint8_t* ga[4];
  const uint8_t* gb[4];
  int kc[4], so[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
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
      const bool ok = t * F8_BK + kc[j] < K;
      if (j < NA) ra[j] = ok ? *reinterpret_cast<const uint4*>(ga[j] + t * F8_BK) : uint4{0u, 0u, 0u, 0u};
      rb[j] = ok ? *reinterpret_cast<const uint4*>(gb[j] + t * F8_BK) : uint4{0u, 0u, 0u, 0u};
    }
  };
  fetch(0);
  for (int t = 0; t < nt; ++t) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < NA) *reinterpret_cast<uint4*>(As + so[j]) = ra[j];
      *reinterpret_cast<uint4*>(Bs + so[j]) = rb[j];
    }
    __syncthreads();
    if (t + 1 < nt) fetch(t + 1);
    if constexpr (!SCALED) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
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
    } else {
      i32x8 af[NA], bfr[4];  // features 32 g .. + 32 of the step: chunks 2 g and 2 g + 1
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int row = wm * (TM / 2) + a * 16 + i;
        const uint4 lo = *reinterpret_cast<const uint4*>(As + row * F8_BK + (((2 * g) ^ ((row >> 1) & 7)) << 4));
        const uint4 hi = *reinterpret_cast<const uint4*>(As + row * F8_BK + (((2 * g + 1) ^ ((row >> 1) & 7)) << 4));
        af[a] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int row = wn * 64 + b * 16 + i;
        const uint4 lo = *reinterpret_cast<const uint4*>(Bs + row * F8_BK + (((2 * g) ^ ((row >> 1) & 7)) << 4));
        const uint4 hi = *reinterpret_cast<const uint4*>(Bs + row * F8_BK + (((2 * g + 1) ^ ((row >> 1) & 7)) << 4));
        bfr[b] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
      }
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[a], bfr[b], acc[a][b], 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
    }
  }
  const int mw = m0 + wm * (TM / 2) + g * 4, nw = n0 + wn * 64 + i;
  float sc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) sc[b] = p.cs[min(nw + b * 16, p.cols - 1)];
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
}

static float code_value(uint8_t c) {
  const int s = c >> 7, e = (c >> 3) & 15, m = c & 7;
  const float mag = e == 0 ? m / 8.0f * 0.015625f : (1.0f + m / 8.0f) * exp2f((float)(e - 7));
  return s ? -mag : mag;
}

template <int TM, bool SCALED>
static void run(const Dfp8Args& a) {
  hipLaunchKernelGGL((probe_kernel<TM, SCALED>), dim3((a.cols + F8_B - 1) / F8_B, (a.nq + TM - 1) / TM), dim3(256), 0, 0, a);
}
static void run_arm(int arm, const Dfp8Args& a) {
  if (a.nq <= 32) arm ? run<32, true>(a) : run<32, false>(a);
  else arm ? run<128, true>(a) : run<128, false>(a);
}

int main() {
  const int dp = 768, ncols = 131072, nqmax = 1024;
  // integer and half code values in [-4, 4] for the check, every non-NaN code for the timing (the time does not depend on the values)
  std::vector<uint8_t> gridc;
  for (int c = 0; c < 256; ++c) {
    if (((c >> 3) & 15) == 15 && (c & 7) == 7) continue;
    const float v = code_value((uint8_t)c);
    if (v >= -4.f && v <= 4.f && v * 2 == (float)(int)(v * 2)) gridc.push_back((uint8_t)c);
  }
  std::vector<uint8_t> hq((size_t)nqmax * dp), hc((size_t)ncols * dp);
  std::vector<float> hqs(nqmax), hcs(ncols);
  uint32_t s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  for (auto& x : hq) x = gridc[rnd() % gridc.size()];
  for (auto& x : hc) x = gridc[rnd() % gridc.size()];
  for (auto& x : hqs) x = exp2f((float)((int)(rnd() % 9) - 3));
  for (auto& x : hcs) x = exp2f((float)((int)(rnd() % 9) - 3));
  uint8_t *dq, *dc;
  float *dqs, *dcs, *dS;
  CHECK(hipMalloc(&dq, hq.size())); CHECK(hipMalloc(&dc, hc.size()));
  CHECK(hipMalloc(&dqs, nqmax * 4)); CHECK(hipMalloc(&dcs, ncols * 4));
  CHECK(hipMalloc(&dS, (size_t)nqmax * ncols * 4));
  CHECK(hipMemcpy(dq, hq.data(), hq.size(), hipMemcpyHostToDevice)); CHECK(hipMemcpy(dc, hc.data(), hc.size(), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dqs, hqs.data(), nqmax * 4, hipMemcpyHostToDevice)); CHECK(hipMemcpy(dcs, hcs.data(), ncols * 4, hipMemcpyHostToDevice));

  // ---- check: 129 x 1003 cells on the 128-row tile, 17 x 1003 on the 32-row tile, both arms, against the host
  for (int nq : {129, 17}) {
    const int cols = 1003, ld = 1008;
    for (int arm = 0; arm < 2; ++arm) {
      Dfp8Args a{};
      a.Qc = dq; a.qs = dqs; a.Cc = dc; a.cs = dcs; a.nq = nq; a.cols = cols; a.dp = dp; a.S = dS; a.ld = ld;
      CHECK(hipMemset(dS, 0xA5, (size_t)nq * ld * 4));
      run_arm(arm, a);
      CHECK(hipDeviceSynchronize());
      std::vector<float> hS((size_t)nq * ld);
      CHECK(hipMemcpy(hS.data(), dS, hS.size() * 4, hipMemcpyDeviceToHost));
      long bad = 0;
      for (int m = 0; m < nq; ++m)
        for (int n = 0; n < cols; ++n) {
          double acc = 0;
          for (int t = 0; t < dp; ++t) acc += (double)code_value(hq[(size_t)m * dp + t]) * code_value(hc[(size_t)n * dp + t]);
          bad += hS[(size_t)m * ld + n] != (float)(acc * hqs[m] * hcs[n]);
        }
      printf("check nq=%d arm=%d: %ld of %d cells differ from the host\n", nq, arm, bad, nq * cols);
      if (bad) return 1;
    }
  }

  // ---- timing: arms alternate, 3 warm-up + 20 timed rounds
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  for (int nq : {1, 32, 1024}) {
    Dfp8Args a{};
    a.Qc = dq; a.qs = dqs; a.Cc = dc; a.cs = dcs; a.nq = nq; a.cols = ncols; a.dp = dp; a.S = dS; a.ld = ncols;
    std::vector<float> ms[2];
    for (int r = 0; r < 23; ++r)
      for (int arm = 0; arm < 2; ++arm) {
        CHECK(hipEventRecord(e0, 0));
        run_arm(arm, a);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float t;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (r >= 3) ms[arm].push_back(t * 1e3f);
      }
    for (int arm = 0; arm < 2; ++arm) {
      std::sort(ms[arm].begin(), ms[arm].end());
      printf("nq=%4d cols=%d dp=%d arm=%d (%s): median %.1f us (min %.1f - max %.1f)\n", nq, ncols, dp, arm,
             arm ? "16x16x128 f8f6f4, scales 127" : "16x16x32 fp8_fp8", ms[arm][ms[arm].size() / 2], ms[arm].front(), ms[arm].back());
    }
  }
  return 0;
}
