// valu_issue_probe -- what does one vector instruction cost a SIMD to issue, alone and with four waves sharing the SIMD?  The shared row
// softmax of the batch-32 step's second launch (csrc/step_small.h, ss_row_softmax) runs on sixteen waves per CU with nothing to wait
// for once its slabs are there: its time is its instructions' issue cycles, and their prices are not uniform.
// One 1024-thread workgroup per CU (100 KiB of LDS each, so that two never share a CU) on 100 CUs.  Every timed wave runs ITERS turns
// of a loop whose body is 64 independent instances of ONE instruction (or of one short pattern) in a single asm statement, between two
// pairs of stamps (s_memtime shader cycles and the 100 MHz wall clock); the same loop with an empty body is subtracted.  At "one wave per
// SIMD" waves 4-15 of the workgroup leave before the start barrier, at "four" all sixteen run.  ASSUMED, not read from HW_ID: waves
// 0-3 of a workgroup are placed on the four SIMDs of the CU in turn (two of them on one SIMD would show as 8 cycles for an instruction
// that costs 4: every 4.0 in the table's first half speaks for the assumption).
// Printed per instruction: cycles per instruction as one wave sees them, and per SIMD (the wave's figure over the waves sharing the
// SIMD).  The "chain" rows are DEPENDENT sequences as the softmax has them (a DPP operand read needs two wait states behind the VALU
// write: the s_nop 1 is part of the price).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 scratch/valu_issue_probe.hip -o scratch/valu_issue_probe
//   scratch/valu_issue_probe [iters = 2000]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int NWG = 100, NWAVE = 16;
struct Rec { unsigned long long cyc, wall; };

#define X8(f) f(d0) f(d1) f(d2) f(d3) f(d4) f(d5) f(d6) f(d7)
#define X64(f) X8(f) X8(f) X8(f) X8(f) X8(f) X8(f) X8(f) X8(f)
#define P4(f) f(p0) f(p1) f(p2) f(p3)
#define P64(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f) P4(f)
#define DPPC " row_mask:0xf bank_mask:0xf"

#define F_ADD(d) "v_add_f32 %[" #d "], %[a], %[b]\n"
#define F_MUL(d) "v_mul_f32 %[" #d "], %[a], %[b]\n"
#define F_FMA(d) "v_fma_f32 %[" #d "], %[a], %[b], %[b]\n"
#define F_PKADD(d) "v_pk_add_f32 %[" #d "], %[pa], %[pb]\n"
#define F_PKMUL(d) "v_pk_mul_f32 %[" #d "], %[pa], %[pb]\n"
#define F_PKFMA(d) "v_pk_fma_f32 %[" #d "], %[pa], %[pb], %[pb]\n"
#define F_EXP(d) "v_exp_f32 %[" #d "], %[a]\n"
#define F_RCP(d) "v_rcp_f32 %[" #d "], %[a]\n"
#define F_CMPCND(d) "v_cmp_eq_u32 vcc, %[a], %[b]\ns_nop 1\nv_cndmask_b32 %[" #d "], %[a], %[b], vcc\n"  /* as hipcc pads the adjacent pair */
#define F_MAX3(d) "v_max3_f32 %[" #d "], %[a], %[b], %[b]\n"
#define F_MAX(d) "v_max_f32 %[" #d "], %[a], %[b]\n"
#define F_MAXDPP(d) "v_max_f32_dpp %[" #d "], %[a], %[b] row_ror:8" DPPC "\n"
#define F_ADDDPP(d) "v_add_f32_dpp %[" #d "], %[a], %[b] row_ror:8" DPPC "\n"
#define F_CVTBF(d) "v_cvt_pk_bf16_f32 %[" #d "], %[a], %[b]\n"
#define F_NOP1(d) "s_nop 1\n"
#define F_VNOP(d) "v_nop\n"
// four compares into four scalar pairs, then the four selects: no pad needed (what a scheduled select stream can reach)
#define CMPCND4(x, y, z, w) "v_cmp_eq_u32 s[40:41], %[a], %[b]\nv_cmp_eq_u32 s[42:43], %[a], %[b]\nv_cmp_eq_u32 s[44:45], %[a], %[b]\nv_cmp_eq_u32 s[46:47], %[a], %[b]\n" \
  "v_cndmask_b32 %[" #x "], %[a], %[b], s[40:41]\nv_cndmask_b32 %[" #y "], %[a], %[b], s[42:43]\nv_cndmask_b32 %[" #z "], %[a], %[b], s[44:45]\nv_cndmask_b32 %[" #w "], %[a], %[b], s[46:47]\n"
#define CMPCND8 CMPCND4(d0, d1, d2, d3) CMPCND4(d4, d5, d6, d7)
#define UB4(x, y, z, w) "v_cvt_f32_ubyte0 %[" #x "], %[a]\nv_cvt_f32_ubyte1 %[" #y "], %[a]\nv_cvt_f32_ubyte2 %[" #z "], %[a]\nv_cvt_f32_ubyte3 %[" #w "], %[a]\n"
#define UB8 UB4(d0, d1, d2, d3) UB4(d4, d5, d6, d7)
// the swap reads what a swap four places ahead wrote: outside the two wait states of the VALU-write -> permlane-read rule
#define SWAP4 "v_permlane16_swap_b32 %[d0], %[d1]\nv_permlane16_swap_b32 %[d2], %[d3]\nv_permlane16_swap_b32 %[d4], %[d5]\nv_permlane16_swap_b32 %[d6], %[d7]\n"
#define SWAP8 SWAP4 SWAP4
// mixed pairs of the softmax: one exponential among three adds; a packed product between scalar adds
#define EXPADD4(x, y, z, w) "v_exp_f32 %[" #x "], %[a]\nv_add_f32 %[" #y "], %[a], %[b]\nv_add_f32 %[" #z "], %[a], %[b]\nv_add_f32 %[" #w "], %[a], %[b]\n"
#define EXPADD8 EXPADD4(d0, d1, d2, d3) EXPADD4(d4, d5, d6, d7)
#define PKADD2(p, x) "v_pk_mul_f32 %[" #p "], %[pa], %[pb]\nv_add_f32 %[" #x "], %[a], %[b]\n"
#define PKADD8 PKADD2(p0, d0) PKADD2(p1, d1) PKADD2(p2, d2) PKADD2(p3, d3)
// dependent chains, one step = one row rotation of a 16-lane reduction
#define CH_ADD(d) "s_nop 1\nv_add_f32_dpp %[" #d "], %[" #d "], %[" #d "] row_ror:8" DPPC "\n"
#define CH_MAX1(d) "s_nop 1\nv_max_f32_dpp %[" #d "], %[" #d "], %[" #d "] row_ror:8" DPPC "\n"
#define CH_MAX3(d) "s_nop 1\nv_mov_b32_dpp %[d7], %[" #d "] row_ror:8" DPPC "\nv_max_f32 %[d7], %[d7], %[d7]\nv_max_f32 %[" #d "], %[" #d "], %[d7]\n"
#define CH8(f) f(d0) f(d0) f(d0) f(d0) f(d0) f(d0) f(d0) f(d0)
#define R8(s) s s s s s s s s

#define PROBE(name, BODY)                                                                                                              \
  __global__ __launch_bounds__(1024) void k_##name(Rec* out, int iters, int waves) {                                                   \
    const int wave = threadIdx.x >> 6;                                                                                                  \
    if (wave >= waves) return;                                                                                                          \
    float d0 = threadIdx.x, d1 = 1.f, d2 = 2.f, d3 = 3.f, d4 = 4.f, d5 = 5.f, d6 = 6.f, d7 = 7.f, a = 1.5f, b = 0.25f;                  \
    f2 p0 = {0.f, 1.f}, p1 = {2.f, 3.f}, p2 = {4.f, 5.f}, p3 = {6.f, 7.f}, pa = {1.5f, 0.5f}, pb = {0.25f, 0.75f};                      \
    asm volatile("" : "+v"(a), "+v"(b), "+v"(pa), "+v"(pb));                                                                            \
    __syncthreads();                                                                                                                    \
    const unsigned long long c0 = clock64(), w0 = wall_clock64();                                                                       \
    for (int it = 0; it < iters; ++it)                                                                                                  \
      asm volatile(BODY : [d0] "+v"(d0), [d1] "+v"(d1), [d2] "+v"(d2), [d3] "+v"(d3), [d4] "+v"(d4), [d5] "+v"(d5), [d6] "+v"(d6),      \
                   [d7] "+v"(d7), [p0] "+v"(p0), [p1] "+v"(p1), [p2] "+v"(p2), [p3] "+v"(p3)                                            \
                   : [a] "v"(a), [b] "v"(b), [pa] "v"(pa), [pb] "v"(pb)                                                                 \
                   : "vcc", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47");                                                   \
    const unsigned long long c1 = clock64(), w1 = wall_clock64();                                                                       \
    if ((threadIdx.x & 63) == 0) {                                                                                                      \
      out[blockIdx.x * NWAVE + wave].cyc = c1 - c0;                                                                                     \
      out[blockIdx.x * NWAVE + wave].wall = w1 - w0;                                                                                    \
    }                                                                                                                                   \
    if (d0 + d1 + d2 + d3 + d4 + d5 + d6 + d7 + p0[0] + p0[1] + p1[0] + p1[1] + p2[0] + p2[1] + p3[0] + p3[1] == 12345.678f)            \
      out[0].cyc = 0;                                                                                                                   \
  }

PROBE(empty, "")
PROBE(add, X64(F_ADD))
PROBE(mul, X64(F_MUL))
PROBE(fma, X64(F_FMA))
PROBE(pkadd, P64(F_PKADD))
PROBE(pkmul, P64(F_PKMUL))
PROBE(pkfma, P64(F_PKFMA))
PROBE(exp, X64(F_EXP))
PROBE(rcp, X64(F_RCP))
PROBE(cmpcnd, X64(F_CMPCND))
PROBE(cmpcnd4, R8(CMPCND8))
PROBE(max3, X64(F_MAX3))
PROBE(max, X64(F_MAX))
PROBE(maxdpp, X64(F_MAXDPP))
PROBE(adddpp, X64(F_ADDDPP))
PROBE(swap, R8(SWAP8))
PROBE(cvtbf, X64(F_CVTBF))
PROBE(ubyte, R8(UB8))
PROBE(nop1, X64(F_NOP1))
PROBE(vnop, X64(F_VNOP))
PROBE(expadd, R8(EXPADD8))
PROBE(pkscalar, R8(PKADD8))
PROBE(ch_add, R8(CH8(CH_ADD)))
PROBE(ch_max1, R8(CH8(CH_MAX1)))
PROBE(ch_max3, R8(CH8(CH_MAX3)))

typedef void (*Kern)(Rec*, int, int);
struct Row { const char* name; Kern k; int per_iter; const char* unit; };

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 2000;
  const Row rows[] = {
      {"v_add_f32", k_add, 64, "instruction"},
      {"v_mul_f32", k_mul, 64, "instruction"},
      {"v_fma_f32", k_fma, 64, "instruction"},
      {"v_pk_add_f32", k_pkadd, 64, "instruction"},
      {"v_pk_mul_f32", k_pkmul, 64, "instruction"},
      {"v_pk_fma_f32", k_pkfma, 64, "instruction"},
      {"v_exp_f32", k_exp, 64, "instruction"},
      {"v_rcp_f32", k_rcp, 64, "instruction"},
      {"v_cmp_eq_u32 vcc + s_nop 1 + v_cndmask_b32", k_cmpcnd, 64, "pair"},
      {"4 v_cmp_eq_u32 (SGPR pairs) then 4 v_cndmask_b32", k_cmpcnd4, 64, "pair"},
      {"v_max3_f32", k_max3, 64, "instruction"},
      {"v_max_f32", k_max, 64, "instruction"},
      {"v_max_f32_dpp row_ror", k_maxdpp, 64, "instruction"},
      {"v_add_f32_dpp row_ror", k_adddpp, 64, "instruction"},
      {"v_permlane16_swap_b32", k_swap, 64, "instruction"},
      {"v_cvt_pk_bf16_f32", k_cvtbf, 64, "instruction"},
      {"v_cvt_f32_ubyte0..3", k_ubyte, 64, "instruction"},
      {"s_nop 1", k_nop1, 64, "instruction"},
      {"v_nop", k_vnop, 64, "instruction"},
      {"v_exp_f32 + 3 v_add_f32", k_expadd, 16, "group of 4"},
      {"v_pk_mul_f32 + v_add_f32", k_pkscalar, 32, "group of 2"},
      {"chain: s_nop 1 + v_add_f32_dpp", k_ch_add, 64, "step"},
      {"chain: s_nop 1 + v_max_f32_dpp", k_ch_max1, 64, "step"},
      {"chain: s_nop 1 + v_mov_b32_dpp + 2 v_max_f32", k_ch_max3, 64, "step"},
  };
  const size_t lds = 100 * 1024;
  Rec* d;
  CK(hipMalloc(&d, sizeof(Rec) * NWG * NWAVE));
  std::vector<Rec> h(NWG * NWAVE);
  int rate = 0;
  CK(hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, 0));
  // median over every timed wave of the third of three launches
  auto run = [&](Kern k, int waves, double& cyc, double& ns) -> int {
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int rep = 0; rep < 3; ++rep) {
      CK(hipMemset(d, 0, sizeof(Rec) * NWG * NWAVE));
      hipLaunchKernelGGL(k, dim3(NWG), dim3(1024), lds, 0, d, iters, waves);
      CK(hipGetLastError());
      CK(hipDeviceSynchronize());
    }
    CK(hipMemcpy(h.data(), d, sizeof(Rec) * NWG * NWAVE, hipMemcpyDeviceToHost));
    std::vector<double> c, w;
    for (int b = 0; b < NWG; ++b)
      for (int v = 0; v < waves; ++v) { c.push_back((double)h[b * NWAVE + v].cyc); w.push_back((double)h[b * NWAVE + v].wall); }
    std::sort(c.begin(), c.end());
    std::sort(w.begin(), w.end());
    cyc = c[c.size() / 2];
    ns = w[w.size() / 2] * 1e6 / rate;
    return 0;
  };
  printf("valu_issue_probe: %d workgroups x 1024 threads, %d turns of the loop, wall clock %d kHz; medians over the timed waves\n", NWG, iters, rate);
  printf("cycles = s_memtime ticks, ns = wall clock; empty loop subtracted; per SIMD = per wave / waves on the SIMD\n");
  double ecyc[2], ens[2];
  for (int o = 0; o < 2; ++o) {
    if (run(k_empty, o ? 16 : 4, ecyc[o], ens[o])) return 1;
    printf("empty loop, %d wave(s) per SIMD: %.0f cycles, %.0f ns (%.2f cycles per turn)\n", o ? 4 : 1, ecyc[o], ens[o], ecyc[o] / iters);
  }
  printf("%-50s %-12s | %28s | %40s\n", "", "", "one wave per SIMD", "four waves per SIMD");
  printf("%-50s %-12s | %9s %9s %8s | %9s %9s %9s %8s\n", "instruction", "per", "cyc/wave", "ns/wave", "MHz", "cyc/wave", "cyc/SIMD", "ns/SIMD", "MHz");
  for (const Row& r : rows) {
    double cyc[2], ns[2];
    for (int o = 0; o < 2; ++o)
      if (run(r.k, o ? 16 : 4, cyc[o], ns[o])) return 1;
    const double n = (double)iters * r.per_iter;
    const double c1 = (cyc[0] - ecyc[0]) / n, n1 = (ns[0] - ens[0]) / n, c4 = (cyc[1] - ecyc[1]) / n, n4 = (ns[1] - ens[1]) / n;
    printf("%-50s %-12s | %9.2f %9.3f %8.0f | %9.2f %9.2f %9.3f %8.0f\n", r.name, r.unit, c1, n1, cyc[0] / ns[0] * 1e3, c4, c4 / 4, n4 / 4, cyc[1] / ns[1] * 1e3);
  }
  return 0;
}
