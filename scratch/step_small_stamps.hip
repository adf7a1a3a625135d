// experiment: per-workgroup wall-clock stamps (10 ns ticks) of the batch-32 step's softmax + backward launch, as it is (small_step_roles = 0:
// step_small_kernel, slots = DPRHOT_TM 8..15) and split by role (1 / 2: step_small_kernel_roles; 3: step_small_kernel_out, whose loss
// block has a stamp row of its own, DPRHOT_TMB kind 3, and whose two row-store blocks use kind 0, which form 0 alone uses otherwise).
// Every role's stamp 0 is the first statement of its body.  Also the sim launch's own stamps (sim_small_kernel, workgroup (0, 0, 0):
// DPRHOT_TM 0 / 1 / 4 / 6).  Not shipped.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 scratch/step_small_stamps.hip -o scratch/step_small_stamps
//   scratch/step_small_stamps [Nc = 256] [d = 768] [small_step_roles = 0] [launches = 41] [small_sim_copy = library default]
// Prints, per role: workgroup 0 (the lead), a middle one and the last to finish -- start and end since the launch's first stamp and the
// time between consecutive stamps, each the median over the launches.
// The sim launch is stamped in EVERY workgroup (the tool's own DPRHOT_TM: slots 0..7 go to a row per workgroup, in dispatch order),
// and reported by what the wave copies besides its tile: nothing, Cb (row tile 0), Qb (column tile 0) or both, plus the last wave
// dispatched and the last one to end.
#define DPRHOT_TIMING 1
#include <hip/hip_runtime.h>
__device__ unsigned long long g_dprhot_tm[64];
__device__ unsigned long long g_sim_tm[4096 * 8];
#define DPRHOT_TM(i)                                                                                                 \
  do {                                                                                                               \
    if (threadIdx.x == 0) {                                                                                          \
      if ((i) < 8) {                                                                                                 \
        const unsigned lin_ = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;                        \
        if (lin_ < 4096) g_sim_tm[lin_ * 8 + (i)] = wall_clock64();                                                  \
      } else if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) g_dprhot_tm[i] = wall_clock64();            \
    }                                                                                                                \
  } while (0)
__device__ unsigned long long g_dprhot_tmb[4 * 4096 * 8];
#include "../dpr_scale_amd/csrc/dprhot.hip"
#include <algorithm>
#include <stdio.h>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
static double med(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; }
int main(int argc, char** argv) {
  const int B = 32, Nc = argc > 1 ? atoi(argv[1]) : 256, d = argc > 2 ? atoi(argv[2]) : 768, roles = argc > 3 ? atoi(argv[3]) : 0;
  const int launches = argc > 4 ? atoi(argv[4]) : 41;
  if (dprhot_set_option("small_step_roles", roles)) { printf("%s\n", dprhot_last_error()); return 1; }
  if (argc > 5 && dprhot_set_option("small_sim_copy", atoi(argv[5]))) { printf("%s\n", dprhot_last_error()); return 1; }
  float *q, *c, *dq, *dc; uint16_t *Qb, *Cb, *G; int64_t* y; float *loss, *lse, *sum; void* ws; size_t wsb;
  dprhot_workspace_bytes(B, Nc, d, &wsb);
  CK(hipMalloc(&q, (size_t)B * d * 4)); CK(hipMalloc(&c, (size_t)Nc * d * 4)); CK(hipMalloc(&Qb, (size_t)B * d * 2)); CK(hipMalloc(&Cb, (size_t)Nc * d * 2));
  CK(hipMalloc(&G, (size_t)B * Nc * 2)); CK(hipMalloc(&dq, (size_t)B * d * 4)); CK(hipMalloc(&dc, (size_t)Nc * d * 4));
  float* dscale; CK(hipMalloc(&dscale, 4));  // the upstream gradient, on the device as the benchmark and the autograd operator pass it
  CK(hipMalloc(&y, B * 8)); CK(hipMalloc(&loss, B * 4)); CK(hipMalloc(&lse, B * 4)); CK(hipMalloc(&sum, 4)); CK(hipMalloc(&ws, wsb));
  std::vector<float> h((size_t)Nc * d);
  unsigned s = 12345;
  for (auto& v : h) { s = s * 1664525u + 1013904223u; v = (((s >> 8) & 0xffff) / 65536.0f - 0.5f) * 0.4f; }
  CK(hipMemcpy(q, h.data() + 17, (size_t)B * d * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(c, h.data(), (size_t)Nc * d * 4, hipMemcpyHostToDevice));
  std::vector<int64_t> hy(B); for (int i = 0; i < B; ++i) hy[i] = i * (Nc / B); CK(hipMemcpy(y, hy.data(), B * 8, hipMemcpyHostToDevice));
  const float one = 1.0f; CK(hipMemcpy(dscale, &one, 4, hipMemcpyHostToDevice));
  unsigned long long* dptr; CK(hipGetSymbolAddress((void**)&dptr, HIP_SYMBOL(g_dprhot_tmb)));
  std::vector<unsigned long long> t(4 * 4096 * 8);
  const int NK = 4;
  const bool split = roles == 3;  // kind 0 is the row-store role there
  const char* rname[NK] = {split ? "row-store role" : "step_small_kernel (both products per workgroup)", "dC role", "dQ role", split ? "loss role" : "output role"};
  const int nst[NK] = {split ? 3 : 8, 5, 6, 5};
  const char* pname0[8] = {"", "issue loads", "softmax + G / logits stores (waits for slabs; thread 0)", "", "", "", "", ""};
  const char* pname[NK][8] = {{"", "issue loads", "tiles->LDS (waits for Q, C)", "slab sum (waits for slabs)", "softmax + G", "barrier", "dQ MFMA + slice store + barrier", "dC MFMA + stores + dQ slice sum"},
                             {"", "issue loads", "softmax + G (waits for slabs)", "barrier", "dC MFMA + stores", "", "", ""},
                             {"", "issue loads (waves 0-7)", "softmax + G half (thread 0)", "barrier (C tile of waves 8-15)", "dQ MFMA + slice store + barrier", "slice sum + store", "", ""},
                             {"", "issue loads", "softmax + row stores (waits for slabs)", "barrier", "loss sum + store", "", "", ""}};
  if (split) for (int i = 0; i < 8; ++i) pname[0][i] = pname0[i];
  unsigned long long* dtm; CK(hipGetSymbolAddress((void**)&dtm, HIP_SYMBOL(g_dprhot_tm)));
  unsigned long long tm[64];
  std::vector<double> sim[3];  // sim launch, workgroup (0, 0, 0): stamps 0 -> 1 -> 4 -> 6
  // sim launch, every workgroup: grid (row tiles, column tiles, chunks) as launch_sim_small makes it at small_sim = 1
  unsigned long long* dstm; CK(hipGetSymbolAddress((void**)&dstm, HIP_SYMBOL(g_sim_tm)));
  std::vector<unsigned long long> stm(4096 * 8);
  // (small_sim_copy = 1: behind the gx * gy * gz compute waves, gz or 2 gz layers of copy waves -- sim_small_split_kernel)
  int copyw = 0; dprhot_get_option("small_sim_copy", &copyw);
  const int gx = (B + 15) / 16, gy = (Nc + 15) / 16, gz = d / 256, ncomp = gx * gy * gz;
  const int nsim = std::min(ncomp + (copyw ? (gx + gy + gx * gy - 1) / (gx * gy) * ncomp : 0), 4096);
  // rows of the report: 0 no copy, 1 Cb only, 2 Qb only, 3 both (median over the class's waves; with copy waves: 0 the compute waves,
  // 1 / 2 the copy waves of C / Q tiles), 4 workgroup (0, 0, 0), 5 the last compute wave dispatched, 6 the last wave to end, 7 the
  // last compute wave to end, 8 the last copy wave to end; columns: start, front, middle, tail, end
  std::vector<double> simc[9][5], simspan;
  std::vector<int> simlast;
  // [role][which workgroup: 0 = wg 0, 1 = middle, 2 = last to finish][column: 0 = start, 1.. = phases, nst = end] -> samples
  std::vector<double> samp[NK][3][10], span, spank[NK];
  int nwg[NK] = {0, 0, 0, 0};
  for (int it = 0; it < launches + 3; ++it) {
    CK(hipMemset(dptr, 0, t.size() * 8));
    CK(hipMemset(dtm, 0, sizeof(tm)));
    CK(hipMemset(dstm, 0, stm.size() * 8));
    int rc = dprhot_inbatch_step_f32(q, c, Qb, Cb, B, Nc, d, y, 0, nullptr, 1.f, 1.f / B, 1.f, dscale, nullptr, loss, lse, sum, G, dq, dc, ws, wsb, nullptr);
    if (rc) { printf("rc=%d %s\n", rc, dprhot_last_error()); return 1; }
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(t.data(), dptr, t.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(tm, dtm, sizeof(tm), hipMemcpyDeviceToHost));
    CK(hipMemcpy(stm.data(), dstm, stm.size() * 8, hipMemcpyDeviceToHost));
    if (it < 3) continue;
    if (stm[0] && stm[6]) {
      for (int i = 0; i < 8; ++i) tm[i] = stm[i];
      unsigned long long s0 = ~0ull, s1 = 0; int last = 0, lastk[2] = {0, -1};
      for (int w = 0; w < nsim; ++w) {
        const unsigned long long* r = &stm[(size_t)w * 8];
        if (!r[0] || !r[6]) continue;  // (a copy wave without a tile leaves at once: stamp 0 alone)
        s0 = std::min(s0, r[0]);
        if (r[6] > s1) { s1 = r[6]; last = w; }
        int& lk = lastk[w >= ncomp];
        if (lk < 0 || r[6] > stm[(size_t)lk * 8 + 6]) lk = w;
      }
      simspan.push_back((s1 - s0) * 0.01); simlast.push_back(last);
      std::vector<double> cls[4][5];
      auto cols = [&](int w, double (&o)[5]) {
        const unsigned long long* r = &stm[(size_t)w * 8];
        const unsigned long long r4 = r[4] ? r[4] : r[1];  // (a copy wave has no middle stamp: its tail is waits, conversions and stores)
        o[0] = (r[0] - s0) * 0.01; o[1] = (r[1] - r[0]) * 0.01; o[2] = (r4 - r[1]) * 0.01; o[3] = (r[6] - r4) * 0.01; o[4] = (r[6] - s0) * 0.01;
      };
      for (int w = 0; w < nsim; ++w) {
        if (!stm[(size_t)w * 8] || !stm[(size_t)w * 8 + 6]) continue;
        const int x = w % gx, y = (w / gx) % gy, id = w % (gx * gy) + ((w - ncomp) / (gx * gy) >= gz ? gx * gy : 0);
        const int k = w >= ncomp ? (id < gy ? 1 : 2) : copyw ? 0 : (x == 0 ? 1 : 0) + (y == 0 ? 2 : 0);
        double o[5]; cols(w, o);
        for (int c2 = 0; c2 < 5; ++c2) cls[k][c2].push_back(o[c2]);
      }
      for (int k = 0; k < 4; ++k) for (int c2 = 0; c2 < 5; ++c2) if (!cls[k][c2].empty()) simc[k][c2].push_back(med(cls[k][c2]));
      const int one[5] = {0, ncomp - 1, last, lastk[0], lastk[1]};
      for (int k = 0; k < 5; ++k) {
        if (one[k] < 0) continue; double o[5]; cols(one[k], o); for (int c2 = 0; c2 < 5; ++c2) simc[4 + k][c2].push_back(o[c2]); }
    }
    if (tm[0] && tm[6]) { sim[0].push_back((tm[1] - tm[0]) * 0.01); sim[1].push_back((tm[4] - tm[1]) * 0.01); sim[2].push_back((tm[6] - tm[4]) * 0.01); }
    unsigned long long g0 = ~0ull, g1 = 0;
    for (int k = 0; k < NK; ++k)
      for (int b = 0; b < 4096; ++b) { const unsigned long long* r = &t[((size_t)k * 4096 + b) * 8]; if (r[0]) { g0 = std::min(g0, r[0]); if (r[nst[k] - 1]) g1 = std::max(g1, r[nst[k] - 1]); } }
    if (g1 == 0) { printf("no stamps: did the shape take the small step?\n"); return 1; }
    span.push_back((g1 - g0) * 0.01);
    for (int k = 0; k < NK; ++k) {
      std::vector<int> ids;
      for (int b = 0; b < 4096; ++b) { const unsigned long long* r = &t[((size_t)k * 4096 + b) * 8]; if (r[0] && r[nst[k] - 1]) ids.push_back(b); }
      nwg[k] = (int)ids.size();
      if (ids.empty()) continue;
      int last = ids[0];
      for (int b : ids) if (t[((size_t)k * 4096 + b) * 8 + nst[k] - 1] > t[((size_t)k * 4096 + last) * 8 + nst[k] - 1]) last = b;
      spank[k].push_back((t[((size_t)k * 4096 + last) * 8 + nst[k] - 1] - g0) * 0.01);
      const int pick[3] = {ids[0], ids[ids.size() / 2], last};
      for (int w = 0; w < 3; ++w) {
        const unsigned long long* r = &t[((size_t)k * 4096 + pick[w]) * 8];
        samp[k][w][0].push_back((r[0] - g0) * 0.01);
        for (int i = 1; i < nst[k]; ++i) samp[k][w][i].push_back((r[i] - r[i - 1]) * 0.01);
        samp[k][w][nst[k]].push_back((r[nst[k] - 1] - g0) * 0.01);
      }
    }
  }
  printf("B=%d Nc=%d d=%d small_step_roles=%d, %d launches; us, medians; time zero = first stamp of the launch\n", B, Nc, d, roles, launches);
  printf("launch, first stamp -> last stamp: %.2f\n", med(span));
  const char* wname[3] = {"first workgroup ", "middle workgroup", "last to finish  "};
  for (int k = 0; k < NK; ++k) {
    if (!nwg[k]) continue;
    printf("%s: %d workgroups, its last one ends at %.2f\n", rname[k], nwg[k], med(spank[k]));
    for (int w = 0; w < 3; ++w) {
      printf("  %s start %.2f |", wname[w], med(samp[k][w][0]));
      for (int i = 1; i < nst[k]; ++i) printf(" %s %.2f |", pname[k][i], med(samp[k][w][i]));
      printf(" end %.2f\n", med(samp[k][w][nst[k]]));
    }
  }
  if (!sim[0].empty())
    printf("sim launch (sim_small_kernel, workgroup (0, 0, 0), from its first stamp): address arithmetic + issue loads %.2f | waits, conversions, MFMA chain %.2f | copies + slab stores issued %.2f | in all %.2f\n",
           med(sim[0]), med(sim[1]), med(sim[2]), med(sim[0]) + med(sim[1]) + med(sim[2]));
  if (!simspan.empty()) {
    std::sort(simlast.begin(), simlast.end());
    const int lw = simlast[simlast.size() / 2];
    printf("sim launch, every workgroup (%d x %d x %d single-wave workgroups in dispatch order; a wave's dispatch index w = (chunk * %d + column tile) * %d + row tile):\n", gx, gy, gz, gy, gx);
    printf("  first stamp -> last stamp of the launch: %.2f; the last wave to end is w = %d at the median (row tile %d, column tile %d, chunk %d)\n",
           med(simspan), lw, lw % gx, (lw / gx) % gy, lw / (gx * gy));
    const char* cn[9] = {copyw ? "compute waves (median)         " : "no copy (median of its waves)  ", copyw ? "copy waves of C tiles (median) " : "Cb copy only (median)          ",
                         copyw ? "copy waves of Q tiles (median) " : "Qb copy only (median)          ", "both copies (median)           ",
                         "workgroup (0, 0, 0)            ", "last compute wave dispatched   ", "last wave to end               ", "last compute wave to end       ", "last copy wave to end          "};
    if (copyw) printf("  small_sim_copy = 1: waves w >= %d are copy waves (front + loads issued | - | waits, conversions, stores issued)\n", ncomp);
    for (int k = 0; k < 9; ++k) {
      if (simc[k][0].empty()) continue;
      printf("  %s start %.2f | front + loads issued %.2f | waits, conversions, MFMA chain %.2f | copies + slab stores issued %.2f | end %.2f\n", cn[k], med(simc[k][0]),
             med(simc[k][1]), med(simc[k][2]), med(simc[k][3]), med(simc[k][4]));
    }
  }
  float hs; CK(hipMemcpy(&hs, sum, 4, hipMemcpyDeviceToHost)); printf("loss_sum %.4f\n", hs);
  return 0;
}
