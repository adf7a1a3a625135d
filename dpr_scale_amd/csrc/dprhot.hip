// dprhot.hip -- C ABI (include/dprhot.h) over the gfx950 kernels in gemm_bf16.h / gemm256.h / step_small.h / rowwise.h.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC dprhot.hip -o libdprhot.so
//
// Launch structure of one training step on one rank:
//   dprhot_inbatch_step_f32   2 launches at the BASELINE shapes: sim GEMM (fp32 in, partial-logit slabs) -> one kernel
//                             for softmax-CE, dScores, dQ and dC (step_small.h); elsewhere = the two calls below
//   dprhot_inbatch_fwd(_f32)  2 launches: sim GEMM (+mask, 1/T, softmax statistics or K-split slabs) -> G + loss
//   dprhot_inbatch_bwd        1 launch: dC_part = G^T Q and dQ = G C side by side (+1 when dQ is split over Nc)
//   few rows x many contexts (B <= 128, Nc >= 2048: cfg3 per rank): the four launches of skinny.h (sk_plan)
// Plans (tile, split-K, kernel family) are pure functions of the shape: pick_tile / fwd_plan / dq_plan / big_ok /
// big_bwd_ok / small_step_ok below.
#include "../../include/dprhot.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <dlfcn.h>

#include <type_traits>
#include "gemm_bf16.h"
#include "sim_small.h"
#include "gemm256.h"
#include "gemm8p.h"
#include "gemm8pb.h"
#include "gemm128d.h"
#include "rowwise.h"
#include "step_small.h"
#include "skinny.h"
#include "gradcomm.h"
#include "wide.h"
#include "wideselect.h"
#include "maxsim.h"
#include "ivf.h"
#include "ivf_pack.h"
#include "ivf_pq.h"
#include "router_head.h"
#include "colbert.h"
#include "colbert_cand.h"
#include "colbert_cen.h"
#include "colbert_res.h"
#include "colbert_pq.h"
#include "spar.h"
#include "dense_fp8.h"

using namespace dprhot;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// Multi-rank packed layout (dprhot_inbatch_step_packed_f32): where base is set, the sim epilogues read the column mask from the gathered
// buffer; where stamp_src is set, the dC epilogues stamp the loss numerator (see EpiSim / EpiScaleF32).
struct PackedSpec {
  const uint8_t* base = nullptr;
  int rows_c = 1, n_ctx = 0, row_bytes = 0;
  const float* stamp_src = nullptr;
};
template <class E>
E with_packed_mask(const PackedSpec& pk, E e) {
  if (pk.base != nullptr) {
    e.packed = pk.base;
    e.p_rows_c = pk.rows_c;
    e.p_n_ctx = pk.n_ctx;
    e.p_row_bytes = pk.row_bytes;
  }
  return e;
}
template <class E>
E with_loss_stamp(const PackedSpec& pk, E e) {
  if (pk.stamp_src != nullptr) {
    e.stamp_src = pk.stamp_src;
    e.stamp_period = pk.rows_c;
    e.stamp_row = pk.n_ctx;
  }
  return e;
}

// The one-call training step may carry the sum of the row losses into the launch that combines its dQ slabs (splitk_reduce_loss_kernel): the
// record is a local of inbatch_step_body, `armed` while its forward runs, `pending` from launch_loss_sum's skipped launch until launch_slab_sum
// (or the step's own fall-back) consumes it.
struct LossDefer { bool armed = false, pending = false; const float* src = nullptr; int n = 0; float scale = 1.f; float* out = nullptr; };

// What a call of the training-step family carries besides its public arguments, passed down explicitly; the default value is a plain call.
struct StepCtx {
  PackedSpec packed;
  float loss_scale = 1.0f;   // loss_sum[0] = loss_scale * sum of the row losses (dprhot_train_step_*: the mean of dpr_task.py:212, no division launch)
  bool dc_bf16 = false;      // dC_part as bf16, the reduce-scatter's wire format: only the few-rows step has such an epilogue (step_admit)
  float* dq_part = nullptr;  // the few-rows step leaves its split-K dQ slabs here and skips its reduction launch (dprhot_rescale_grads adds them up)
  LossDefer* defer = nullptr;
};

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return fail(DPRHOT_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// Every kernel launch of this file: raise the dynamic-LDS limit where needed, launch, read the launch's error.
// The state is per kernel: Kern is a template argument, so every instantiation of a __global__ template has its own `raised`.  It holds,
// per device ordinal (one code object per device), the largest dynamic-LDS size raised so far -- a kernel whose LDS grows with the shape
// (step_small.h) raises the limit again when a larger shape follows a smaller one.  Requests up to 48 KiB need no attribute and cost
// no host call besides the launch itself (the eager driver of the batch-32 step is host-paced).
struct LdsRaised {
  size_t dev[64] = {};
  size_t& cur() {
    int d = 0;
    (void)hipGetDevice(&d);
    return dev[d & 63];
  }
};
// a failure names its kernel, "dprhot::sk_bwd_kernel (73984 bytes of dynamic LDS): invalid argument": the name is cut out of launch's own
// __PRETTY_FUNCTION__ ("... [Kern = &dprhot::sk_bwd_kernel, Args = <...>]")
int launch_failed(const char* pretty, size_t lds, hipError_t e) {
  const char* s = strstr(pretty, "Kern = &");
  s = s != nullptr ? s + 8 : pretty;
  const char* end = strstr(s, ", Args");
  return fail(DPRHOT_E_HIP, "%.*s (%zu bytes of dynamic LDS): %s", end != nullptr ? (int)(end - s) : (int)strlen(s), s, lds, hipGetErrorString(e));
}
template <auto Kern, class... Args>
int launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
  if (lds > 48 * 1024) {
    static LdsRaised raised;  // benign race: idempotent
    size_t& r = raised.cur();
    if (r < lds) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return launch_failed(__PRETTY_FUNCTION__, lds, e);
      r = lds;
    }
  }
  hipLaunchKernelGGL(Kern, grid, block, lds, st, args...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return launch_failed(__PRETTY_FUNCTION__, lds, e);
  return DPRHOT_OK;
}

#define REQUIRE(cond, ...) \
  do {                     \
    if (!(cond)) return fail(DPRHOT_E_INVALID, __VA_ARGS__); \
  } while (0)

// ---- explicit process-wide options (dprhot_set_option): test and A/B switches of the plans.  Production never sets one; they replace
// the environment switches the library used to cache on first use (hidden configuration behind an ABI that advertises none).
enum OptId { OPT_TILE, OPT_NO_TR, OPT_BIG_MIN, OPT_NO_SKINNY, OPT_NO_SMALL_STEP, OPT_NO_WIDE, OPT_NO_WIDE_BWD, OPT_SK_FUSED, OPT_SK_W8,
             OPT_SK_PAIR, OPT_SK_TAIL, OPT_SK_DC_REGSCALE, OPT_NL_P16, OPT_SK_DQ_ATOMIC, OPT_NL_MIN, OPT_G128_DMA, OPT_LOSS_WITH_DQ,
             OPT_NL128, OPT_PAIR128, OPT_P16_STAGED, OPT_SMALL_SIM, OPT_SMALL_STEP_ROLES, OPT_SMALL_SIM_COPY, OPT_COUNT };
struct OptDef { OptId id; const char* name; int def; const char* what; };
constexpr OptDef kOptDefs[OPT_COUNT] = {
    {OPT_TILE, "tile", -1, "0..5 pins the tile of the single-GEMM launches (gemm_bf16.h), -1 = plan"},
    {OPT_NO_TR, "no_tr", 0, "1 swaps the LDS transpose read for plain 16-bit gathers (cross-check)"},
    {OPT_BIG_MIN, "big_min", 256, "fewest 256x256 tiles for which the large-shape kernels are chosen (0 = never; tests lower it)"},
    {OPT_NO_SKINNY, "no_skinny", 0, "1 disables the few-rows x many-contexts plan (skinny.h)"},
    {OPT_NO_SMALL_STEP, "no_small_step", 0, "1 disables the fused softmax+backward kernel of the latency-bound shapes (step_small.h)"},
    {OPT_NO_WIDE, "no_wide", 0, "1 keeps vocabulary-wide fp32 operands on the register-staged sim kernel (wide.h off)"},
    {OPT_NO_WIDE_BWD, "no_wide_bwd", 0, "1 keeps the backward of vocabulary-wide vectors on the generic pair kernel (skinny.h units off)"},
    {OPT_SK_FUSED, "sk_fused", 1, "few-rows plan without its dScores launch (G == NULL): 1 = where it measured faster (B x Nc >= 2^19), 2 = wherever the plan exists (tests), 0 = never"},
    {OPT_SK_W8, "sk_w8", 1, "fused few-rows backward with eight waves per workgroup (512 threads, half the output tile per wave: 13.0-13.5 against 13.9-14.4 us at cfg3 per rank); 0 = four"},
    {OPT_SK_PAIR, "sk_pair", 0, "fused few-rows backward with one kind of unit (sk_bwdp_kernel: a P tile is loaded once for both products: measured 21.2 against 13.5 us at cfg3 per rank); 0 = dQ units and dC units (sk_bwdf_kernel)"},
    {OPT_SK_TAIL, "sk_tail", 0, "fused few-rows backward: 1 = the dQ slabs are folded by the last workgroups of the backward launch itself, behind a count of the dQ units (write-through slab stores, sc1 loads; no sk_dq_finish launch), 2 = the same with ordinary stores + one release fence per dQ unit and an acquire fence in the finishing role; 0 = the finishing launch (measured: scratch/negative/README.md, round 5)"},
    {OPT_SK_DC_REGSCALE, "sk_dc_regscale", 0, "fused few-rows backward, dC units: 1 = the Q fragments are scaled by f in registers between the transpose read and the MFMA (no scale pass over the LDS image, one workgroup barrier less; measured: the pass's 0.75 us reappear in the MFMA loop, step 25.7-25.8 against 25.3-25.6 us), 0 = the scale pass of round 4"},
    {OPT_NL_P16, "nl_p16", 1, "no-logits forward with the dScores wanted: 1 = ONE pass of the GEMM (strip statistics + the tile's fp16 softmax numerators, Epi8StatsP, two-phase schedule) and a row kernel that rescales them into G in place; 0 = two GEMM passes (statistics, then the logits recomputed into G: Epi8G)"},
    {OPT_SK_DQ_ATOMIC, "sk_dq_atomic", 0, "fused few-rows backward: 1 = the dQ units scale their tiles to the row softmax themselves and ADD them into dQ (global_atomic_add_f32; dQ zero-filled by the sim launch): no slabs, no finishing launch -- dQ reproducible to rounding, not to the bit; 0 = slice-normalised slabs + sk_dq_finish_kernel (bit-reproducible)"},
    {OPT_NL_MIN, "nl_min", 128, "fewest 256x256 tiles from which the forward never stores the logits (round 6: 128 -- with the one-pass forward 1024 x 8192 x 768 steps in 81 instead of 92 us, 512 x 16384 in 116 instead of 126; at 64 tiles it is a wash, at 32 it loses); the smaller of this and big_min counts"},
    {OPT_G128_DMA, "g128_dma", 1, "128 x 128 x 64 tile of the GEMM engine with its operands staged by LDS-DMA (gemm128d.h) instead of global -> VGPR -> ds_write (gemm_bf16.h): 1 = wherever the launch qualifies (bf16 operands, whole 64-deep K steps, 32-bit offsets); 0 = never"},
    {OPT_LOSS_WITH_DQ, "loss_with_dq", 1, "one-call training step on the no-logits forward, single rank: 1 = the sum of the row losses is formed by one more workgroup of the launch that combines the dQ slabs (same arithmetic as reduce_sum_kernel) instead of a launch of its own between forward and backward; 0 = its own launch"},
    {OPT_NL128, "nl128", 1, "training forward (dScores wanted, logits not) in ONE pass on the 128 x 128 LDS-DMA tile (EpiSimP: strip statistics + fp16 softmax numerators, then the row kernel of the 256 x 256 family) where the 256-wide tiles would leave most of the chip idle: 1 = on, 0 = the logits-storing forward (sim GEMM with fp32 S, streaming softmax) there"},
    {OPT_PAIR128, "pair128", 1, "backward pair (dC tiles next to split-K dQ tiles in one launch) on the 128 x 128 LDS-DMA tile (gemm128d_pair_kernel): 1 = where the rule pair128_use picks it, 2 = wherever the launch qualifies (A/B), 0 = never (the register-staged pair / the 256 x 256 pair)"},
    {OPT_P16_STAGED, "p16_staged", 1, "one-pass forward on the 256 x 256 kernel: the fp16 numerators leave through the per-wave LDS patch (64-byte pieces of 16 rows per store instruction instead of 32-byte pieces of 32 rows; bit-identical): 1 = except where the row pitch of G is a multiple of 128 KiB (forward us, arms alternating, profiles/r06_p16_staged_ab.txt: 8192^2 155.4 -> 147.8, 4096 x 8192 83.2 -> 79.3, 4096 x 16384 153 -> 146 and its step 390 -> 372; at 65536 columns the forward gains nothing and the step of 8192 x 65536 LOSES 100 us of 2880), 2 = always, 0 = never"},
    {OPT_SMALL_SIM, "small_sim", 1, "sim launch of the batch-32 step (B <= 32, fp32 q, 256-deep K chunks: sim_small.h): 1 = one wave per 16 x 16 tile and K chunk on an exact 3-D grid (row tile, column tile, chunk: no division and one wait on the arguments in front of the first operand load, the mask byte loaded last), whole-line loads rounded into a wave-private LDS patch, no barrier (bit-identical to the engine; 32 x 256 x 768 step 9.19 -> 8.29 us, with the 3-D grid 7.21 -> 7.05); 0 = the GEMM engine (tile 5); A/B only: 2 = fp32 straight into fragment registers, no LDS (8.52 us), 3 / 4 = forms 1 / 2 with two waves per workgroup (8.70 / 9.41 us)"},
    {OPT_SMALL_STEP_ROLES, "small_step_roles", 3, "softmax + backward launch of the batch-32 step (B <= 32, at most 768 columns: step_small_kernel_roles / step_small_kernel_out in step_small.h): one launch split by role -- d / 16 dC workgroups (slabs + Q tile, full softmax, one barrier, dC product and stores) next to one dQ workgroup per 16-row half and column tile (half the slabs + C tile, 8 K slices); 3 = form 2 with the outputs written by workgroups of their own that have no product to do, in front of the grid, instead of by the dC workgroup of tile 0: a loss block (softmax up to the row loss, logsumexp / row loss, one barrier, the loss sum) and two row-store blocks (one 16-row half each: dScores / logits, no barrier); the device-side scale is the last load of a role, not a wait in front of it (a stamping launch of the packed step keeps form 2), 2 = 32-column dQ tiles (d % 32 == 0, else form 1; 32 x 256 x 768 step 8.29 -> 7.74 us), 1 = 16-column dQ tiles (7.84 us), 0 = every workgroup does both products (step_small_kernel); all forms bit-identical (tests/test_small_step_roles.py, tests/test_small_step_out.py, tests/test_small_step_split_gpu.py)"},
    {OPT_SMALL_SIM_COPY, "small_sim_copy", 1, "sim launch of the batch-32 step where small_sim selects form 1: 1 = the bf16 copies Qb / Cb are written by waves of their own behind the compute waves in dispatch order (sim_small_split_kernel: 16 rows x one 256-deep chunk of one operand per wave, whole-line loads, the same v_cvt_pk_bf16_f32 pairing; the compute waves go from their MFMA chain straight to their slab stores; bit-identical), and the copy waves store 16-byte WRITE-THROUGH (sc1) pieces -- lanes 2m / 2m + 1 exchange one 8-byte piece by DPP quad_perm [1, 0, 3, 2], eight buffer stores per lane, nothing waits for them -- so the copies' 442 KB are not dirty lines of the XCD L2s that the kernel boundary writes back behind the last wave (profiles/dirty_boundary_probe.txt: 0.2 us per boundary; 32 x 256 x 768 step 6.62 -> 6.42 us, profiles/small_wt_ab.txt; tests/test_small_wt_gpu.py); 2 = the copy waves with the 8-byte plain stores they had before (A/B); 0 = every compute wave of row tile 0 / column tile 0 stores the copies itself, in front of its slab stores (sim_small_kernel).  The same write-through form for the dC tiles of the second launch LOST (scratch/negative/README.md)"},
};
constexpr bool opt_table_in_enum_order() {  // (round 6: a row added in the wrong place made two options answer to each other's names)
  for (int i = 0; i < OPT_COUNT; ++i)
    if (kOptDefs[i].id != (OptId)i) return false;
  return true;
}
static_assert(opt_table_in_enum_order(), "kOptDefs must list the options in the order of enum OptId");
long long g_opt_epoch = 0;  // bumped by every dprhot_set_option: host-side caches of plan facts key on it (dprhot_options_epoch)
int g_opt[OPT_COUNT];  // the defaults of the table above (one place: a default typed twice was typed wrong once)
const bool g_opt_defaults = [] {
  for (int i = 0; i < OPT_COUNT; ++i) g_opt[i] = kOptDefs[i].def;
  return true;
}();
inline int opt(OptId i) { return __atomic_load_n(&g_opt[i], __ATOMIC_RELAXED); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Scratch that a call needs zeroed is zeroed by a KERNEL of the caller's stream, never by hipMemsetAsync: the candidate counters of the
// filtered searches (dprhot_search, dprhot_spar_search, dprhot_dense_fp8_search), the rank counters of dprhot_sim_rank / _rank_loss and
// the score buffer of an IVF search without CLS vectors.  Eagerly the memsets did their work.  OBSERVED: with the memset captured as
// the FIRST node of a graph and the graph replayed right behind a caller's fill of the workspace on the same stream, the zeroes were
// absent when the next kernel node ran -- the IVF scores came out on top of the fill pattern in one run of two, and dprhot_search,
// whose filter epilogues then indexed their candidate lists by atomicAdd(&cnt[row], 1) without a bound, stored far outside the
// workspace and faulted (tests/test_stream_capture_gpu.py, rows `ivf-no-cls` and `search`).  SUPPOSED, not established: that the
// runtime does not order such a memset node behind work already queued on the launching stream.  Either way a kernel node is ordered
// like every other launch of the call, and the epilogues now check the position against the list's length (gemm_bf16.h, gemm8p.h,
// spar.h, dense_fp8.h; the merge clamps the count it reads): a stale counter can lose candidates, it cannot store or read outside.
__global__ void zero_words_kernel(unsigned* p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0u;
}
int zero_words(void* p, size_t n_words, hipStream_t st) {
  const size_t blocks = (n_words + 255) / 256;
  return launch<zero_words_kernel>(dim3((unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks))), dim3(256), 0, st, static_cast<unsigned*>(p), n_words);
}

bool use_tr() { return opt(OPT_NO_TR) == 0; }

int force_tile() { return opt(OPT_TILE); }

constexpr int kNumCU = 256;

// tile configurations {BM, BN, BK}
struct TileSpec { int bm, bn, bk; };
constexpr int kNumTiles = 7;  // 0-5: gemm_bf16.h (register staging); 6: gemm256.h (k-major x k-major, K % 64 == 0 only)
constexpr int kBigTile = 6;
constexpr TileSpec kTiles[kNumTiles] = {{128, 128, 64}, {64, 128, 64}, {64, 64, 64}, {32, 64, 64}, {32, 64, 256}, {32, 32, 256},
                                        {256, 256, 64}};

int big_min_wgs() { return opt(OPT_BIG_MIN); }
bool big_ok(int M, int N, int K) {
  const long wgs = (long)((M + 255) / 256) * ((N + 255) / 256);
  return M > 128 && K % 64 == 0 && K >= 128 && big_min_wgs() > 0 && wgs >= big_min_wgs();
}

// The phase-interleaved persistent 256x256 kernel (gemm8p.h) and the forward built on it that never stores the logits: same gate
// as the 256x256 tile, plus an even number of K steps and operands addressable with 32-bit byte offsets.
// (the storing / filtering uses of the same kernel -- dprhot_sim_fwd, dprhot_search -- keep the 256-tile gate they were measured at)
bool g8_ok(int M, int N, int K) {
  return force_tile() < 0 && big_ok(M, N, K) && K % 128 == 0 && (double)M * K * 2 < 4.0e9 && (double)N * K * 2 < 4.0e9;
}
bool nl_ok(int M, int N, int K) {
  const long wgs = (long)((M + 255) / 256) * ((N + 255) / 256);
  const int need = big_min_wgs() < opt(OPT_NL_MIN) ? big_min_wgs() : opt(OPT_NL_MIN);
  const bool big = M > 128 && K % 64 == 0 && K >= 128 && big_min_wgs() > 0 && wgs >= need;  // (big_ok with this plan's own tile count)
  return force_tile() < 0 && big && K % 128 == 0 && (double)M * K * 2 < 4.0e9 && (double)N * K * 2 < 4.0e9;
}

// One-pass training forward on the 128 x 128 LDS-DMA tile (EpiSimP + g8_lse_p2g_kernel): more than 128 rows, whole 64-deep K steps,
// at least kNl128MinTiles 128-wide tiles; where the 256 x 256 forward qualifies too, at most one round of them (kNl128MaxTiles) and
// fewer than 256 tiles of 256 x 256 -- where it does not (K a multiple of 64 but not of 128), every size; 32-bit element offsets.
// kNl128MinTiles: 32 against 128, step us: 512 x 2048 44.1 -> 40.7, 768 x 2048 49.7 -> 42.5, 1024 x 1024 47.3 -> 43.5, 256 x 4096 /
// 192 x 4096 / 256 x 2048 level.  kNl128MaxTiles: 512 = one round of two workgroups per CU; beyond, where the 256 x 256 no-logits forward
// qualifies, that one runs: 1536 x 8192 x 768, 768 tiles, 48.6 us against ~37.
constexpr int kNl128MinTiles = 32, kNl128MaxTiles = 512;
bool nl128_ok(int M, int N, int K) {
  if (!opt(OPT_NL128) || !opt(OPT_G128_DMA) || !opt(OPT_NL_P16) || force_tile() >= 0) return false;
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128), t256 = (long)((M + 255) / 256) * ((N + 255) / 256);
  return M > 128 && K % 64 == 0 && K >= 64 && N % 8 == 0 && N >= 1024 && t128 >= kNl128MinTiles && (!nl_ok(M, N, K) || (t128 <= kNl128MaxTiles && t256 < 256)) &&
         (double)M * K < 4.0e9 && (double)N * K < 4.0e9 && (N + 63) / 64 <= 1024 * 64;
}

// Tile for D[M,N] with contraction length K: the largest tile (BM capped by M) that still yields `want`
// workgroups, else the smallest; small-M problems with a long K use the BK=256 variants (latency-bound:
// fewer, fatter K steps keep a whole K range in flight).
int pick_tile(int M, int N, int K, int splits_hint, int want) {
  if (force_tile() >= 0 && force_tile() < kBigTile) return force_tile();
  if (M <= 32) {
    if (K < 256) return 3;
    const long wg64 = (long)cdiv(N, 64) * splits_hint;
    return wg64 >= want / 2 ? 4 : 5;
  }
  const int first = M <= 64 ? 1 : 0;
  // (round 6: the 128 x 128 tile is the LDS-DMA kernel now and wins earlier -- 768 x 8192 x 768 stored-logits GEMM 30.0 -> 22.6 us with 384
  //  workgroups where the plan wanted 512 and took 64 x 128 tiles; a tie at 256 workgroups, a loss below: scratch/sim_tile_ab.py)
  if (first == 0 && opt(OPT_G128_DMA) != 0 && K % 64 == 0 &&
      (long)cdiv(M, kTiles[0].bm) * cdiv(N, kTiles[0].bn) * splits_hint * 8 >= (long)want * 5)
    return 0;
  for (int t = first; t <= 2; ++t) {
    const long wgs = (long)cdiv(M, kTiles[t].bm) * cdiv(N, kTiles[t].bn) * splits_hint;
    if (wgs >= want) return t;
  }
  return 2;
}

// The kernel of a bf16 score GEMM S[M,N] = Q x C^T (both operands k-major, no split-K) that stores or filters its tile: the storing
// forward (sim_fwd_body) and the filtered chunks of dprhot_search make this one choice.
struct SimGemm { bool g8; int tile, kchunk; };  // g8: the phase-interleaved kernel (gemm8p.h); else the tile id of launch_gemm and its K range
SimGemm sim_gemm(int M, int N, int K) {
  if (g8_ok(M, N, K)) return SimGemm{true, kBigTile, K};
  const int tile = (force_tile() < 0 && big_ok(M, N, K)) ? kBigTile : pick_tile(M, N, K, 1, 2 * kNumCU);
  return SimGemm{false, tile, cdiv(K, kTiles[tile].bk) * kTiles[tile].bk};
}

template <int BM, int BN, int BK, bool AK, bool BKM, bool TR, class Epi, bool AF = false, bool BF = false>
int launch_one(const GemmArgs& a, const Epi& epi, int splits, hipStream_t st) {
  dim3 grid(cdiv(a.N, BN), cdiv(a.M, BM), splits);
  return launch<gemm_bf16_kernel<BM, BN, BK, 2, 2, AK, BKM, TR, Epi, AF, BF>>(grid, dim3(256), gemm_lds_bytes<BM, BN, BK, AK, BKM>(), st, a, epi);
}

// persistent (one workgroup per CU walking its tiles with the K pipeline running across tile boundaries) when the
// epilogue stores next to nothing; one workgroup per tile when it stores the whole tile: a finished workgroup's stores
// drain while its successor on the CU is already loading, a persistent one would have to wait for them
template <class Epi, bool PERSIST>
int launch_big(const GemmArgs& a, const Epi& epi, hipStream_t st) {
  const int nbx = cdiv(a.N, G2_B), nby = cdiv(a.M, G2_B);
  const int grid = (!PERSIST || nbx * nby < kNumCU) ? nbx * nby : kNumCU;
  return launch<gemm256_kernel<Epi, PERSIST>>(dim3((unsigned)grid), dim3(G2_THREADS), g2_lds_total, st, a, epi, nbx, nby);
}

// SCHED: 4 = four phases of 8 MFMAs per K step, 2 = two phases of 16 (bit-identical; the dScores pass, whose store epilogue delays
// the first DMA waits of the next tile, is consistently ~4 % faster on the two-phase schedule: 111-114 vs 116-121 us at 8192^2 x 768)
template <class Epi, int SCHED = 4>
int launch_g8(const GemmArgs& a, const Epi& epi, hipStream_t st) {
  const int nbx = cdiv(a.N, G2_B), nby = cdiv(a.M, G2_B);
  const int grid = nbx * nby < kNumCU ? nbx * nby : kNumCU;
  return launch<gemm8p_kernel<Epi, 0, SCHED>>(dim3((unsigned)grid), dim3(G2_THREADS), g8_lds_total, st, a, epi, nbx, nby);
}
// the inputs every gemm8p.h sim epilogue shares
Epi8Base g8_base(const PackedSpec& pk, const dprhot_bf16* Q, int B, int Nc, const int64_t* y, int64_t y_offset, const uint8_t* colmask, float inv_T,
                 float* gold) {
  EpiSim e{nullptr, colmask, B, Nc, inv_T, nullptr, nullptr, y, y_offset, gold, nullptr, 0};
  Epi8Base b;
  b.sim = with_packed_mask(pk, e);
  b.dummy = Q;
  return b;
}

// whether a launch on tile 0 runs with LDS-DMA staging (gemm128d.h) instead of register staging: launch_gemm's rule, also read by the
// plan query of the search (gemm_form)
template <bool AK, bool BKM>
bool g128d_takes(const GemmArgs& a) {
  constexpr bool needs_tr = !(AK && BKM);
  const bool tr = needs_tr ? use_tr() : false;
  // (K: whole 64-deep steps -- or, with B mn-major, any K from 64 on (a multiple of 8 when A is k-major): the partial last step is read against zeros, g1_tile)
  return opt(OPT_G128_DMA) != 0 && (tr || !needs_tr) && (a.K % 64 == 0 || (!BKM && a.K >= 64 && (!AK || a.K % 8 == 0))) && a.kchunk % 64 == 0 && a.M >= 8 && a.N >= 8 &&
         (double)(AK ? a.M : a.K) * a.lda < 4.0e9 && (double)(BKM ? a.N : a.K) * a.ldb < 4.0e9;  // (32-bit element offsets inside one K range)
}

template <bool AK, bool BKM, class Epi>
int launch_gemm(int tile, const GemmArgs& a, const Epi& epi, int splits, hipStream_t st) {
  if constexpr (AK && BKM) {
    if (tile == kBigTile) {
      if (splits != 1 || a.K % 64 != 0) return fail(DPRHOT_E_UNSUPPORTED, "256x256 tile: no split-K, K %% 64 == 0");
      return launch_big<Epi, std::is_same<Epi, EpiFilter>::value>(a, epi, st);
    }
  }
  constexpr bool needs_tr = !(AK && BKM);
  const bool tr = needs_tr ? use_tr() : false;
  if (tile == 0 && g128d_takes<AK, BKM>(a)) {
    // the same tile with LDS-DMA staging (gemm128d.h): same images, same fragments, same epilogues
    return launch<gemm128d_kernel<AK, BKM, Epi>>(dim3(cdiv(a.N, 128), cdiv(a.M, 128), splits), dim3(256), g1_lds_bytes, st, a, epi);
  }
#define DPRHOT_TILE_CASE(T, BM, BN, BK_)                                                       \
  case T:                                                                                      \
    if constexpr (needs_tr) {                                                                  \
      return tr ? launch_one<BM, BN, BK_, AK, BKM, true, Epi>(a, epi, splits, st)              \
                : launch_one<BM, BN, BK_, AK, BKM, false, Epi>(a, epi, splits, st);            \
    } else {                                                                                   \
      return launch_one<BM, BN, BK_, AK, BKM, false, Epi>(a, epi, splits, st);                 \
    }
  switch (tile) {
    DPRHOT_TILE_CASE(0, 128, 128, 64)
    DPRHOT_TILE_CASE(1, 64, 128, 64)
    DPRHOT_TILE_CASE(2, 64, 64, 64)
    DPRHOT_TILE_CASE(3, 32, 64, 64)
    DPRHOT_TILE_CASE(4, 32, 64, 256)
    DPRHOT_TILE_CASE(5, 32, 32, 256)
  }
#undef DPRHOT_TILE_CASE
  return fail(DPRHOT_E_UNSUPPORTED, "bad tile id %d", tile);
}

// sim GEMM reading fp32 operands directly (AF: q is fp32, BF: c is fp32); bf16 copies go to a.Acopy / a.Bcopy
template <bool AF, bool BF>
int launch_sim_f32(int tile, const GemmArgs& a, const EpiSim& epi, int splits, hipStream_t st) {
  switch (tile) {
    case 0: return launch_one<128, 128, 64, true, true, false, EpiSim, AF, BF>(a, epi, splits, st);
    case 1: return launch_one<64, 128, 64, true, true, false, EpiSim, AF, BF>(a, epi, splits, st);
    case 2: return launch_one<64, 64, 64, true, true, false, EpiSim, AF, BF>(a, epi, splits, st);
    case 3: return launch_one<32, 64, 64, true, true, false, EpiSim, AF, BF>(a, epi, splits, st);
    case 4: return launch_one<32, 64, 256, true, true, false, EpiSim, AF, BF>(a, epi, splits, st);
    case 5: return launch_one<32, 32, 256, true, true, false, EpiSim, AF, BF>(a, epi, splits, st);
  }
  return fail(DPRHOT_E_UNSUPPORTED, "bad tile id %d", tile);
}

// ---- backward pair: dC (tile 0 or 2) next to dQ (tile 0, 2 or 4) in one launch --------------------------
template <class C1, class C2>
int launch_pair_one(const GemmArgs& a1, const EpiScaleF32& e1, const GemmArgs& a2, const EpiScaleF32& e2, int splits2,
                    hipStream_t st) {
  constexpr size_t lds = C1::lds > C2::lds ? C1::lds : C2::lds;
  const int nbx1 = cdiv(a1.N, C1::BN), nby1 = cdiv(a1.M, C1::BM);
  const int nbx2 = cdiv(a2.N, C2::BN), nby2 = cdiv(a2.M, C2::BM);
  const long blocks = (long)nbx1 * nby1 + (long)nbx2 * nby2 * splits2;
  if (blocks > 0x7fffffffL) return fail(DPRHOT_E_UNSUPPORTED, "grid too large");
  return launch<gemm_pair_kernel<C1, C2, EpiScaleF32, EpiScaleF32>>(dim3((unsigned)blocks), dim3(256), lds, st, a1, e1, nbx1, nby1, a2, e2, nbx2, nby2);
}

template <bool TR>
int launch_pair_tr(int t1, int t2, const GemmArgs& a1, const EpiScaleF32& e1, const GemmArgs& a2, const EpiScaleF32& e2,
                   int splits2, hipStream_t st) {
  using DC0 = GemmCfg<128, 128, 64, false, false, TR>;
  using DC2 = GemmCfg<64, 64, 64, false, false, TR>;
  using DQ0 = GemmCfg<128, 128, 64, true, false, TR>;
  using DQ2 = GemmCfg<64, 64, 64, true, false, TR>;
  using DQ4 = GemmCfg<32, 64, 256, true, false, TR>;
  if (t1 == 0 && t2 == 0) return launch_pair_one<DC0, DQ0>(a1, e1, a2, e2, splits2, st);
  if (t1 == 0 && t2 == 2) return launch_pair_one<DC0, DQ2>(a1, e1, a2, e2, splits2, st);
  if (t1 == 0 && t2 == 4) return launch_pair_one<DC0, DQ4>(a1, e1, a2, e2, splits2, st);
  if (t1 == 2 && t2 == 0) return launch_pair_one<DC2, DQ0>(a1, e1, a2, e2, splits2, st);
  if (t1 == 2 && t2 == 2) return launch_pair_one<DC2, DQ2>(a1, e1, a2, e2, splits2, st);
  if (t1 == 2 && t2 == 4) return launch_pair_one<DC2, DQ4>(a1, e1, a2, e2, splits2, st);
  return fail(DPRHOT_E_UNSUPPORTED, "no fused backward for tiles (%d,%d)", t1, t2);
}

int check_shape(int B, int Nc, int d) {
  REQUIRE(B > 0 && Nc > 0 && d > 0, "non-positive shape B=%d Nc=%d d=%d", B, Nc, d);
  REQUIRE(d % 8 == 0, "d=%d must be a multiple of 8 (16-byte rows)", d);
  REQUIRE(Nc % 8 == 0, "Nc=%d must be a multiple of 8 (16-byte rows; pad with masked columns)", Nc);
  return DPRHOT_OK;
}

// split-K plan of dQ = G x C  (M = B, N = d, K = Nc); tile restricted to what the fused pair kernel has
struct DqPlan { int tile, splits, kchunk; bool big; };
// the 256x256 LDS-DMA backward pair (gemm256.h): both contraction lengths multiples of 64, enough 256-row blocks to
// matter, operands addressable with 32-bit element offsets
bool big_bwd_ok(int B, int Nc, int d) {
  if (force_tile() >= 0 || big_min_wgs() <= 0) return false;
  if (B % 64 != 0 || Nc % 64 != 0) return false;
  if ((double)B * Nc >= 4.0e9 || (double)Nc * d >= 4.0e9) return false;
  const long units = (long)((Nc + 255) / 256 + (B + 255) / 256) * ((d + 255) / 256);
  if (big_min_wgs() < 96) return units >= big_min_wgs();  // DPRHOT_BIG_MIN lowered: tests push small shapes through
  return B >= 256 && Nc >= 1024 && d >= 256 && units >= 96;
}
DqPlan dq_plan(int B, int Nc, int d) {
  DqPlan p;
  p.big = big_bwd_ok(B, Nc, d);
  if (p.big) {
    // dQ units as long as dC units (K = B each): split Nc into ~Nc/B slices, at most 16
    int splits = (Nc + B - 1) / B;
    // at most 16 slices (bounds the fp32 slab traffic) -- 32 under 512 rows when the launch takes more than one round of the chip anyway:
    // the dQ units are then as short as the dC units (K = B) instead of the long pole at the end of the grid.  Measured, step us
    // (profiles/r06_dq_cap_ab.txt): 256 x 32768 172.6 -> 146.6, 384 x 16384 116.5 -> 107.4, 448 x 16384 124.1 -> 113.5; where 16 slices
    // fit one round, 32 lose or change nothing (256 x 16384 86.0 -> 100.3, 256 x 8192 60.2 -> 60.9).
    int cap = 16;
    if (B < 512) {
      const long at16 = (long)cdiv(Nc, 256) * cdiv(d, 256) + (long)cdiv(B, 256) * cdiv(d, 256) * 16;
      cap = at16 > kNumCU ? 32 : 16;
    }
    if (splits > cap) splits = cap;
    // Long context axis (the dQ units run in a launch of their own: dprhot_inbatch_bwd's long_axis rule): ONE round of units on the
    // 256 CUs instead -- 1024 x 65536 x 768: 12 tiles x 21 slices = 252 units where 16 slices left a quarter of the chip idle;
    // 2048 x 65536: 24 x 10 = 240 units in one round where 24 x 16 = 384 took two (round 6; backward us against at most 16 slices:
    // 1536 x 65536 x 768 419 -> 351, 2048 x 65536 497 -> 459, 1024 x 65536 294 -> 282: profiles/r06_dq_round_ab.txt)
    if (B >= 1024 && B <= 2048 && (long)Nc >= 32L * B) {
      const int tiles = cdiv(B, 256) * cdiv(d, 256);
      int one = kNumCU / tiles;
      if (one > 32) one = 32;
      if (one >= 1 && one < (Nc + B - 1) / B) splits = one;
    }
    if (splits < 1) splits = 1;
    p.tile = kBigTile;
    p.kchunk = cdiv(cdiv(Nc, 128), splits) * 128;  // an even number of 64-deep K steps per slice (gemm8pb.h)
    p.splits = cdiv(Nc, p.kchunk);
    return p;
  }
  if (B <= 32 && Nc >= 256) p.tile = 4;
  else if (B <= 256) p.tile = 2;
  else p.tile = 0;
  const TileSpec ts = kTiles[p.tile];
  const int tiles = cdiv(B, ts.bm) * cdiv(d, ts.bn);
  const int ksteps = cdiv(Nc, ts.bk);
  int splits = cdiv(kNumCU, tiles);
  const int min_steps = ts.bk >= 256 ? 1 : 2;
  if (splits > ksteps / min_steps) splits = ksteps / min_steps;
  if (splits > 16) splits = 16;  // bounds the fp32 slab traffic (splits * B * d * 4 bytes each way)
  if (splits < 1) splits = 1;
  p.kchunk = cdiv(ksteps, splits) * ts.bk;
  p.splits = cdiv(Nc, p.kchunk);
  return p;
}

// The backward pair on the 128 x 128 LDS-DMA tile (gemm128d_pair_kernel): dC over K = B (any count above 64: the last step may be partial,
// g1_tile), dQ over K = Nc in slices of whole steps (any multiple of 8 -- the packed layout of 2 or 4 ranks is rarely a multiple of 64),
// 32-bit element offsets, the LDS transpose read for the mn-major operands.
struct Pair128Plan { bool ok; int splits, kchunk; };
Pair128Plan pair128_plan(int B, int Nc, int d) {
  Pair128Plan p{};
  p.ok = opt(OPT_PAIR128) != 0 && opt(OPT_G128_DMA) != 0 && use_tr() && force_tile() < 0 && Nc % 8 == 0 &&
         d % 8 == 0 && B >= 64 && d >= 8 && (double)B * Nc < 4.0e9 && (double)Nc * d < 4.0e9;
  // K slices of a dQ tile.  The dQ units lead the grid and the (shorter) dC tiles fill in behind them, so the launch is as long as the
  // larger of one dQ unit and the chip's share of all K steps; every slice costs a slab of B x d fp32 written and read again.  Two
  // lower bounds, the larger wins, at most 16: (balance) a dQ unit no longer than twice the per-slot average of the launch's K steps
  // (512 slots: two workgroups per CU); (traffic is cheap) slabs up to a quarter of the dC bytes: Nc / (4 B).  Measured against 8 / 16 /
  // 32 slices (profiles/r06_pair128_ab.txt): 256 x 8192 22.2 / 22.7 / 26.9 us, 384 x 8192 24.6 / 28.9 / 29.4, 512 x 8192 28.5 / 33.1 /
  // 33.2, 448 x 16384 42.8 / 45.3 / 53.0, 256 x 32768 55.8 / 50.2 / 54.6.
  const double avg = (double)B * Nc * ((d + 127) / 128 * 128) / 268435456.0;  // K steps per slot: 2 B Nc d / (128 * 128 * 64) / 512
  int s = (int)((double)Nc / (128.0 * (avg < 1.0 ? 1.0 : avg)) + 0.999);
  if (s < Nc / (4 * B)) s = Nc / (4 * B);
  if (s > 16) s = 16;
  if (s > Nc / 256) s = Nc / 256;
  if (s < 1) s = 1;
  p.kchunk = cdiv(cdiv(Nc, 64), s) * 64;
  p.splits = cdiv(Nc, p.kchunk);
  return p;
}
// Where it runs (measured against the plan it replaces at 60 shapes, profiles/r06_pair128_ab.txt): under 1024 query rows everywhere, and up
// to B x Nc = 2^25 scores above that.  Beyond, the 256 x 256 kernels keep the backward: their tiles need half the operand bytes per flop,
// and at that size they fill the chip (8192^2: 191 against 200 us; 1024 x 65536: 258 / 295, the 128-wide tiles' pieces alias at a 128 KiB
// row pitch; 4096 x 32768: 410 / 458) -- although 4096 x 16384 (216 / 201) and 2048 x 49152 (393 / 359) would still gain.
// What it replaced: the register-staged pair under the 256 x 256 gate (2048 x 4096 x 768: 70 -> 39 us, 1024 x 4096 44 -> 27, 4096 x 4096
// 86 -> 62), the 256 x 256 pair of the few-rows shapes (256 x 8192 29.7 -> 21.0, 768 x 16384 76.8 -> 57.0, 256 x 32768 76.9 -> 52.5,
// 1024 x 16384 79.5 -> 70.3) and the two separate launches of the long axis under 512 rows (512 x 65536 184 -> 164, 128 x 32768 63 -> 37).
bool pair128_use(int B, int Nc, int d) {
  if (!pair128_plan(B, Nc, d).ok) return false;
  if (opt(OPT_PAIR128) == 2) return true;
  // (not under 2048 contexts -- 1024 with at most 512 rows: a dozen 128-wide tiles lose to the smaller register-staged ones there,
  //  128 x 128 5.8 against 3.8 us, 512 x 512 12.6 / 11.6, 1024 x 1024 19.8 / 18.9; 512 x 1024 14.7 / 17.2 and 512 x 2048 15.8 / 21.1 win)
  if (Nc < 1024 || (Nc < 2048 && B > 512)) return false;
  // (above the bound only the shapes the 256 x 256 pair does not take -- row or column counts that are no multiples of 64: they would run
  //  on the register-staged pair, 2000 x 32000 x 768: 448 against 262 us)
  if (B < 1024 || !big_bwd_ok(B, Nc, d)) return true;
  if ((double)B * Nc > 33554432.0) return false;
  // From 1024 rows on the 256 x 256 pair keeps the shapes whose units fill whole rounds of the 256 CUs: with d = 1024 (four column tiles)
  // 1024 x 8192, 2048 x 8192 and 4096 x 8192 are exactly 256 units and 2048 x 16384 is 512 -- 48.9 / 73.2 / 124.9 / 141.2 us against 55.7 /
  // 91.8 / 132.4 / 148.5 on the 128-wide pair -- where d = 768 leaves them at 192 / 384 units, three quarters of a round (tie, tie, tie,
  // 124 -> 111 for the 128-wide pair): profiles/r06_pair128_dim_ab.txt.
  const DqPlan p8 = dq_plan(B, Nc, d);
  const long u8 = ((long)cdiv(Nc, 256) + (long)cdiv(B, 256) * p8.splits) * cdiv(d, 256);
  const long rounds = (u8 + kNumCU - 1) / kNumCU;
  return u8 * 10 < rounds * kNumCU * 9;  // (fill below 0.9)
}

int dc_tile(int B, int Nc, int d) { return ((long)cdiv(Nc, 128) * cdiv(d, 128) >= kNumCU) ? 0 : 2; }

// Few query rows against many contexts (skinny.h): B <= 128 (a multiple of 32), d a multiple of 128 up to 1024, 512 (256 above 64 rows) <= Nc <= 16384
// (beyond that the per-unit recomputation of the row logsumexp from Nc / 128 tile values stops being cheap).  Lower bound, measured
// against the three-launch plan and the fused small step (scripts/bench_rankstep.py, round 3): 128 x 520 18.2 vs 22.0 us, 128 x 1032
// 18.5 vs 26.2, 96 x 776 17.8 vs 22.8, 64 x 776 17.1 vs 18.0, 64 x 1088 18.2 vs 20.1 (64 x 520: 17.0 both); with B = 32 the fused
// small step wins up to ~1000 columns (776: 16.2 vs 16.4; 904: 16.4 vs 16.5) and loses above (1056: 17.4 vs 16.6).
struct SkPlan { bool ok; int nt, nts, scols, nrb, ksteps, nslices; };
SkPlan sk_plan(int B, int Nc, int d) {
  const bool off = opt(OPT_NO_SKINNY) != 0, no_small = opt(OPT_NO_SMALL_STEP) != 0;  // (no_small lets this plan take the small-step shapes)
  const int min_nc = B > 64 ? 256 : 512;  // (128 x 264: 17.8 vs 21.1 us; 96 x 392: 17.5 vs 21.2; 64 x 392: 17.0 vs 16.8)
  const bool fused_small = (B <= SS_ROWS && Nc <= 1024) || (B <= SS_MAXB && Nc <= 256);  // shapes the fused small step keeps (small_step_ok)
  SkPlan p{};
  p.ok = !off && force_tile() < 0 && B <= SK_MAXB && B % 32 == 0 && d % 128 == 0 && d >= 128 && d <= 1024 && Nc >= min_nc &&
         Nc <= 16384 && (no_small || !fused_small);
  p.nt = cdiv(Nc, SK_COLS);
  {
    // sim unit width: 128 columns x 4 ring slots, or 64 columns x 8 slots (twice the units, two thirds of a unit's K range in flight).
    // The narrow unit pays when the wide ones would leave most of the chip idle (B = 32 x Nc = 2112, cfg2 gathered over 8 ranks: 17
    // wide units, step 18.8 -> 17.6 us); with every CU busy it loses (cfg3 per rank, 260 wide units: sim 12.4 vs 11.0 us, and the G
    // launch then folds twice the tile statistics).
    const bool narrow = cdiv(B, SK_ROWS) * cdiv(Nc, SK_COLS) < kNumCU / 2;
    p.scols = (narrow && cdiv(Nc, SK_SCOLS) <= 8 * SK_MAXG) ? SK_SCOLS : SK_COLS;
  }
  p.nts = cdiv(Nc, p.scols);  // statistics tiles = sim units per row block
  p.nrb = cdiv(B, SK_ROWS);
  if (!p.ok) return p;  // (also keeps d < 64 away from the division below: every entry point derives this plan for its workspace layout)
  const int nk = cdiv(Nc, 64), ndt = d / SK_QN;
  int ns = kNumCU / 2 / ndt;  // dQ units: (slice of contexts) x (64 columns of d); ~half a unit per CU measured best: the
  if (nk <= 8) ns = 1;  // up to 512 contexts one slice is short enough, and it needs no partial sums and no reduction launch (128 x 264: 17.8 -> 15.7 us;
                        // at 520 contexts it is a tie, beyond that the unsplit units are the launch's long pole)
  if (ns < 1) ns = 1;         // units run next to the dC units, and fewer slices mean fewer partial sums to write and re-read
  if (ns > 64) ns = 64;   // bounds the fp32 partial traffic
  p.ksteps = cdiv(nk, ns);
  p.nslices = cdiv(nk, p.ksteps);
  return p;
}

// The few-rows step without its dScores launch (skinny.h, round 4: sk_sim_kernel writes the tile-local softmax, sk_bwdf_kernel derives
// the row logsumexp and the per-tile factors itself).  nts = statistics tiles, nk = 64-context steps of the dQ units (tile space: the
// packed layout's remapped tiles skip the header rows).  128-column statistics tiles only (a dC unit is one tile), at most 128 of
// them, the dQ slices as the plan cut them and short enough for a unit's factor table (SK_FT tiles).
// Where it is chosen (option sk_fused = 1): B x Nc >= 2^19 -- measured with eight-wave units (profiles/r04_rank_shapes_w8.txt, one box, us per
// step without / with the dScores launch): 128 x 8256 x 768 25.4-26.1 / 29.5; 128 x 6208 x 768 23.7 / 25.5; 128 x 4160 x 768 21.9 / 22.4;
// 128 x 4160 x 1024 23.2 / 24.9; 128 x 8256 x 256 18.8 / 20.2; 96 x 6208 x 768 22.6 / 24.2; 64 x 8256 x 512 / 768 / 1024 20.6 / 20.8,
// 23.4 / 25.7, 29.6 / 32.4; below 2^19 scores (128 x 2112, 64 x 4160) the two plans tie.  (With four-wave units the plan lost below
// 2^20: r04_fused_ab.txt.)  What it always buys is accuracy: the gold terms stay in fp32 (gradients 3e-5 of max |grad| from an fp64
// reference instead of 1e-3).
struct SkFused { bool ok; int ksteps, nslices; bool pair; int tpu, ns; };  // nslices x ksteps: the dQ units' slices; pair: sk_bwdp_kernel with ns slices of tpu statistics tiles
SkFused sk_fused_plan(const SkPlan& sk, int nts, int nk, int B, int Nc, int d) {
  SkFused f{false, 0, 0, false, 0, 0};
  const int mode = opt(OPT_SK_FUSED);
  if (mode == 0 || (mode == 1 && (long)B * Nc < (1l << 19))) return f;
  if (!sk.ok || sk.scols != SK_COLS || nts > 128 || sk.nslices < 1 || sk.nslices > 64) return f;
  f.nslices = sk.nslices;
  f.ksteps = cdiv(nk, f.nslices);  // (a tiling with fewer steps may leave the last slices empty: their units write zero slabs)
  if ((f.ksteps + 1) / 2 + 1 > SK_FT) {
    // the plan's slices span more statistics tiles than a dQ unit's factor table holds (long rows, or few slices at d = 1024).
    // This form can cut its own, 13 steps each (7 tiles + 1) -- but those are shapes with more workgroups than the chip holds at
    // once, and there it measured SLOWER than the plan with the dScores launch (128 x 12352 x 768: 40.0 against 35.7 us;
    // 128 x 8256 x 1024: 33.6 / 31.8; 64 x 8256 x 1024: 30.2 / 29.6): only on request (sk_fused = 2)
    if (mode != 2) return f;
    f.ksteps = 2 * (SK_FT - 1) - 1;
    f.nslices = cdiv(nk, f.ksteps);
  }
  f.ok = f.nslices <= 64 && (f.ksteps + 1) / 2 + 1 <= SK_FT;
  if (f.ok && opt(OPT_SK_PAIR) != 0 && d % SK_QN == 0) {
    // one workgroup per CU (152 KiB of LDS each): at most kNumCU units, at most 16 slabs (one batch of the finishing launch's loads)
    const int ndt = d / SK_QN;
    int maxs = kNumCU / ndt;
    if (maxs > 16) maxs = 16;
    if (maxs < 1) maxs = 1;
    f.tpu = cdiv(nts, maxs);
    f.ns = cdiv(nts, f.tpu);
    f.pair = f.tpu <= SK_PT;
  }
  return f;
}

struct FwdPlan { bool short_rows; int tile, splits, kchunk, nt, tpr, cpt, threads, blocks; };
FwdPlan fwd_plan(int B, int Nc, int d);

// workspace carve-up (all offsets 256-byte aligned); fp and sk are the shape's fwd_plan and sk_plan
struct WsLayout {
  size_t header, gold, lse, rloss, part_m, part_s, logits, dq_part, total;
};
WsLayout ws_layout(int B, int Nc, int d, const FwdPlan& fp, const SkPlan& sk) {
  WsLayout w;
  const size_t ntmax = (size_t)cdiv(Nc, 32);
  size_t off = 0;
  w.header = off; off += 256;
  w.gold = off; off += align256((size_t)B * 4);
  w.lse = off; off += align256((size_t)B * 4);    // no-logits forward: row logsumexp for the dScores pass / rank: gold logits
  w.rloss = off; off += align256((size_t)B * 4);  // no-logits forward: row losses / rank: counts
  w.part_m = off; off += align256((size_t)B * ntmax * 4);
  w.part_s = off; off += align256((size_t)B * ntmax * 4);
  {
    // short rows: split-K slabs of partial logits (4, or up to 32 for wide vectors)
    const size_t slabs = (Nc <= 4096 && (B <= 64 || fp.short_rows)) ? (size_t)(fp.short_rows && fp.splits > 4 ? fp.splits : 4) : 1;
    // no-logits shapes: the forward never stores S (a caller who wants the logits passes S_out)
    w.logits = off; off += nl_ok(B, Nc, d) ? 0 : align256((size_t)B * Nc * 4 * slabs);
  }
  const DqPlan p = dq_plan(B, Nc, d);
  int slabs = sk.ok && sk.nslices > p.splits ? sk.nslices : p.splits;
  {
    const Pair128Plan pp = pair128_plan(B, Nc, d);
    if (pp.ok && pp.splits > slabs) slabs = pp.splits;
  }
  if (sk.ok && slabs < 16) slabs = 16;  // (sk_bwdp_kernel: up to 16 slices)
  if (sk.ok && slabs < cdiv(cdiv(Nc, 64), 2 * (SK_FT - 1) - 1)) slabs = cdiv(cdiv(Nc, 64), 2 * (SK_FT - 1) - 1);  // (sk_fused_plan's own slices)
  w.dq_part = off; off += align256((size_t)slabs * B * d * 4);
  w.total = off;
  return w;
}

// Forward plan, a pure function of the shape (both forward launches derive it independently).
//  short rows (the BASELINE training shapes): sim split over K into `splits` slabs, softmax with the row in registers
//  long rows: sim with per-tile statistics, then the streaming gfinal kernel
FwdPlan fwd_plan(int B, int Nc, int d) {
  FwdPlan p{};
  // wide: vocabulary-wide vectors (CITADEL router, d = 30522): the contraction is long and the logit matrix small -- the
  // K range is what has to be spread over the chip (B = 128, Nc = 1024 are only 32 tiles of 64 x 64)
  const bool wide = d >= 4096 && Nc <= 4096 && B <= 256;
  p.short_rows = Nc <= 4096 && (B <= 64 || wide) && force_tile() < 0;
  if (!p.short_rows) {
    p.tile = (force_tile() < 0 && big_ok(B, Nc, d)) ? kBigTile : pick_tile(B, Nc, d, 1, 2 * kNumCU);
    p.splits = 1;
    p.kchunk = cdiv(d, kTiles[p.tile].bk) * kTiles[p.tile].bk;
    p.nt = cdiv(Nc, kTiles[p.tile].bn);
    return p;
  }
  p.tile = B <= 32 ? (d >= 256 ? 5 : 3) : 2;
  if (wide && B >= 128) p.tile = 2;  // 64 x 64 (128 x 128 with twice the slabs measured within 5 %: the fp32 ingest is the limiter)
  const int bk = kTiles[p.tile].bk, ksteps = cdiv(d, bk);
  int splits = ksteps < 4 ? ksteps : 4;
  if (wide) {  // one 128 x 128 tile per CU (wide.h; the register-staged kernel then gets more, thinner workgroups), at least 4 K steps
               // each, at most 32 slabs of partial logits
    const int per_split = cdiv(B, WD_B) * cdiv(Nc, WD_B);
    splits = cdiv(kNumCU, per_split);
    if (splits > ksteps / 4) splits = ksteps / 4;
    if (splits > 32) splits = 32;
    if (splits < 4) splits = 4;
  }
  // 768 < Nc <= SS_MAXNC (the BASELINE shape gathered over 3..4 ranks): enough column tiles without a K split, and
  // every workgroup of the fused softmax+backward kernel that follows re-reads the logits -- one slab, not four.  (Up to 768
  // columns the K split still pays: 32 x 528, cfg2 over two ranks, 13.25 -> 12.85 us; 32 x 648 13.75 -> 13.55.)
  if (B <= SS_ROWS && Nc > 768 && Nc <= SS_MAXNC) splits = 1;
  p.kchunk = cdiv(ksteps, splits) * bk;
  p.splits = cdiv(d, p.kchunk);
  const int cpr = Nc / 8;
  p.cpt = cpr > 256 ? 2 : 1;
  int tpr = 16;
  while (tpr * p.cpt < cpr) tpr <<= 1;
  p.tpr = tpr;
  int rpb = 1024 / tpr;
  if (rpb > B) rpb = B;
  if (p.splits > 4 && rpb > cdiv(B, 128)) rpb = cdiv(B, 128);  // many slabs: the launch is the slab read (up to 16 MB) -- >= 128 workgroups
  if (rpb < 1) rpb = 1;
  p.threads = rpb * tpr;
  p.blocks = cdiv(B, rpb);
  return p;
}

// the LDS-DMA fp32 sim (wide.h): vocabulary-wide short-row shapes whose K chunks are whole 32-float steps and whose operands are
// addressable with 32-bit byte offsets
bool wide_sim_ok(int B, int Nc, int d, const FwdPlan& fp) {
  return !opt(OPT_NO_WIDE) && d >= 4096 && Nc <= 4096 && B <= 256 && fp.short_rows && d % WD_KS == 0 && fp.kchunk % WD_KS == 0 &&
         (double)Nc * d * 4 < 4.0e9 && (double)B * d * 4 < 4.0e9;
}

// backward of the same shape class on the units of skinny.h (dprhot_inbatch_bwd): rows in blocks of 32 up to 128, vectors in whole
// 64-column dQ tiles, contexts within one dQ slice (<= 24 ring steps of 64), 32-bit element offsets
bool wide_bwd_ok(int B, int Nc, int d) {
  return !opt(OPT_NO_WIDE_BWD) && !opt(OPT_NO_SKINNY) && force_tile() < 0 && d >= 4096 && d % 64 == 0 && B <= SK_MAXB &&
         B % 32 == 0 && Nc % 8 == 0 && Nc >= 64 && Nc <= 1536 && (double)Nc * d < 4.0e9;
}

// The barrier-free sim launch (sim_small.h) takes the short-row plan's tile 5 where every K chunk is one whole 256-deep step of a
// wave: B <= 32, d a multiple of 256, kchunk == 256 (so not the single-slab plan above 768 columns, whose one chunk is all of d: a
// wave would chain d / 32 MFMAs behind 2 x 16 x d x 4 bytes of loads -- it stays on the engine).  Shapes it takes are the ones it was
// measured at (profiles/small_sim_ab.txt): d = 768 and 1024, up to 768 columns.
bool small_sim_ok(int B, int Nc, int d, const FwdPlan& fp) {
  return opt(OPT_SMALL_SIM) != 0 && force_tile() < 0 && fp.short_rows && fp.tile == 5 && B <= 32 && fp.kchunk == SMS_KC && d % SMS_KC == 0 &&
         d >= 768 && d <= 1024 && Nc <= 768 && fp.splits * SMS_KC == d;
}
int launch_sim_small(bool b_f32, const GemmArgs& a, const EpiSim& epi, int splits, hipStream_t st) {
  const int v = opt(OPT_SMALL_SIM);
  const int form = (v == 2 || v == 4) ? SS_REG : SS_PATCH, wpg = (v == 3 || v == 4) ? 2 : 1;
  // an exact 3-D grid (row tile x wpg, column tile, K chunk): the kernel takes its tile from the block index, without a division
  const int nrt = cdiv(a.M, 16), nct = cdiv(a.N, 16);
  const size_t lds = sim_small_lds(form, b_f32, wpg);
  if (v == 1 && opt(OPT_SMALL_SIM_COPY) != 0) {
    // the copies on waves of their own: `splits` layers of copy waves behind the compute waves, one wave per operand tile and chunk
    // (C tiles only where the contexts are fp32 and have a copy) -- two layers per chunk where a layer of the grid is smaller than that
    const int units = (b_f32 && a.Bcopy != nullptr ? nct : 0) + (a.Acopy != nullptr ? nrt : 0);
    const dim3 grid(nrt, nct, splits + cdiv(units, nrt * nct) * splits), block(64);
    if (opt(OPT_SMALL_SIM_COPY) != 2)  // write-through copies (a template argument, not a branch in the kernel)
      return b_f32 ? launch<sim_small_split_kernel<true, 1>>(grid, block, lds, st, splits, a, epi)
                   : launch<sim_small_split_kernel<false, 1>>(grid, block, lds, st, splits, a, epi);
    return b_f32 ? launch<sim_small_split_kernel<true>>(grid, block, lds, st, splits, a, epi)
                 : launch<sim_small_split_kernel<false>>(grid, block, lds, st, splits, a, epi);
  }
  const dim3 grid(cdiv(nrt, wpg), nct, splits), block(64 * wpg);
  if (form == SS_REG)
    return b_f32 ? launch<sim_small_kernel<true, SS_REG>>(grid, block, lds, st, wpg, a, epi)
                 : launch<sim_small_kernel<false, SS_REG>>(grid, block, lds, st, wpg, a, epi);
  return b_f32 ? launch<sim_small_kernel<true, SS_PATCH>>(grid, block, lds, st, wpg, a, epi)
               : launch<sim_small_kernel<false, SS_PATCH>>(grid, block, lds, st, wpg, a, epi);
}

// the latency-bound shapes of the one-call step (step_small.h)
bool small_step_ok(int B, int Nc, int d, const FwdPlan& fp) {
  // two row blocks (32 < B <= 64) up to 256 columns only -- measured (scratch/rb_probe.py, two launches against three): 64 x 256 x 768
  // 13.3 against 16.2 us, 64 x 128 x 1024 13.5 / 14.0, but 64 x 512 18.6 / 17.5 and 64 x 768 24.0 / 22.8: every workgroup repeats
  // BOTH blocks' softmax, and beyond 256 columns that second helping costs more than the launch it saves
  return !opt(OPT_NO_SMALL_STEP) && B <= SS_MAXB && Nc <= (B <= SS_ROWS ? SS_MAXNC : 256) && d % 16 == 0 && fp.short_rows && fp.splits <= 4;
}

// The plan of one shape, derived once per call: what dprhot_inbatch_step_f32 runs there; every entry point of the family, the host queries
// (dprhot_step_wants_g, dprhot_train_dq_slabs, dprhot_fwd_one_pass, dprhot_fwd_no_logits) and step_admit read their answers from it.
enum StepFamily { FAM_FEW_ROWS, FAM_SMALL_STEP, FAM_GENERAL };                                   // sk_step / step_small / forward + backward
enum FwdKind { FWD_ONE_PASS_128, FWD_ONE_PASS_256, FWD_NO_LOGITS, FWD_SHORT_ROWS, FWD_TILED };  // the general family's forward
struct StepPlan {
  StepFamily family;
  bool nl, nl128;  // nl_ok, nl128_ok
  FwdPlan fp;
  SkPlan sk;
  SkFused fz;  // judged on the plain column tiling: the packed layout's remapped tiles are never more and their slices never longer
  WsLayout wl;
  FwdKind fwd(bool logits, bool g) const {  // the forward of a call that wants the logits stored / the dScores
    if (!logits && g && nl128) return FWD_ONE_PASS_128;
    if (!logits && g && nl && opt(OPT_NL_P16) != 0) return FWD_ONE_PASS_256;
    if (!logits && nl) return FWD_NO_LOGITS;
    return fp.short_rows ? FWD_SHORT_ROWS : FWD_TILED;
  }
  // split-K slabs of dQ the step can leave to its caller: the few-rows plan's, unless it runs without the dScores (slice-normalised slabs
  // need the row statistics to be combined: the step's own finishing launch)
  int dq_slabs() const { return sk.ok && sk.nslices > 1 && !fz.ok ? sk.nslices : 0; }
};
StepPlan step_plan(int B, int Nc, int d) {
  StepPlan p;
  p.fp = fwd_plan(B, Nc, d);
  p.sk = sk_plan(B, Nc, d);
  p.fz = sk_fused_plan(p.sk, cdiv(Nc, SK_COLS), cdiv(Nc, 64), B, Nc, d);
  p.family = p.sk.ok ? FAM_FEW_ROWS : (small_step_ok(B, Nc, d, p.fp) ? FAM_SMALL_STEP : FAM_GENERAL);
  p.nl = nl_ok(B, Nc, d);
  p.nl128 = nl128_ok(B, Nc, d);
  p.wl = ws_layout(B, Nc, d, p.fp, p.sk);
  return p;
}

// the workspace of an entry point of the family (needed: this call's plan touches it; align: the entry point insists on 16-byte alignment)
int claim_ws(const char* who, const WsLayout& wl, void* workspace, size_t workspace_bytes, bool needed, bool align, char** ws) {
  *ws = static_cast<char*>(workspace);
  if (!needed) return DPRHOT_OK;
  if (workspace == nullptr || workspace_bytes < wl.total)
    return fail(DPRHOT_E_WORKSPACE, "%s needs %zu workspace bytes, got %zu", who, wl.total, workspace_bytes);
  REQUIRE(!align || aligned16(workspace), "workspace must be 16-byte aligned");
  return DPRHOT_OK;
}

// the loss launch of the no-logits forward -- or, inside the one-call step, a note for launch_slab_sum
int launch_loss_sum(const float* src, int n, float scale, float* out, hipStream_t st, LossDefer* defer) {
  if (defer != nullptr && defer->armed) {
    defer->pending = true;
    defer->src = src; defer->n = n; defer->scale = scale; defer->out = out;
    return DPRHOT_OK;
  }
  return launch<reduce_sum_kernel>(dim3(1), dim3(256), 0, st, src, n, scale, out);
}

// the row kernel of the one-pass forwards (128 x 128 and 256 x 256 tiles): logsumexp / loss from the strip statistics, and the fp16 numerators
// rescaled into the bf16 dScores in place
int launch_lse_p2g(const float* part_m, const float* part_s, int npart, int B, int Nc, const int64_t* y, int64_t y_offset, float grad_scale,
                   float* row_lse, float* row_loss, dprhot_bf16* G, char* ws, const WsLayout& wl, hipStream_t st) {
  return launch<g8_lse_p2g_kernel>(dim3((unsigned)B), dim3(256), 0, st, part_m, part_s, npart, reinterpret_cast<const float*>(ws + wl.gold), B, Nc, y,
                                   y_offset, grad_scale, reinterpret_cast<float*>(ws + wl.lse), row_lse, row_loss, reinterpret_cast<float*>(ws + wl.rloss), G);
}

// dQ = scale * (slab 0 + slab 1 + ...), in slab order; inside the one-call step the same launch also forms the loss sum (launch_loss_sum)
int launch_slab_sum(const float* part, int splits, int B, int d, float h_scale, const float* d_scale, float* dQ, hipStream_t st, LossDefer* defer) {
  const size_t n4 = (size_t)B * d / 4;
  const int blocks = (int)((n4 + 255) / 256 > 1024 ? 1024 : (n4 + 255) / 256);
  if (defer != nullptr && defer->pending) {
    defer->pending = false;
    return launch<splitk_reduce_loss_kernel>(dim3(blocks + 1), dim3(256), 0, st, part, splits, n4, h_scale, d_scale, dQ, defer->src, defer->n,
                                             defer->scale, defer->out);
  }
  return launch<splitk_reduce_kernel>(dim3(blocks), dim3(256), 0, st, part, splits, n4, h_scale, d_scale, dQ);
}

// dQ = G x C on the plan p (dq_plan): the split-K GEMM (gemm_too) and the sum of its slabs
int launch_dq(DqPlan p, const dprhot_bf16* G, const dprhot_bf16* C, int B, int Nc, int d, float h_scale, const float* d_scale, float* dQ,
              char* ws, const WsLayout& wl, hipStream_t st, bool gemm_too, LossDefer* defer) {
  if (p.big) p.tile = 0;  // stand-alone dQ (dprhot_dq): same K slices on the 128x128 tile
  if (gemm_too) {
    GemmArgs a{G, C, B, d, Nc, Nc, d, p.kchunk};
    if (p.splits == 1) {
      EpiScaleF32 epi{dQ, B, d, h_scale, d_scale};
      return launch_gemm<true, false>(p.tile, a, epi, 1, st);
    }
    EpiScaleF32 epi{reinterpret_cast<float*>(ws + wl.dq_part), B, d, 1.0f, nullptr};
    if (int rc = launch_gemm<true, false>(p.tile, a, epi, p.splits, st)) return rc;
  }
  if (p.splits > 1) return launch_slab_sum(reinterpret_cast<const float*>(ws + wl.dq_part), p.splits, B, d, h_scale, d_scale, dQ, st, defer);
  return DPRHOT_OK;
}

// ---- few rows x many contexts: the four launches of skinny.h -------------------------------------------------------
template <int NCH, int COLS, int SLOTS>
int launch_sk_sim_c(const SkSimArgs& a, int grid, hipStream_t st) {
  const size_t lds = sk_sim_lds();
  if (a.q == nullptr) return launch<sk_sim_kernel<NCH, false, COLS, SLOTS>>(dim3((unsigned)grid), dim3(SK_THREADS), lds, st, a);
  if constexpr (COLS == SK_COLS) {  // fp32 q at 128-column units: eight waves per workgroup
    if (grid <= kNumCU) {
      // wave-private rings and no barrier in the K loop, one workgroup per CU (round 5): as many chunks in flight per wave as 160 KiB of
      // LDS hold next to the q block
      constexpr int PS = NCH <= 12 ? 6 : (NCH <= 14 ? 5 : 4);
      return launch<sk_simp_kernel<NCH, PS>>(dim3((unsigned)grid), dim3(512), sk_simp_lds(NCH, PS), st, a);
    }
    return launch<sk_sim_kernel<NCH, true, COLS, SLOTS, 8>>(dim3((unsigned)grid), dim3(512), lds, st, a);
  } else {
    return launch<sk_sim_kernel<NCH, true, COLS, SLOTS>>(dim3((unsigned)grid), dim3(SK_THREADS), lds, st, a);
  }
}
template <int NCH>
int launch_sk_sim(const SkSimArgs& a, int grid, int scols, hipStream_t st) {
  return scols == SK_COLS ? launch_sk_sim_c<NCH, SK_COLS, SK_SLOTS>(a, grid, st) : launch_sk_sim_c<NCH, SK_SCOLS, 2 * SK_SLOTS>(a, grid, st);
}

// the backward units of skinny.h (dC tiles next to split-K dQ tiles, `units` workgroups) and the sum of the dQ slabs behind them:
// the launches sk_step and dprhot_inbatch_bwd share
int launch_sk_bwd(const SkBwdArgs& b, int units, hipStream_t st) {
  return launch<sk_bwd_kernel>(dim3((unsigned)units), dim3(SK_THREADS), sk_bwd_lds(), st, b);
}
int launch_sk_dq_reduce(const float* part, int nslices, int B, int d, float h_scale, const float* d_scale, float* dQ, hipStream_t st) {
  const size_t n4 = (size_t)B * d / 4;
  return launch<sk_dq_reduce_kernel>(dim3((unsigned)((n4 + 63) / 64)), dim3(256), 0, st, part, nslices, n4, h_scale, d_scale, dQ);
}

int sk_step(const StepCtx& cx, const float* q, const dprhot_bf16* Cb, dprhot_bf16* Qb, int B, int Nc, int d, const int64_t* y, int64_t y_offset,
            const uint8_t* colmask, float inv_T, float grad_scale, float h_scale, const float* d_scale, float* S_out, float* row_loss,
            float* row_lse, float* loss_sum, dprhot_bf16* G, float* dQ, float* dC_part, char* ws, const WsLayout& wl, const SkPlan& sk,
            hipStream_t st) {
  const PackedSpec& pk = cx.packed;
  float* S = S_out ? S_out : reinterpret_cast<float*>(ws + wl.logits);
  float* tile_lse = reinterpret_cast<float*>(ws + wl.part_m);
  float* gold = reinterpret_cast<float*>(ws + wl.gold);
  // packed layout whose ranks hold a whole number of sim tiles: only the real rows are multiplied (SkSimArgs::tiles_per_rank)
  const bool remap = pk.base != nullptr && pk.rows_c > pk.n_ctx && pk.n_ctx % sk.scols == 0 &&
                     Nc % pk.rows_c == 0;
  const int tpr = remap ? pk.n_ctx / sk.scols : 0;
  const int nts = remap ? (Nc / pk.rows_c) * tpr : sk.nts;
  SkSimArgs a{q, nullptr, Cb, Qb, B, Nc, d, y, y_offset, colmask, inv_T, S, tile_lse, gold, pk.base, pk.rows_c,
              pk.n_ctx, pk.row_bytes, tpr};
  // G == NULL (nobody wants the dScores): three launches -- the sim launch leaves the tile-local softmax in the logit workspace
  const int nk_f = remap ? 2 * nts : cdiv(Nc, 64);
  const SkFused fz = sk_fused_plan(sk, nts, nk_f, B, Nc, d);
  const bool fused = G == nullptr && S_out == nullptr && fz.ok;
  if (G == nullptr && !fused) return fail(DPRHOT_E_INVALID, "few-rows step: G == NULL needs the fused-dScores plan (dprhot_step_wants_g)");
  // the finishing role inside the backward launch (sk_fin_unit): two-kinds form only
  const bool tail = fused && !fz.pair && opt(OPT_SK_TAIL) != 0 && fz.nslices <= 62 && d <= 1024;
  unsigned* const tail_cnt = reinterpret_cast<unsigned*>(ws + wl.header + 128);
  // round 6: no finishing launch at all -- the dQ units add their tiles into dQ, zero-filled by the sim launch (two-kinds form, dQ wanted)
  const bool dq_atomic = fused && !fz.pair && !tail && opt(OPT_SK_DQ_ATOMIC) != 0 && opt(OPT_SK_W8) != 0 && dQ != nullptr;
  if (fused) {
    a.S = nullptr;
    a.P = reinterpret_cast<uint16_t*>(ws + wl.logits);
    if (tail) a.zero_me = tail_cnt;
    if (dq_atomic) {
      a.zero_dq = dQ;
      a.zero_n4 = (int)((size_t)B * d / 4);
    }
  }
  const int grid1 = sk.nrb * nts;
  int rc = DPRHOT_OK;
  switch (d / 128) {  // NCH = d / 64
    case 1: rc = launch_sk_sim<2>(a, grid1, sk.scols, st); break;
    case 2: rc = launch_sk_sim<4>(a, grid1, sk.scols, st); break;
    case 3: rc = launch_sk_sim<6>(a, grid1, sk.scols, st); break;
    case 4: rc = launch_sk_sim<8>(a, grid1, sk.scols, st); break;
    case 5: rc = launch_sk_sim<10>(a, grid1, sk.scols, st); break;
    case 6: rc = launch_sk_sim<12>(a, grid1, sk.scols, st); break;
    case 7: rc = launch_sk_sim<14>(a, grid1, sk.scols, st); break;
    case 8: rc = launch_sk_sim<16>(a, grid1, sk.scols, st); break;
    default: return fail(DPRHOT_E_UNSUPPORTED, "skinny step: d=%d", d);
  }
  if (rc) return rc;
  if (fused) {
    if (cx.dq_part != nullptr) return fail(DPRHOT_E_INVALID, "few-rows step without dScores: dQ is finished by the step itself (dprhot_train_dq_slabs = 0)");
    float* part = reinterpret_cast<float*>(ws + wl.dq_part);
    const int ndq = fz.nslices * (d / SK_QN), ndq_pad = (ndq + 7) & ~7, ndc = nts * (d / SK_DN);
    SkBwdFArgs b{a.P, Qb, Cb, B, Nc, d, tile_lse, gold, y, y_offset, nts, tpr, pk.rows_c, pk.n_ctx, grad_scale, h_scale, d_scale,
                 dC_part, cx.dc_bf16 ? 1 : 0, pk.stamp_src != nullptr ? pk.rows_c : 0, pk.n_ctx, loss_sum, cx.loss_scale,
                 row_loss, row_lse, fz.ksteps, fz.nslices, part, dQ, ndq_pad, /*nt_store=*/1, /*dbg=*/0};
    b.reg_scale = opt(OPT_SK_DC_REGSCALE) != 0 ? 1 : 0;
    b.dq_atomic = dq_atomic ? 1 : 0;
    const size_t lds = sk_bwdf_lds();
    if (fz.pair) {
      // one kind of unit: (slice of fz.tpu statistics tiles) x (64 columns of d), one workgroup per CU
      b.ksteps = fz.tpu;
      b.nslices = fz.ns;
      const size_t ldsp = sk_bwdp_lds();
      const dim3 gridp((unsigned)(fz.ns * (d / SK_QN)));
      rc = nts <= 64 ? launch<sk_bwdp_kernel<8>>(gridp, dim3(512), ldsp, st, b) : launch<sk_bwdp_kernel<16>>(gridp, dim3(512), ldsp, st, b);
    } else {
      const bool w8 = opt(OPT_SK_W8) != 0;
      const int threads = w8 ? 512 : SK_THREADS;
      if (tail) {
        b.tail_cnt = tail_cnt;
        b.nfin = cdiv(B, threads / 256);
        b.tail_fence = opt(OPT_SK_TAIL) == 2 ? 1 : 0;
      }
      const dim3 grid((unsigned)(ndq_pad + ndc + b.nfin)), block((unsigned)threads);  // (b.nfin == 0 without the finishing role)
      if (dq_atomic)  // (eight-wave units only: the form production runs)
        rc = nts <= 64 ? launch<sk_bwdf_kernel<8, 8, true>>(grid, block, lds, st, b) : launch<sk_bwdf_kernel<16, 8, true>>(grid, block, lds, st, b);
      else if (nts <= 64) rc = w8 ? launch<sk_bwdf_kernel<8, 8>>(grid, block, lds, st, b) : launch<sk_bwdf_kernel<8, 4>>(grid, block, lds, st, b);
      else rc = w8 ? launch<sk_bwdf_kernel<16, 8>>(grid, block, lds, st, b) : launch<sk_bwdf_kernel<16, 4>>(grid, block, lds, st, b);
    }
    if (rc) return rc;
    if (!tail && !dq_atomic) {
      // one workgroup per row where the row fits 256 threads (d <= 1024): the row's statistics are derived once, not once per part
      const int fthreads = d / 4 >= 256 ? 256 : cdiv(d / 4, 64) * 64;
      const int parts = cdiv(d / 4, fthreads);
      SkFinArgs f{part, fz.pair ? fz.ns : fz.nslices, fz.ksteps, nk_f, B, d, tile_lse, nts, gold, y, y_offset, Cb, grad_scale, h_scale, d_scale, dQ, parts,
                  fz.pair ? 1 : 0};
      return launch<sk_dq_finish_kernel>(dim3((unsigned)(B * parts)), dim3((unsigned)fthreads), 0, st, f);
    }
    return DPRHOT_OK;
  }
  float* rl = row_loss ? row_loss : reinterpret_cast<float*>(ws + wl.rloss);  // the backward launch forms the loss from the row losses
  {
    const int parts = B >= 128 ? 2 : (B >= 64 ? 4 : 8);  // >= 256 workgroups; a part is at most 4 x 256 chunks of 8 columns
    int pp = parts;
    while (cdiv(Nc / 8, pp) > 4 * SK_THREADS) pp *= 2;
    SkGArgs g{S, tile_lse, gold, nts, B, Nc, y, y_offset, grad_scale, G, rl, row_lse, pp};
    if ((rc = launch<sk_g_kernel>(dim3((unsigned)(B * pp)), dim3(SK_THREADS), 0, st, g))) return rc;
  }
  {
    float* part = cx.dq_part != nullptr ? cx.dq_part : reinterpret_cast<float*>(ws + wl.dq_part);
    const int ndq = sk.nslices * (d / SK_QN), ndq_pad = (ndq + 7) & ~7, ndc = sk.nt * (d / SK_DN);
    SkBwdArgs b{G, Qb, Cb, B, Nc, d, h_scale, d_scale, dC_part, rl, loss_sum, cx.loss_scale, cx.dc_bf16 ? 1 : 0,
                pk.stamp_src != nullptr ? pk.rows_c : 0, pk.n_ctx, sk.ksteps, sk.nslices, part, dQ, ndq_pad, /*nt_store=*/1};
    if ((rc = launch_sk_bwd(b, ndq_pad + ndc, st))) return rc;
    // (else the caller's finishing launch forms dQ from the slabs: dprhot_rescale_grads; one slice: the dQ units stored the scaled sum themselves)
    if (cx.dq_part == nullptr && sk.nslices > 1) return launch_sk_dq_reduce(part, sk.nslices, B, d, h_scale, d_scale, dQ, st);
  }
  return DPRHOT_OK;
}

// ---- the training step: the bodies of its public entry points.  A body takes the call's context (or the part it reads), the shape's plan
// and the claimed workspace; it validates nothing and calls no member of the family through its public name ------------------------------

int sim_fwd_body(const PackedSpec& pk, const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const uint8_t* colmask, float inv_T,
                 float* S, hipStream_t st) {
  const SimGemm g = sim_gemm(B, Nc, d);
  if (g.g8) {
    // large score matrices (validation with the logits wanted, the head chunk of a retrieval): the phase-interleaved kernel with
    // the store epilogue that writes whole rows (Epi8Store)
    Epi8Store epi;
    static_cast<Epi8Base&>(epi) = g8_base(pk, Q, B, Nc, nullptr, 0, colmask, inv_T, nullptr);
    epi.S = S;
    GemmArgs a8{Q, C, B, Nc, d, d, d, d};
    return launch_g8<Epi8Store, 2>(a8, epi, st);
  }
  const int tile = g.tile;
  GemmArgs a{Q, C, B, Nc, d, d, d, g.kchunk};
  EpiSim epi{S, colmask, B, Nc, inv_T, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0};
  epi = with_packed_mask(pk, epi);
  return launch_gemm<true, true>(tile, a, epi, 1, st);
}

int dc_body(const PackedSpec& pk, const dprhot_bf16* G, const dprhot_bf16* Q, int B, int Nc, int d, float h_scale, const float* d_scale,
            float* dC_part, hipStream_t st) {
  // A(m = ctx column, k = query row) = G[k][m]  (mn-major, lda = Nc);  B(k, n) = Q[k][n]  (mn-major, ldb = d)
  GemmArgs a{G, Q, Nc, d, B, Nc, d, cdiv(B, 64) * 64};
  const EpiScaleF32 epi = with_loss_stamp(pk, EpiScaleF32{dC_part, Nc, d, h_scale, d_scale});
  const int tile = force_tile() >= 0 && force_tile() <= 3 ? force_tile() : dc_tile(B, Nc, d);
  return launch_gemm<false, false>(tile, a, epi, 1, st);
}

// bf16 copies of the fp32 operands in one launch (c == NULL: the contexts are bf16 already)
int cast_operands(const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d, hipStream_t st) {
  return c != nullptr ? dprhot_prep(q, (size_t)B * d, Qb, c, (size_t)Nc * d, Cb, st) : dprhot_cast_bf16(q, Qb, (size_t)B * d, st);
}

// launch 1 of the fused forward: logits + per-tile softmax statistics + gold logit (and clears the loss
// accumulator words the next launch adds into)
int sim_stats_body(const PackedSpec& pk, const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                   const uint8_t* colmask, float inv_T, float* S_out, const StepPlan& p, char* ws, hipStream_t st) {
  const WsLayout& wl = p.wl;
  if (S_out == nullptr && p.nl) {
    // no-logits plan: strip statistics + gold logit only; softmax_finish_body turns them into logsumexp / loss and
    // dscores_body recomputes the logits into G
    Epi8Stats epi;
    static_cast<Epi8Base&>(epi) = g8_base(pk, Q, B, Nc, y, y_offset, colmask, inv_T, reinterpret_cast<float*>(ws + wl.gold));
    epi.part_m = reinterpret_cast<float*>(ws + wl.part_m);
    epi.part_s = reinterpret_cast<float*>(ws + wl.part_s);
    epi.npart = cdiv(Nc, G2_B) * 4;
    GemmArgs a8{Q, C, B, Nc, d, d, d, d};
    return launch_g8(a8, epi, st);
  }
  const FwdPlan& fp = p.fp;
  GemmArgs a{Q, C, B, Nc, d, d, d, fp.kchunk};
  if (fp.short_rows) {  // partial logits per K split; the softmax launch sums them (and fills S_out if asked)
    EpiSim epi{reinterpret_cast<float*>(ws + wl.logits), colmask, B, Nc, inv_T, nullptr, nullptr, nullptr, 0, nullptr,
               reinterpret_cast<unsigned long long*>(ws + wl.header), 2, (size_t)B * Nc};
    epi = with_packed_mask(pk, epi);
    return launch_gemm<true, true>(fp.tile, a, epi, fp.splits, st);
  }
  float* S = S_out ? S_out : reinterpret_cast<float*>(ws + wl.logits);
  EpiSim epi{S, colmask, B, Nc, inv_T, reinterpret_cast<float*>(ws + wl.part_m), reinterpret_cast<float*>(ws + wl.part_s),
             y, y_offset, reinterpret_cast<float*>(ws + wl.gold), reinterpret_cast<unsigned long long*>(ws + wl.header), 2};
  epi = with_packed_mask(pk, epi);
  return launch_gemm<true, true>(fp.tile, a, epi, 1, st);
}

// launch 1 with fp32 operands: q [B,d] fp32 always; c [Nc,d] fp32 when non-NULL (single rank: no gather), else
// Cb is the (gathered) bf16 input.  Qb (and Cb when c is given) receive the bf16 copies the backward reads.
int sim_stats_f32_body(const PackedSpec& pk, const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d, const int64_t* y,
                       int64_t y_offset, const uint8_t* colmask, float inv_T, float* S_out, const StepPlan& p, char* ws, hipStream_t st) {
  const WsLayout& wl = p.wl;
  if (B > 128) {
    // Beyond the latency-bound sizes reading fp32 operands in the GEMM costs more than it saves (twice the staging
    // registers and bytes per tile, measured 250 vs 580 TFLOP/s at 8192^2): cast once, then the bf16 kernels.
    if (int rc = cast_operands(q, c, Qb, Cb, B, Nc, d, st)) return rc;
    return sim_stats_body(pk, Qb, B, Cb, Nc, d, y, y_offset, colmask, inv_T, S_out, p, ws, st);
  }
  const FwdPlan& fp = p.fp;
  GemmArgs a{reinterpret_cast<const uint16_t*>(q), c ? reinterpret_cast<const uint16_t*>(c) : Cb, B, Nc, d, d, d, fp.kchunk};
  a.Acopy = Qb;
  a.Bcopy = c ? Cb : nullptr;
  if (fp.short_rows) {
    if (c != nullptr && wide_sim_ok(B, Nc, d, fp) && pk.base == nullptr) {
      // vocabulary-wide fp32 operands: LDS-DMA ring of fp32 tiles, bf16 rounding on the fragment read (wide.h)
      WideSimArgs wa{q, c, Qb, Cb, B, Nc, d, colmask, inv_T, reinterpret_cast<float*>(ws + wl.logits), (size_t)B * Nc, fp.kchunk,
                     reinterpret_cast<unsigned long long*>(ws + wl.header), 2, /*no_copy=*/0, cdiv(Nc, WD_B), cdiv(B, WD_B)};
      return launch<wide_sim_kernel>(dim3((unsigned)(wa.nbx * wa.nby * fp.splits)), dim3(WD_THREADS), wd_lds_bytes, st, wa);
    }
    EpiSim epi{reinterpret_cast<float*>(ws + wl.logits), colmask, B, Nc, inv_T, nullptr, nullptr, nullptr, 0, nullptr,
               reinterpret_cast<unsigned long long*>(ws + wl.header), 2, (size_t)B * Nc};
    epi = with_packed_mask(pk, epi);
    if (small_sim_ok(B, Nc, d, fp)) return launch_sim_small(c != nullptr, a, epi, fp.splits, st);
    return c ? launch_sim_f32<true, true>(fp.tile, a, epi, fp.splits, st) : launch_sim_f32<true, false>(fp.tile, a, epi, fp.splits, st);
  }
  float* S = S_out ? S_out : reinterpret_cast<float*>(ws + wl.logits);
  EpiSim epi{S, colmask, B, Nc, inv_T, reinterpret_cast<float*>(ws + wl.part_m), reinterpret_cast<float*>(ws + wl.part_s),
             y, y_offset, reinterpret_cast<float*>(ws + wl.gold), reinterpret_cast<unsigned long long*>(ws + wl.header), 2};
  epi = with_packed_mask(pk, epi);
  return c ? launch_sim_f32<true, true>(fp.tile, a, epi, 1, st) : launch_sim_f32<true, false>(fp.tile, a, epi, 1, st);
}

// launch 2 of the fused forward: logsumexp from the statistics, G in one pass over S, loss numerator
int softmax_finish_body(const StepCtx& cx, const float* S_in, int B, int Nc, int d, const int64_t* y, int64_t y_offset, float grad_scale,
                        float* row_loss, float* row_lse, float* loss_sum, dprhot_bf16* G, const StepPlan& p, char* ws, hipStream_t st) {
  const WsLayout& wl = p.wl;
  if (S_in == nullptr && p.nl) {
    // no-logits plan (same test as sim_stats_body): logsumexp and loss from the strip statistics; there are no logits to turn
    // into G here -- dscores_body recomputes them
    if (int rc = launch<g8_lse_kernel>(dim3(cdiv(B, 4)), dim3(256), 0, st, reinterpret_cast<const float*>(ws + wl.part_m),
                                       reinterpret_cast<const float*>(ws + wl.part_s), cdiv(Nc, G2_B) * 4, reinterpret_cast<const float*>(ws + wl.gold), B,
                                       reinterpret_cast<float*>(ws + wl.lse), row_lse, row_loss, reinterpret_cast<float*>(ws + wl.rloss)))
      return rc;
    return launch_loss_sum(reinterpret_cast<const float*>(ws + wl.rloss), B, cx.loss_scale, loss_sum, st, cx.defer);
  }
  const FwdPlan& fp = p.fp;  // same plan as sim_stats_body -> same intermediate layout
  if (fp.short_rows) {
    // S_in, when given, is where the caller wants the summed logits (the slabs always live in the workspace)
    GShortArgs g{reinterpret_cast<const float*>(ws + wl.logits), fp.splits, (size_t)B * Nc, B, Nc, y, y_offset, grad_scale,
                 const_cast<float*>(S_in), row_loss, row_lse, G, reinterpret_cast<unsigned long long*>(ws + wl.header), loss_sum, fp.tpr, cx.loss_scale};
    if (fp.blocks > 65535) return fail(DPRHOT_E_UNSUPPORTED, "softmax_finish: B=%d rows need %d workgroups (max 65535)", B, fp.blocks);
    if (fp.cpt == 1) return launch<gfinal_short_kernel<1>>(dim3(fp.blocks), dim3(fp.threads), 0, st, g);
    return launch<gfinal_short_kernel<2>>(dim3(fp.blocks), dim3(fp.threads), 0, st, g);
  }
  const float* S = S_in ? S_in : reinterpret_cast<const float*>(ws + wl.logits);
  const int nt = fp.nt;
  if (nt > kGfMaxPairs) return fail(DPRHOT_E_UNSUPPORTED, "Nc=%d too long for the statistics buffer (%d column tiles)", Nc, nt);
  GFinalArgs g{S, B, Nc, y, y_offset, grad_scale, reinterpret_cast<const float*>(ws + wl.part_m),
               reinterpret_cast<const float*>(ws + wl.part_s), nt, reinterpret_cast<const float*>(ws + wl.gold), row_loss, row_lse,
               G, reinterpret_cast<unsigned long long*>(ws + wl.header), loss_sum, cx.loss_scale};
  const bool thin = (long)B * (Nc / 8) <= 1L << 18;  // latency-bound sizes: one chunk per thread, many small workgroups
  int rpb, xblocks;
  gfinal_geometry(Nc, thin ? 1 : 8, &rpb, &xblocks);
  if (cdiv(B, rpb) > 65535)  // grid.y limit, and the arrival ticket of the loss accumulation is 16 bits wide
    return fail(DPRHOT_E_UNSUPPORTED, "softmax_finish: B=%d rows need %d row blocks (max 65535)", B, cdiv(B, rpb));
  dim3 grid(xblocks, cdiv(B, rpb));
  if (thin) return launch<gfinal_kernel<1>>(grid, dim3(256), 0, st, g);
  return launch<gfinal_kernel<8>>(grid, dim3(256), 0, st, g);
}

// dScores of the no-logits forward: G = (softmax(S) - onehot) * grad_scale with S recomputed tile by tile (the same GEMM as
// sim_stats_body, bit-identical accumulators) from the rows' logsumexp
int dscores_body(const PackedSpec& pk, const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                 const uint8_t* colmask, float inv_T, float grad_scale, const float* row_lse, dprhot_bf16* G, hipStream_t st) {
  Epi8G epi;
  static_cast<Epi8Base&>(epi) = g8_base(pk, Q, B, Nc, y, y_offset, colmask, inv_T, nullptr);
  epi.row_lse = row_lse;
  epi.G = G;
  epi.grad_scale = grad_scale;
  GemmArgs a8{Q, C, B, Nc, d, d, d, d};
  return launch_g8<Epi8G, 2>(a8, epi, st);
}

int inbatch_fwd_body(const StepCtx& cx, const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                     const uint8_t* colmask, float inv_T, float grad_scale, float* S_out, float* row_loss, float* row_lse, float* loss_sum,
                     dprhot_bf16* G, const StepPlan& p, char* ws, hipStream_t st) {
  const WsLayout& wl = p.wl;
  const FwdKind kind = p.fwd(S_out != nullptr, G != nullptr);
  if (kind == FWD_ONE_PASS_128 || kind == FWD_ONE_PASS_256) {
    // ONE pass of the GEMM (round 6): strip statistics + fp16 softmax numerators into the G buffer, then one row kernel: logsumexp / loss,
    // and the numerators rescaled into the bf16 dScores in place
    float *part_m = reinterpret_cast<float*>(ws + wl.part_m), *part_s = reinterpret_cast<float*>(ws + wl.part_s), *gold = reinterpret_cast<float*>(ws + wl.gold);
    const int npart = kind == FWD_ONE_PASS_128 ? cdiv(Nc, 64) : cdiv(Nc, G2_B) * 4;
    GemmArgs a{Q, C, B, Nc, d, d, d, d};
    if (kind == FWD_ONE_PASS_128) {
      // on the 128 x 128 LDS-DMA tile (EpiSimP): the shapes whose 256-wide tiles cannot fill the chip
      EpiSimP epi;
      static_cast<EpiSim&>(epi) = with_packed_mask(cx.packed, EpiSim{nullptr, colmask, B, Nc, inv_T, part_m, part_s, y, y_offset, gold, nullptr, 0});
      epi.P = G;
      epi.npart = npart;
      if (int rc = launch<gemm128d_kernel<true, true, EpiSimP, false>>(dim3(cdiv(Nc, 128), cdiv(B, 128), 1), dim3(256), g1_lds_bytes, st, a, epi)) return rc;
    } else {
      // on the 256 x 256 tile of the no-logits forward (Epi8StatsP)
      Epi8StatsP epi;
      static_cast<Epi8Base&>(epi) = g8_base(cx.packed, Q, B, Nc, y, y_offset, colmask, inv_T, gold);
      epi.part_m = part_m;
      epi.part_s = part_s;
      epi.npart = npart;
      epi.P = G;
      if (opt(OPT_P16_STAGED) == 2 || (opt(OPT_P16_STAGED) == 1 && ((size_t)Nc * 2) % ((size_t)128 << 10) != 0)) {
        Epi8StatsPS es;
        static_cast<Epi8Stats&>(es) = static_cast<const Epi8Stats&>(epi);
        es.P = G;
        if (int rc = launch_g8<Epi8StatsPS, 2>(a, es, st)) return rc;
      } else if (int rc = launch_g8<Epi8StatsP, 2>(a, epi, st)) return rc;  // (two-phase schedule, as every storing epilogue; the four-phase instantiation spilled two registers)
    }
    if (int rc = launch_lse_p2g(part_m, part_s, npart, B, Nc, y, y_offset, grad_scale, row_lse, row_loss, G, ws, wl, st)) return rc;
    return launch_loss_sum(reinterpret_cast<const float*>(ws + wl.rloss), B, cx.loss_scale, loss_sum, st, cx.defer);
  }
  // no-logits forward: statistics pass -> logsumexp / loss -> dScores pass (logits recomputed), S is never in memory; elsewhere the
  // softmax launch reads the stored logits and writes G itself
  const bool recompute = kind == FWD_NO_LOGITS;
  if (int rc = sim_stats_body(cx.packed, Q, B, C, Nc, d, y, y_offset, colmask, inv_T, S_out, p, ws, st)) return rc;
  if (int rc = softmax_finish_body(cx, S_out, B, Nc, d, y, y_offset, grad_scale, row_loss, row_lse, loss_sum, recompute ? nullptr : G, p, ws, st))
    return rc;
  if (!recompute || G == nullptr) return DPRHOT_OK;
  return dscores_body(cx.packed, Q, B, C, Nc, d, y, y_offset, colmask, inv_T, grad_scale, reinterpret_cast<const float*>(ws + wl.lse), G, st);
}

int inbatch_fwd_f32_body(const StepCtx& cx, const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d, const int64_t* y,
                         int64_t y_offset, const uint8_t* colmask, float inv_T, float grad_scale, float* S_out, float* row_loss, float* row_lse,
                         float* loss_sum, dprhot_bf16* G, const StepPlan& p, char* ws, hipStream_t st) {
  if (S_out == nullptr && B > 128 && (p.nl || (G != nullptr && p.nl128))) {  // cast once, then the no-logits forward on the bf16 copies
    if (int rc = cast_operands(q, c, Qb, Cb, B, Nc, d, st)) return rc;
    return inbatch_fwd_body(cx, Qb, B, Cb, Nc, d, y, y_offset, colmask, inv_T, grad_scale, nullptr, row_loss, row_lse, loss_sum, G, p, ws, st);
  }
  if (int rc = sim_stats_f32_body(cx.packed, q, c, Qb, Cb, B, Nc, d, y, y_offset, colmask, inv_T, S_out, p, ws, st)) return rc;
  return softmax_finish_body(cx, S_out, B, Nc, d, y, y_offset, grad_scale, row_loss, row_lse, loss_sum, G, p, ws, st);
}

// The backward's plan: which launches form dC_part and dQ, and how many split-K slabs of dQ pass through the workspace (above one).
// both: dQ and dC_part are wanted; stamp: the packed step's dC epilogue stamps the loss, which the units of skinny.h cannot.
enum BwdKind { BWD_APART, BWD_FEW_ROWS, BWD_WIDE, BWD_PAIR128, BWD_PAIR256, BWD_PAIR };
struct BwdPlan { BwdKind kind; int slabs; DqPlan dq; Pair128Plan pp; };
BwdPlan bwd_plan(int B, int Nc, int d, const SkPlan& sk, bool both, bool stamp) {
  BwdPlan b{};
  b.dq = dq_plan(B, Nc, d);
  b.slabs = b.dq.splits;
  // (the long context axis under fewer than 512 rows: both GEMMs on the 128 x 128 engine -- see `long_axis` below; 256 x 65536 x 768:
  //  146 us against 174 with the dQ units on the 256 x 256 kernel and 252 for the pair)
  // (round 6, with the LDS-DMA 128 x 128 tile: also 512 <= B < 1024 from Nc >= 32 B on -- 512 x 16384 56 against 65 us with the dQ units on
  //  the 256 x 256 kernel and 73 for the pair, 512 x 32768 90 / 100 / 116: profiles/r06_bwd_plan_ab.txt)
  const bool long_axis_small = ((B < 512 && Nc >= 56 * 1024) || (B >= 512 && B < 1024 && (long)Nc >= 32L * B)) && !sk.ok &&
                               !wide_bwd_ok(B, Nc, d) && big_bwd_ok(B, Nc, d) && !pair128_use(B, Nc, d);
  b.kind = b.dq.big ? BWD_PAIR256 : BWD_PAIR;
  if (!both || force_tile() >= 0 || long_axis_small) b.kind = BWD_APART;  // dC and dQ in launches of their own
  else if (!stamp && sk.ok) b.kind = BWD_FEW_ROWS, b.slabs = sk.nslices;
  else if (!stamp && wide_bwd_ok(B, Nc, d)) b.kind = BWD_WIDE, b.slabs = 1;
  else if (pair128_use(B, Nc, d)) b.kind = BWD_PAIR128, b.pp = pair128_plan(B, Nc, d), b.slabs = b.pp.splits;
  return b;
}

int inbatch_bwd_body(const StepCtx& cx, const BwdPlan& bp, const dprhot_bf16* G, const dprhot_bf16* Q, const dprhot_bf16* C, int B, int Nc, int d,
                     float h_scale, const float* d_scale, float* dQ, float* dC_part, const StepPlan& sp, char* ws, hipStream_t st) {
  const WsLayout& wl = sp.wl;
  if (bp.kind == BWD_APART) {
    if (dC_part != nullptr)
      if (int rc = dc_body(cx.packed, G, Q, B, Nc, d, h_scale, d_scale, dC_part, st)) return rc;
    if (dQ != nullptr) return launch_dq(bp.dq, G, C, B, Nc, d, h_scale, d_scale, dQ, ws, wl, st, /*gemm_too=*/true, cx.defer);
    return DPRHOT_OK;
  }
  if (bp.kind == BWD_FEW_ROWS) {
    // Shapes of the few-rows plan: the same backward units as the one-call step (dC tiles and split-K dQ tiles side by side, then the
    // slab reduction) for callers that run sim / loss / backward as separate calls (a subclass's own loss on sim_score's logits):
    // 128 x 8192 x 768 23 -> ~15 us against the generic pair kernel.
    const SkPlan& sk = sp.sk;
    float* part = sk.nslices > 1 ? reinterpret_cast<float*>(ws + wl.dq_part) : nullptr;
    const int ndq = sk.nslices * (d / SK_QN), ndq_pad = (ndq + 7) & ~7, ndc = sk.nt * (d / SK_DN);
    SkBwdArgs b{G, Q, C, B, Nc, d, h_scale, d_scale, dC_part, nullptr, nullptr, 1.0f, 0, 0, 0, sk.ksteps, sk.nslices, part, dQ, ndq_pad,
                /*nt_store=*/1};
    if (int rc = launch_sk_bwd(b, ndq_pad + ndc, st)) return rc;
    if (sk.nslices > 1) return launch_sk_dq_reduce(part, sk.nslices, B, d, h_scale, d_scale, dQ, st);
    return DPRHOT_OK;
  }
  if (bp.kind == BWD_WIDE) {
    // Vocabulary-wide vectors under few rows (CITADEL router: 128 x 1024 x 30528): every unit of either GEMM is a short K loop in front
    // of a large store -- the unit shapes of skinny.h (whole operand footprint in flight by LDS-DMA, stores through LDS in whole
    // lines), dC tiles and dQ tiles side by side in one launch; the contexts fit one dQ slice, so no partial sums and no reduction.
    // The 141 MB of fp32 gradients leave with non-temporal stores: nobody re-reads them inside the step, and written normally they push
    // the step's operands out of the 256 MB Infinity Cache (measured: step 116 -> 99.5 us; the same policy on the
    // 8192^2 launches -- stored logits, 256 x 256 backward -- LOST 5-10 % and is not used there: profiles/r03_nt_stores_ab.txt).
    const int ksteps = cdiv(Nc, 64);
    const int ndq = d / SK_QN, ndq_pad = (ndq + 7) & ~7, ndc = cdiv(Nc, SK_COLS) * cdiv(d, SK_DN);
    SkBwdArgs b{G, Q, C, B, Nc, d, h_scale, d_scale, dC_part, nullptr, nullptr, 1.0f, 0, 0, 0, ksteps, 1, nullptr, dQ, ndq_pad, /*nt_store=*/1};
    return launch_sk_bwd(b, ndq_pad + ndc, st);
  }
  if (bp.kind == BWD_PAIR128) {
    // [dC tiles | dQ tiles x K slices] on the 128 x 128 LDS-DMA tile (round 6): the shapes under the 256 x 256 gate ran this pair on the
    // register-staged tiles (2048 x 4096 x 768: 69.5 us for 26 GFLOP)
    const Pair128Plan& pp = bp.pp;
    GemmArgs a1{G, Q, Nc, d, B, Nc, d, B};
    const EpiScaleF32 e1 = with_loss_stamp(cx.packed, EpiScaleF32{dC_part, Nc, d, h_scale, d_scale});
    GemmArgs a2{G, C, B, d, Nc, Nc, d, pp.kchunk};
    const EpiScaleF32 e2 = pp.splits == 1 ? EpiScaleF32{dQ, B, d, h_scale, d_scale}
                                          : EpiScaleF32{reinterpret_cast<float*>(ws + wl.dq_part), B, d, 1.0f, nullptr};
    const int nbx1 = cdiv(d, 128), nby1 = cdiv(Nc, 128), nbx2 = cdiv(d, 128), nby2 = cdiv(B, 128);
    const long grid = (long)nbx1 * nby1 + (long)nbx2 * nby2 * pp.splits;
    if (grid > 0x7fffffffL) return fail(DPRHOT_E_UNSUPPORTED, "grid too large");
    if (int rc = launch<gemm128d_pair_kernel<EpiScaleF32>>(dim3((unsigned)grid), dim3(256), g1_lds_bytes, st, a1, e1, nbx1, nby1, a2, e2, nbx2, nby2, pp.splits))
      return rc;
    if (pp.splits > 1) return launch_slab_sum(reinterpret_cast<const float*>(ws + wl.dq_part), pp.splits, B, d, h_scale, d_scale, dQ, st, cx.defer);
    return DPRHOT_OK;
  }
  const DqPlan& p = bp.dq;
  // one launch: [dC tiles | dQ tiles x splits]
  GemmArgs a1{G, Q, Nc, d, B, Nc, d, cdiv(B, 64) * 64};
  const EpiScaleF32 e1 = with_loss_stamp(cx.packed, EpiScaleF32{dC_part, Nc, d, h_scale, d_scale});
  GemmArgs a2{G, C, B, d, Nc, Nc, d, p.kchunk};
  EpiScaleF32 e2 = p.splits == 1 ? EpiScaleF32{dQ, B, d, h_scale, d_scale}
                                 : EpiScaleF32{reinterpret_cast<float*>(ws + wl.dq_part), B, d, 1.0f, nullptr};
  if (bp.kind == BWD_PAIR256) {
    // Few query rows against a long context axis (512 <= B <= 2048, Nc >= 32 B: e.g. 8192 global queries x 8 contexts seen from one
    // of 8 ranks): the dC tiles of the pair launch are only K = B deep -- 8 to 32 K steps between a pipeline fill and a 256 KiB store
    // -- next to dQ units several times as long (the K slices of dQ stop at 16), and the launch loses to dC on the 128 x 128 engine in a
    // launch of its own (dc_body) followed by this launch with its dQ units only.  Measured, pair / dC apart, us (d = 768,
    // profiles/r05_bwd_long_axis.txt): 1024 x 32768 181 / 154, 1024 x 49152 292 / 236, 1024 x 65536 482 / 299,
    // 512 x 16384 73 / 70, 512 x 32768 117 / 112, 512 x 65536 356 / 202, 2048 x 65536 611 / 555, 1024 x 32768 x 1024 217 / 197; the
    // pair stays where it wins: 1024 x 8192 43 / 71, 1024 x 16384 82 / 96, 2048 x 16384 122 / 146, 2048 x 32768 228 / 289, 512 x 8192 33 / 50.
    const bool long_axis = B >= 512 && B <= 2048 && (long)Nc >= 32L * B;
    // (round 6: B and Nc multiples of 64 suffice -- a unit with an odd number of K steps skips the MFMAs of its last half pair; the packed
    //  multi-rank layout's column counts are multiples of 64, rarely of 128)
    const bool ok8 = B % 64 == 0 && Nc % 64 == 0 && p.kchunk % 128 == 0 && (double)B * Nc < 2.0e9 && (double)Nc * d < 2.0e9;
    a1.kchunk = B;  // dC: one K range (B % 64 == 0)
    // the same epilogues for the phase-interleaved kernel (gemm8pb.h)
    const Epi8Scale s1{e1.out, e1.M, e1.N, e1.h_scale, e1.d_scale, e1.stamp_src, e1.stamp_period, e1.stamp_row};
    const Epi8Scale s2{e2.out, e2.M, e2.N, e2.h_scale, e2.d_scale, e2.stamp_src, e2.stamp_period, e2.stamp_row};
    if (long_axis && ok8 && ((size_t)Nc * 2) % ((size_t)128 << 10) == 0) {
      // (round 6) the dC tiles ALONE on the phase-interleaved kernel, in a launch of their own in front of the launch with the dQ units: no
      // dQ units four times as long next to them.  Only where the row pitch of G is a multiple of 128 KiB (Nc = 65536): the 128-wide tiles'
      // 256-byte pieces then alias in the memory system -- 180 us where 126 are expected -- and the 512-byte pieces of the 256-wide tile do
      // not: backward 325 -> 275 us at 1024 x 65536, 557 -> 470 at 2048 x 65536; it LOSES at 32768 / 49152 columns
      // (profiles/r06_dc_alone_ab.txt)
      const int nbx1a = cdiv(d, G2_B), nby1a = cdiv(Nc, G2_B);
      if (int rc = launch<gemm8p_bwd_kernel<Epi8Scale>>(dim3((unsigned)(nbx1a * nby1a)), dim3(G2_THREADS), g8_lds_total, st, a1, s1, nbx1a, nby1a, a2, s2,
                                                        cdiv(d, G2_B), 0, p.splits))
        return rc;
    } else if (long_axis) {
      if (int rc = dc_body(cx.packed, G, Q, B, Nc, d, h_scale, d_scale, dC_part, st)) return rc;
    }
    const int nbx1 = cdiv(d, G2_B), nby1 = long_axis ? 0 : cdiv(Nc, G2_B), nbx2 = cdiv(d, G2_B), nby2 = cdiv(B, G2_B);
    const int grid = nbx1 * nby1 + nbx2 * nby2 * p.splits;
    // ok8: the phase-interleaved schedule (gemm8pb.h): an even number of K steps per unit, byte offsets in 32 bits
    const int rc = ok8 ? launch<gemm8p_bwd_kernel<Epi8Scale>>(dim3((unsigned)grid), dim3(G2_THREADS), g8_lds_total, st, a1, s1, nbx1, nby1, a2, s2, nbx2, nby2, p.splits)
                       : launch<gemm256_bwd_kernel<EpiScaleF32>>(dim3((unsigned)grid), dim3(G2_THREADS), g2_lds_total, st, a1, e1, nbx1, nby1, a2, e2, nbx2, nby2, p.splits);
    if (rc) return rc;
    return launch_dq(p, G, C, B, Nc, d, h_scale, d_scale, dQ, ws, wl, st, /*gemm_too=*/false, cx.defer);
  }
  const int t1 = dc_tile(B, Nc, d);
  const int rc = use_tr() ? launch_pair_tr<true>(t1, p.tile, a1, e1, a2, e2, p.splits, st)
                          : launch_pair_tr<false>(t1, p.tile, a1, e1, a2, e2, p.splits, st);
  if (rc) return rc;
  return launch_dq(p, G, C, B, Nc, d, h_scale, d_scale, dQ, ws, wl, st, /*gemm_too=*/false, cx.defer);
}

// the second launch of the latency-bound step (step_small.h)
int launch_step_small(const StepCtx& cx, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d, const int64_t* y, int64_t y_offset, float grad_scale,
                      float h_scale, const float* d_scale, float* S_out, float* row_loss, float* row_lse, float* loss_sum, dprhot_bf16* G, float* dQ,
                      float* dC_part, const StepPlan& p, char* ws, hipStream_t st) {
  const FwdPlan& fp = p.fp;
  const PackedSpec& pk = cx.packed;
  StepSmallArgs a{reinterpret_cast<const float*>(ws + p.wl.logits), fp.splits, (size_t)B * Nc, B, Nc, d, y, y_offset, grad_scale,
                  Qb, Cb, h_scale, d_scale, dQ, dC_part, S_out, row_loss, row_lse, loss_sum, G,
                  pk.stamp_src != nullptr ? pk.rows_c : 0, pk.n_ctx, cx.loss_scale};
  // 16 columns of d per workgroup: every workgroup repeats the softmax, the narrow tile only shortens the GEMM / store tail
  constexpr int tw = 16;
  const size_t lds = step_small_lds(Nc, tw);
  const int ncp = (Nc + 31) / 32 * 32;
  const dim3 grid(d / tw), block(1024);
  if (lds > 160 * 1024) return fail(DPRHOT_E_UNSUPPORTED, "small step: Nc=%d needs %zu bytes of LDS", Nc, lds);
  // (the LDS of all these kernels grows with Nc: launch() raises the limit again when a larger shape follows a smaller one)
  // DPRHOT_BY_SLABS instantiates NS == max(fp.splits, 1): the role-split kernels read exactly NS slabs and add them all, with no
  // run-time look at the slab count (step_small.h: ss_load_slabs), so a plan outside 0 .. 4 must never reach the macro
  if (fp.splits < 0 || fp.splits > 4)
    return fail(DPRHOT_E_UNSUPPORTED, "small step: the plan has %d slabs, the launch reads max(splits, 1) <= 4", fp.splits);
#define DPRHOT_BY_SLABS(LAUNCH, CPT) \
  (fp.splits <= 1 ? LAUNCH(CPT, 1) : fp.splits == 2 ? LAUNCH(CPT, 2) : fp.splits == 3 ? LAUNCH(CPT, 3) : LAUNCH(CPT, 4))
  // the role-split forms (step_small_kernel_roles, step_small_kernel_out): one row block, the multi-slab plans up to 768 columns
  if (const int roles = opt(OPT_SMALL_STEP_ROLES); roles != 0 && B <= SS_ROWS && ncp <= 768) {
    const int qtw = roles >= 2 && d % 32 == 0 ? 32 : 16;
    // Form 3 hands the lead's outputs to workgroups of their own (a loss block and two row-store blocks in front of the grid).  A stamping launch (the packed step) keeps form
    // 2: the loss goes into dC[m][0], whose owner -- the dC workgroup of column 0 -- needs the finished sum, so there the lead stays.
    const bool outwg = roles == 3 && pk.stamp_src == nullptr;
    const size_t rlds = step_roles_lds(Nc, qtw);  // (the maximum over the roles, the output role included)
    const dim3 rgrid(d / 16 + 2 * (d / qtw) + (outwg ? SS_OUT_BLOCKS : 0));
#define DPRHOT_SR_LAUNCH_K(KERN, CPT, NS, QTW) launch<KERN<CPT, NS, QTW>>(rgrid, block, rlds, st, a)
#define DPRHOT_SR_LAUNCH_Q(CPT, NS, QTW) \
  (outwg ? DPRHOT_SR_LAUNCH_K(step_small_kernel_out, CPT, NS, QTW) : DPRHOT_SR_LAUNCH_K(step_small_kernel_roles, CPT, NS, QTW))
#define DPRHOT_SR_LAUNCH(CPT, NS) (qtw == 16 ? DPRHOT_SR_LAUNCH_Q(CPT, NS, 16) : DPRHOT_SR_LAUNCH_Q(CPT, NS, 32))
    if (ncp <= 256) return DPRHOT_BY_SLABS(DPRHOT_SR_LAUNCH, 1);
    if (ncp <= 512) return DPRHOT_BY_SLABS(DPRHOT_SR_LAUNCH, 2);
    return DPRHOT_BY_SLABS(DPRHOT_SR_LAUNCH, 3);
#undef DPRHOT_SR_LAUNCH
#undef DPRHOT_SR_LAUNCH_Q
#undef DPRHOT_SR_LAUNCH_K
  }
#define DPRHOT_SS_LAUNCH_N(CPT, NS, NRB) launch<step_small_kernel<CPT, tw, NS, NRB>>(grid, block, lds, st, a)
#define DPRHOT_SS_LAUNCH(CPT, NS) (B <= SS_ROWS ? DPRHOT_SS_LAUNCH_N(CPT, NS, 1) : DPRHOT_SS_LAUNCH_N(CPT, NS, 2))
  if (ncp <= 256) return DPRHOT_BY_SLABS(DPRHOT_SS_LAUNCH, 1);
  if (ncp <= 512) return DPRHOT_BY_SLABS(DPRHOT_SS_LAUNCH, 2);
  if (ncp <= 768) return DPRHOT_BY_SLABS(DPRHOT_SS_LAUNCH, 3);
  return DPRHOT_SS_LAUNCH_N(5, 1, 1);  // (B <= 32 only: small_step_ok; above 768 columns the sim launch writes one slab: fwd_plan)
#undef DPRHOT_SS_LAUNCH
#undef DPRHOT_SS_LAUNCH_N
#undef DPRHOT_BY_SLABS
}

// A whole training step (forward AND backward).  At the latency-bound shapes (step_small.h) it is TWO launches: the sim GEMM
// (partial-logit slabs) and one kernel that does softmax-CE, dScores and both backward GEMMs; few rows against many contexts run the
// launches of skinny.h; every other shape runs the launches of inbatch_fwd_f32_body + inbatch_bwd_body.
int inbatch_step_body(const StepCtx& cx, const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d, const int64_t* y,
                      int64_t y_offset, const uint8_t* colmask, float inv_T, float grad_scale, float h_scale, const float* d_scale, float* S_out,
                      float* row_loss, float* row_lse, float* loss_sum, dprhot_bf16* G, float* dQ, float* dC_part, const StepPlan& p, char* ws,
                      hipStream_t st) {
  if (p.family == FAM_FEW_ROWS) {
    if (c != nullptr)  // single rank: the contexts arrive as fp32 -- one cast, then they are the bf16 matrix of every launch
      if (int rc = dprhot_cast_bf16(c, Cb, (size_t)Nc * d, st)) return rc;
    return sk_step(cx, q, Cb, Qb, B, Nc, d, y, y_offset, colmask, inv_T, grad_scale, h_scale, d_scale, S_out, row_loss, row_lse, loss_sum, G, dQ,
                   dC_part, ws, p.wl, p.sk, st);
  }
  if (p.family == FAM_SMALL_STEP) {
    if (int rc = sim_stats_f32_body(cx.packed, q, c, Qb, Cb, B, Nc, d, y, y_offset, colmask, inv_T, nullptr, p, ws, st)) return rc;
    return launch_step_small(cx, Qb, Cb, B, Nc, d, y, y_offset, grad_scale, h_scale, d_scale, S_out, row_loss, row_lse, loss_sum, G, dQ, dC_part, p,
                             ws, st);
  }
  // the sum of the row losses may ride in the launch that combines the dQ slabs (LossDefer)
  // (single rank only: the packed step's backward stamps the finished loss into dC_part, so it must exist before that launch)
  LossDefer ld;
  ld.armed = cx.packed.stamp_src == nullptr && opt(OPT_LOSS_WITH_DQ) != 0;
  StepCtx dx = cx;
  dx.defer = &ld;
  int rc = inbatch_fwd_f32_body(dx, q, c, Qb, Cb, B, Nc, d, y, y_offset, colmask, inv_T, grad_scale, S_out, row_loss, row_lse, loss_sum, G, p, ws, st);
  ld.armed = false;
  if (rc == DPRHOT_OK)
    rc = inbatch_bwd_body(dx, bwd_plan(B, Nc, d, p.sk, true, cx.packed.stamp_src != nullptr), G, Qb, Cb, B, Nc, d, h_scale, d_scale, dQ, dC_part, p, ws, st);
  if (ld.pending) {  // a backward without a slab-combining launch (or one that failed): the loss launch after all
    const int rc2 = launch_loss_sum(ld.src, ld.n, ld.scale, ld.out, st, nullptr);
    if (rc == DPRHOT_OK) rc = rc2;
  }
  return rc;
}

// ---- the training step: argument checks; an outer entry point runs the checks of the ones it is made of ----
int check_sim_stats(const dprhot_bf16* Q, const dprhot_bf16* C, const int64_t* y, const float* S_out, int B, int Nc, int d) {
  REQUIRE(Q && C && y, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  REQUIRE(aligned16(Q) && aligned16(C) && aligned16(S_out), "pointers must be 16-byte aligned");
  return DPRHOT_OK;
}
int check_sim_stats_f32(const float* q, const float* c, const dprhot_bf16* Qb, const dprhot_bf16* Cb, const int64_t* y, const float* S_out, int B,
                        int Nc, int d) {
  REQUIRE(q && Qb && Cb && y, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  REQUIRE(aligned16(q) && aligned16(Qb) && aligned16(Cb) && aligned16(c) && aligned16(S_out), "pointers must be 16-byte aligned");
  return DPRHOT_OK;
}
int check_softmax_finish(const float* S_in, const int64_t* y, const float* loss_sum, const dprhot_bf16* G, int B, int Nc, int d) {
  REQUIRE(y && loss_sum, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  REQUIRE(aligned16(G) && aligned16(S_in), "pointers must be 16-byte aligned");
  return DPRHOT_OK;
}

// What dprhot_train_step_* asks of the shape's plan, before anything else is looked at (a plain step asks for neither): dC_part as bf16
// only from the few-rows step, whose dC units have such an epilogue; dQ slabs only where the step leaves some.
int step_admit(int dc_kind, const float* dq_part, int B, int Nc, int d, StepPlan* p) {
  if (int rc = check_shape(B, Nc, d)) return rc;
  *p = step_plan(B, Nc, d);
  if (dc_kind != GC_FP32 && !(dc_kind == GC_BF16 && p->family == FAM_FEW_ROWS))
    return fail(DPRHOT_E_UNSUPPORTED, "train_step: dc_kind=%d at B=%d Nc=%d d=%d: this shape's plan writes fp32 dC_part only (ask for dc_kind = 2)", dc_kind,
                B, Nc, d);
  if (dq_part == nullptr) return DPRHOT_OK;
  REQUIRE(aligned16(dq_part), "dq_part must be 16-byte aligned");
  if (p->dq_slabs() == 0)
    return fail(DPRHOT_E_INVALID, "train_step: dq_part given but B=%d Nc=%d d=%d leaves no slabs (dprhot_train_dq_slabs = 0)", B, Nc, d);
  return DPRHOT_OK;
}

// the packed layout of a multi-rank step: the gathered buffer carries the column mask, the loss numerator rides in dC_part
int packed_spec(const float* q, const dprhot_bf16* gathered, const dprhot_bf16* Qb, const int64_t* y, const float* loss_sum, int W, int rank, int n_ctx,
                int d, PackedSpec* ps, int* rows_c) {
  REQUIRE(q && gathered && Qb && y && loss_sum, "NULL pointer");
  REQUIRE(W > 0 && rank >= 0 && rank < W && n_ctx > 0 && d > 0 && d % 8 == 0, "bad argument W=%d rank=%d n_ctx=%d d=%d", W, rank, n_ctx, d);
  if (int rc = dprhot_packed_rows(n_ctx, d, rows_c)) return rc;
  ps->base = reinterpret_cast<const uint8_t*>(gathered);
  ps->rows_c = *rows_c;
  ps->n_ctx = n_ctx;
  ps->row_bytes = d * 2;
  ps->stamp_src = loss_sum;
  return DPRHOT_OK;
}

// every public form of the one-call step ends here, its shape admitted and planned (step_admit)
int run_step(const StepCtx& cx, const StepPlan& p, const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d,
             const int64_t* y, int64_t y_offset, const uint8_t* colmask, float inv_T, float grad_scale, float h_scale, const float* d_scale, float* S_out,
             float* row_loss, float* row_lse, float* loss_sum, dprhot_bf16* G, float* dQ, float* dC_part, void* workspace, size_t workspace_bytes,
             hipStream_t st) {
  REQUIRE(loss_sum && dQ && dC_part, "NULL pointer (loss_sum, dQ and dC_part are required)");
  REQUIRE(aligned16(G) && aligned16(dQ) && aligned16(dC_part), "pointers must be 16-byte aligned");
  REQUIRE(G != nullptr || p.fz.ok, "G == NULL at B=%d Nc=%d d=%d: this shape's plan materialises the dScores (dprhot_step_wants_g = 1)", B, Nc, d);
  if (int rc = check_sim_stats_f32(q, c, Qb, Cb, y, S_out, B, Nc, d)) return rc;
  char* ws;
  if (int rc = claim_ws("inbatch_step", p.wl, workspace, workspace_bytes, true, true, &ws)) return rc;
  return inbatch_step_body(cx, q, c, Qb, Cb, B, Nc, d, y, y_offset, colmask, inv_T, grad_scale, h_scale, d_scale, S_out, row_loss, row_lse, loss_sum, G,
                           dQ, dC_part, p, ws, st);
}

}  // namespace

// ---- late-interaction expert scoring (maxsim.h) ---------------------------------------------------------------------------
// Workspace: val [Ny, RK] f32 | arg [Ny, RK] i32 | raw [Ny, RK] f32 (weights only) | parg [Nq, Ny] i32, each 256-byte aligned.
static size_t ms_align(size_t b) { return (b + 255) & ~(size_t)255; }
static int ms_ws_layout(int Nq, int LQ, int KQ, int Ny, int has_w, size_t off[4], size_t* total) {
  REQUIRE(Nq > 0 && LQ > 0 && Ny > 0, "bad shape Nq=%d LQ=%d Ny=%d", Nq, LQ, Ny);
  REQUIRE(KQ >= 1 && KQ <= MS_KMAX, "KQ=%d: 1 <= KQ <= %d", KQ, MS_KMAX);
  const size_t tab = (size_t)Ny * Nq * LQ * KQ * 4;
  off[0] = 0;
  off[1] = ms_align(tab);
  off[2] = off[1] + ms_align(tab);
  off[3] = off[2] + (has_w ? ms_align(tab) : 0);
  *total = off[3] + ms_align((size_t)Nq * Ny * 4);
  return DPRHOT_OK;
}

static int ms_setup(MsArgs& p, const void* q_tok, const void* c_tok, int Nq, int LQ, int Nc, int LD, int dp, const int* q_ids,
                    const int* c_ids, const float* q_w, const float* c_w, int KQ, int KD, int pool, int M, const uint8_t* mask,
                    const void* ws, size_t ws_bytes) {
  REQUIRE(q_tok && c_tok && ws, "NULL pointer (q_tok, c_tok and the workspace are required)");
  REQUIRE(Nq > 0 && Nc > 0 && LQ > 0 && LD > 0, "bad shape Nq=%d LQ=%d Nc=%d LD=%d", Nq, LQ, Nc, LD);
  REQUIRE(LQ <= DPRHOT_MAXSIM_MAX_LEN && LD <= DPRHOT_MAXSIM_MAX_LEN, "LQ=%d LD=%d: token counts are limited to %d", LQ, LD,
          DPRHOT_MAXSIM_MAX_LEN);
  REQUIRE(dp >= 32 && dp % 32 == 0, "dp=%d must be a positive multiple of 32 (zero-pad the features)", dp);
  REQUIRE(KQ >= 1 && KQ <= MS_KMAX && KD >= 1 && KD <= MS_KMAX, "KQ=%d KD=%d: expert slots per token are limited to 1..%d", KQ, KD,
          MS_KMAX);
  REQUIRE((q_ids == nullptr) == (c_ids == nullptr), "expert ids are required on both sides or on neither");
  REQUIRE((q_w == nullptr) == (c_w == nullptr), "expert weights are required on both sides or on neither");
  REQUIRE(q_ids || (KQ == 1 && KD == 1), "KQ=%d KD=%d without expert ids (ColBERT has one slot per token)", KQ, KD);
  REQUIRE(pool == DPRHOT_POOL_SUM || pool == DPRHOT_POOL_MAX, "pool=%d (0 sum, 1 max)", pool);
  REQUIRE(M >= 0, "M=%d", M);
  REQUIRE(M == 0 || (long)Nq * M == (long)Nc, "pairwise: Nc=%d must equal Nq * M = %d * %d", Nc, Nq, M);
  REQUIRE(((uintptr_t)q_tok & 15) == 0 && ((uintptr_t)c_tok & 15) == 0, "token rows must be 16-byte aligned");
  REQUIRE((long)Nq * LQ * KQ <= 0x7fffffffL && (long)Nc * LD * KD <= 0x7fffffffL, "too many token slots");
  const int Ny = M > 0 ? M : Nc;
  const long ntiles = M > 0 ? (long)Nq * ((LQ + MS_BM - 1) / MS_BM) : ((long)Nq * LQ + MS_BM - 1) / MS_BM;
  REQUIRE(ntiles * Ny <= 0x7fffffffL && (long)Nq * Ny <= 0x7fffffffL, "grid too large (Nq=%d Nc=%d)", Nq, Nc);
  size_t off[4], total = 0;
  const int rc = ms_ws_layout(Nq, LQ, KQ, Ny, q_w != nullptr, off, &total);
  if (rc) return rc;
  REQUIRE(ws_bytes >= total, "workspace of %zu bytes, %zu needed (dprhot_maxsim_workspace_bytes)", ws_bytes, total);
  char* w = (char*)ws;
  p = MsArgs{(const uint16_t*)q_tok, (const uint16_t*)c_tok, q_ids, c_ids, q_w, c_w, mask, Nq, LQ, Nc, LD, dp, KQ, KD, M, Ny, pool,
             (float*)(w + off[0]), (int*)(w + off[1]), q_w ? (float*)(w + off[2]) : nullptr, (int*)(w + off[3]), nullptr};
  return DPRHOT_OK;
}

template <int KQT>
static int ms_launch_fwd(const MsArgs& p, unsigned blocks, hipStream_t st) {
  if (p.qid && p.qw) return launch<ms_fwd_kernel<KQT, true, true>>(dim3(blocks), dim3(256), 0, st, p);
  if (p.qid) return launch<ms_fwd_kernel<KQT, true, false>>(dim3(blocks), dim3(256), 0, st, p);
  if (p.qw) return launch<ms_fwd_kernel<KQT, false, true>>(dim3(blocks), dim3(256), 0, st, p);
  return launch<ms_fwd_kernel<KQT, false, false>>(dim3(blocks), dim3(256), 0, st, p);
}

static_assert(MS_SC_SLOTS == DPRHOT_MAXSIM_MAX_LEN * MS_KMAX, "ms_score_kernel's LDS table holds every row slot of one query");

template <int KQT>
static int ms_launch_score(const MsArgs& p, hipStream_t st) {
  const dim3 grid((unsigned)p.Nc), block(256);
  if (p.qid && p.qw) return launch<ms_score_kernel<KQT, true, true>>(grid, block, 0, st, p);
  if (p.qid) return launch<ms_score_kernel<KQT, true, false>>(grid, block, 0, st, p);
  if (p.qw) return launch<ms_score_kernel<KQT, false, true>>(grid, block, 0, st, p);
  return launch<ms_score_kernel<KQT, false, false>>(grid, block, 0, st, p);
}

template <bool IDS, bool W>
static int ms_launch_bwd(const MsArgs& p, const MsBwd& g, hipStream_t st) {
  const int R = p.Nq * p.LQ;
  if (g.dq || g.dwq) {
    const dim3 grid((unsigned)((R + 3) / 4), (unsigned)(g.dq ? (p.dp + MS_DQ_CHUNK - 1) / MS_DQ_CHUNK : 1));
    if (int rc = launch<ms_dq_kernel<IDS, W>>(grid, dim3(256), 0, st, p, g)) return rc;
  }
  if (g.dc || g.dwc) {
    const size_t lds = ((size_t)p.LD * MS_DC_SLICE + (size_t)p.LD * p.KD) * 4;  // (grows with LD and KD: the helper raises the limit as it does)
    const dim3 grid((unsigned)p.Nc, (unsigned)(g.dc ? (p.dp + MS_DC_SLICE - 1) / MS_DC_SLICE : 1));
    return launch<ms_dc_kernel<IDS, W>>(grid, dim3(256), lds, st, p, g);
  }
  return DPRHOT_OK;
}

// ---- CITADEL / SPLADE router head (csrc/router_head.h) ----
// Workspace: the rows' logsumexp [B, T] fp32 (only with want_softmax).
static int rh_check_shape(int B, int T1, int V, int skip, int k) {
  REQUIRE(B > 0 && B <= 65535, "B=%d: 1 <= B <= 65535", B);
  REQUIRE(k >= 0 && k <= RH_KMAX, "k=%d: 0 <= k <= %d", k, RH_KMAX);
  REQUIRE(V >= (k > 1 ? k : 1), "V=%d: the vocabulary must hold at least max(k, 1) = %d columns", V, k > 1 ? k : 1);
  REQUIRE(skip >= 0 && T1 >= 1 && skip <= T1 - 1, "T1=%d skip=%d: at least one token row must remain (T >= 1)", T1, skip);
  REQUIRE((long long)B * T1 <= 0x7fffffffLL && (long long)(T1 - skip) * (k > 0 ? k : 1) <= 0x7fffffffLL, "too many token rows (B=%d T1=%d)", B, T1);
  return DPRHOT_OK;
}
static int rh_check_dtype(int dtype) {
  REQUIRE(dtype == RH_BF16 || dtype == RH_FP16 || dtype == RH_FP32, "dtype=%d (0 bf16, 1 fp16, 2 fp32)", dtype);
  return DPRHOT_OK;
}
static int rh_npt(int V) { return V <= RH_THREADS ? 1 : V <= 4 * RH_THREADS ? 4 : V <= 32 * RH_THREADS ? 32 : 0; }

template <int DT>
static int rh_launch_row(const RhArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((long long)a.B * a.T)), block(RH_THREADS);
  switch (rh_npt(a.V)) {
    case 1: return launch<rh_row_kernel<DT, 1>>(grid, block, 0, st, a);
    case 4: return launch<rh_row_kernel<DT, 4>>(grid, block, 0, st, a);
    case 32: return launch<rh_row_kernel<DT, 32>>(grid, block, 0, st, a);
    default: return launch<rh_row_kernel<DT, 0>>(grid, block, 0, st, a);
  }
}
template <int DT>
static int rh_launch_fwd(const RhArgs& a, hipStream_t st) {
  if (a.k > 0 || a.want_soft)
    if (int rc = rh_launch_row<DT>(a, st)) return rc;
  return launch<rh_col_kernel<DT>>(dim3((unsigned)((a.V + RH_COLS - 1) / RH_COLS), (unsigned)a.B), dim3(RH_COLS), 0, st, a);
}
template <int DT>
static int rh_launch_bwd(const RhArgs& a, hipStream_t st) {
  if (!a.g_soft) {
    const dim3 grid((unsigned)((a.V + RH_COLS - 1) / RH_COLS), (unsigned)((a.T1 + RH_BWD_ROWS - 1) / RH_BWD_ROWS), (unsigned)a.B);
    return launch<rh_bwd_sparse_kernel<DT>>(grid, dim3(RH_COLS), 0, st, a);
  }
  const dim3 grid((unsigned)((long long)a.B * a.T1)), block(RH_THREADS);
  switch (rh_npt(a.V)) {
    case 1: return launch<rh_bwd_row_kernel<DT, 1>>(grid, block, 0, st, a);
    case 4: return launch<rh_bwd_row_kernel<DT, 4>>(grid, block, 0, st, a);
    default: return launch<rh_bwd_row_kernel<DT, 0>>(grid, block, 0, st, a);
  }
}

extern "C" {

int dprhot_version(void) { return DPRHOT_VERSION; }
const char* dprhot_last_error(void) { return g_err; }

int dprhot_set_option(const char* name, int value) {
  REQUIRE(name != nullptr, "NULL name");
  for (int i = 0; i < OPT_COUNT; ++i)
    if (strcmp(name, kOptDefs[i].name) == 0) {
      __atomic_store_n(&g_opt[i], value, __ATOMIC_RELAXED);
      __atomic_add_fetch(&g_opt_epoch, 1, __ATOMIC_RELAXED);
      return DPRHOT_OK;
    }
  return fail(DPRHOT_E_INVALID, "unknown option '%s'", name);
}

long long dprhot_options_epoch(void) { return __atomic_load_n(&g_opt_epoch, __ATOMIC_RELAXED); }

int dprhot_get_option(const char* name, int* h_value) {
  REQUIRE(name != nullptr && h_value != nullptr, "NULL pointer");
  for (int i = 0; i < OPT_COUNT; ++i)
    if (strcmp(name, kOptDefs[i].name) == 0) {
      *h_value = opt((OptId)i);
      return DPRHOT_OK;
    }
  return fail(DPRHOT_E_INVALID, "unknown option '%s'", name);
}

int dprhot_workspace_bytes(int B, int Nc, int d, size_t* h_out) {
  REQUIRE(h_out != nullptr, "h_out is NULL");
  if (int rc = check_shape(B, Nc, d)) return rc;
  *h_out = step_plan(B, Nc, d).wl.total;
  return DPRHOT_OK;
}

int dprhot_cast_bf16(const float* src, dprhot_bf16* dst, size_t n, void* stream) {
  REQUIRE(src && dst, "NULL pointer");
  REQUIRE(n % 8 == 0, "n=%zu must be a multiple of 8", n);
  REQUIRE(aligned16(src) && aligned16(dst), "pointers must be 16-byte aligned");
  if (n == 0) return DPRHOT_OK;
  const size_t n4 = n / 4, tiles = (n4 + 256 * CAST_UT - 1) / (256 * CAST_UT);
  REQUIRE(tiles < (1ull << 31), "n=%zu", n);
  return launch<cast_bf16_kernel>(dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, src, dst, n4);
}

int dprhot_prep(const float* q, size_t nq, dprhot_bf16* Qb, const float* c, size_t nc, dprhot_bf16* Cdst, void* stream) {
  REQUIRE(q && Qb && c && Cdst, "NULL pointer");
  REQUIRE(nq % 8 == 0 && nc % 8 == 0, "element counts must be multiples of 8 (nq=%zu nc=%zu)", nq, nc);
  REQUIRE(aligned16(q) && aligned16(Qb) && aligned16(c) && aligned16(Cdst), "pointers must be 16-byte aligned");
  const size_t n8 = (nq + nc) / 8;
  if (n8 == 0) return DPRHOT_OK;
  const int blocks = (int)((n8 + 255) / 256 > 2048 ? 2048 : (n8 + 255) / 256);
  return launch<cast2_bf16_kernel>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, q, Qb, nq / 8, c, Cdst, nc / 8);
}

int dprhot_packed_rows(int n_ctx, int d, int* h_rows) {
  REQUIRE(h_rows != nullptr && n_ctx > 0 && d > 0 && d % 8 == 0, "bad argument");
  const int extra = cdiv(n_ctx, 2 * d);           // rows needed for n_ctx mask bytes
  // gathered column count stays a multiple of 8 -- and, from 2048 contexts per rank on (round 6), of 64: the 256 x 256 backward wants
  // whole 64-deep K steps over the gathered axis, and W x 8200 columns (8192 contexts + 8 header rows) sent a large-batch multi-rank
  // step to the 128 x 128 pair kernel; the (at most 56) extra rows are masked columns like every header row
  const int align = n_ctx >= 2048 ? 64 : 8;
  *h_rows = cdiv(n_ctx + extra, align) * align;
  return DPRHOT_OK;
}

int dprhot_pack_ctx(const float* c, const uint8_t* mask, int n_ctx, int d, dprhot_bf16* send, void* stream) {
  REQUIRE(c && send, "NULL pointer");
  REQUIRE(n_ctx > 0 && d > 0 && d % 8 == 0, "bad shape n_ctx=%d d=%d", n_ctx, d);
  REQUIRE(aligned16(c) && aligned16(send), "pointers must be 16-byte aligned");
  int rows_c = 0;
  dprhot_packed_rows(n_ctx, d, &rows_c);
  const size_t n8 = (size_t)rows_c * d / 8;
  const int blocks = (int)((n8 + 255) / 256 > 2048 ? 2048 : (n8 + 255) / 256);
  return launch<pack_ctx_kernel>(dim3(blocks), dim3(256), 0, (hipStream_t)stream, c, mask, n_ctx, d, rows_c, send);
}

int dprhot_unpack_mask(const dprhot_bf16* gathered, int W, int n_ctx, int d, uint8_t* colmask, void* stream) {
  REQUIRE(gathered && colmask, "NULL pointer");
  REQUIRE(W > 0 && n_ctx > 0 && d > 0 && d % 8 == 0, "bad shape W=%d n_ctx=%d d=%d", W, n_ctx, d);
  int rows_c = 0;
  dprhot_packed_rows(n_ctx, d, &rows_c);
  const int total = W * rows_c;
  return launch<unpack_mask_kernel>(dim3(cdiv(total, 256) > 1024 ? 1024 : cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, gathered, W, n_ctx,
                                    d, rows_c, colmask);
}

int dprhot_sim_fwd(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const uint8_t* colmask, float inv_T,
                   float* S, void* stream) {
  REQUIRE(Q && C && S, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  REQUIRE(aligned16(Q) && aligned16(C) && aligned16(S), "pointers must be 16-byte aligned");
  return sim_fwd_body(PackedSpec{}, Q, B, C, Nc, d, colmask, inv_T, S, (hipStream_t)stream);
}

int dprhot_softmax_ce_fwd_bwd(const float* S, int B, int Nc, const int64_t* y, int64_t y_offset, float grad_scale,
                              const int64_t* row_win_start, int win_len, float* row_loss, float* row_lse, dprhot_bf16* G,
                              void* stream) {
  REQUIRE(S && y, "NULL pointer");
  REQUIRE(B > 0 && Nc > 0 && Nc % 8 == 0, "bad shape B=%d Nc=%d (Nc %% 8 == 0)", B, Nc);
  REQUIRE(aligned16(S) && (G == nullptr || aligned16(G)), "pointers must be 16-byte aligned");
  REQUIRE(row_win_start == nullptr || win_len > 0, "win_len must be > 0 with row_win_start");
  SoftmaxArgs p{S, B, Nc, y, y_offset, grad_scale, row_win_start, win_len, row_loss, row_lse, G};
  if (Nc <= 4096) return launch<softmax_ce_kernel<64>>(dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, p);
  return launch<softmax_ce_kernel<256>>(dim3(B), dim3(256), 0, (hipStream_t)stream, p);
}

int dprhot_reduce_sum(const float* x, int n, float scale, float* out, void* stream) {
  REQUIRE(x && out && n > 0, "bad argument");
  return launch<reduce_sum_kernel>(dim3(1), dim3(256), 0, (hipStream_t)stream, x, n, scale, out);
}

int dprhot_dq(const dprhot_bf16* G, const dprhot_bf16* C, int B, int Nc, int d, float h_scale, const float* d_scale, float* dQ,
              void* workspace, size_t workspace_bytes, void* stream) {
  REQUIRE(G && C && dQ, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  REQUIRE(aligned16(G) && aligned16(C) && aligned16(dQ), "pointers must be 16-byte aligned");
  const DqPlan dq = dq_plan(B, Nc, d);
  const WsLayout wl = step_plan(B, Nc, d).wl;
  char* ws;
  if (int rc = claim_ws("dq", wl, workspace, workspace_bytes, dq.splits > 1, true, &ws)) return rc;
  return launch_dq(dq, G, C, B, Nc, d, h_scale, d_scale, dQ, ws, wl, (hipStream_t)stream, /*gemm_too=*/true, nullptr);
}

int dprhot_dc(const dprhot_bf16* G, const dprhot_bf16* Q, int B, int Nc, int d, float h_scale, const float* d_scale,
              float* dC_part, void* stream) {
  REQUIRE(G && Q && dC_part, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  REQUIRE(aligned16(G) && aligned16(Q) && aligned16(dC_part), "pointers must be 16-byte aligned");
  return dc_body(PackedSpec{}, G, Q, B, Nc, d, h_scale, d_scale, dC_part, (hipStream_t)stream);
}

int dprhot_rank_of_gold(const float* S, int rows, int cols, const int64_t* y, int64_t y_offset, int64_t* rank, void* stream) {
  REQUIRE(S && y && rank, "NULL pointer");
  REQUIRE(rows > 0 && cols > 0, "bad shape rows=%d cols=%d", rows, cols);
  if (cols % 4 != 0) return fail(DPRHOT_E_UNSUPPORTED, "cols=%d must be a multiple of 4", cols);
  REQUIRE(aligned16(S), "S must be 16-byte aligned");
  return launch<rank_kernel>(dim3(rows), dim3(256), 0, (hipStream_t)stream, S, rows, cols, y, y_offset, rank);
}

int dprhot_pairwise_fwd(const float* q, const float* c, const uint8_t* mask, int B, int M, int d, float* S, void* stream) {
  REQUIRE(q && c && S, "NULL pointer");
  REQUIRE(B > 0 && M > 0 && d > 0, "bad shape B=%d M=%d d=%d", B, M, d);
  REQUIRE((long)B * M <= 0x7fffffffL, "too many pairs");
  return launch<pairwise_fwd_kernel>(dim3((unsigned)(B * M)), dim3(256), 0, (hipStream_t)stream, q, c, mask, B, M, d, S);
}

int dprhot_pairwise_bwd(const float* g, const float* q, const float* c, int B, int M, int d, float* dq, float* dc, void* stream) {
  REQUIRE(g && q && c, "NULL pointer");
  REQUIRE(B > 0 && M > 0 && d > 0 && B <= 65535, "bad shape B=%d M=%d d=%d", B, M, d);
  return launch<pairwise_bwd_kernel>(dim3((unsigned)cdiv(d, 512), (unsigned)B), dim3(256), 0, (hipStream_t)stream, g, q, c, B, M, d, dq, dc);
}

static int launch_topk(const TopkArgs& p, int rows, hipStream_t st) {
  if (p.k <= TK_KSMALL) return launch<topk_stream_kernel<1024, TK_KSMALL, 4>>(dim3(rows), dim3(256), tk_lds_bytes(1024), st, p);
  if (p.k <= TK_KMAX) return launch<topk_stream_kernel<4096, TK_KMAX, 8>>(dim3(rows), dim3(256), tk_lds_bytes(4096), st, p);
  return launch<topk_stream_kernel<8192, TK_KWIDE, 8>>(dim3(rows), dim3(256), tk_lds_bytes(8192), st, p);  // 1024 < k <= 4096: 8192 slots
}

int dprhot_topk_update(const float* S, int rows, int cols, int64_t ld, int64_t col_offset, int k, float* values,
                       int64_t* indices, int first, void* stream) {
  REQUIRE(S && values && indices, "NULL pointer");
  REQUIRE(rows > 0 && cols > 0 && ld >= cols && k > 0 && k <= TK_KWIDE, "bad shape rows=%d cols=%d ld=%lld k=%d", rows, cols,
          (long long)ld, k);
  REQUIRE(col_offset >= 0, "negative col_offset");
  TopkArgs p{S, rows, cols, (long long)ld, (long long)col_offset, k, values, indices, first ? 1 : 0, nullptr, nullptr};
  return launch_topk(p, rows, (hipStream_t)stream);
}

int dprhot_topk(const float* S, int rows, int cols, int k, float* values, int64_t* indices, void* stream) {
  REQUIRE(k <= cols, "k=%d > cols=%d", k, cols);
  return dprhot_topk_update(S, rows, cols, cols, 0, k, values, indices, 1, stream);
}

// workspace of dprhot_search: [nq x chunk] fp32 (scores of the first chunk / candidate values) + [nq x chunk] int32
// (candidate columns) + [nq] int32 (candidate counts)
static size_t search_ws_bytes(int nq, int chunk) {
  return (size_t)nq * (size_t)chunk * 8 + ((size_t)nq * 4 + 255) / 256 * 256;
}

// ---- k beyond the LDS-resident selection kernels (csrc/wideselect.h): state in HBM, radix select + block sort + merge passes ----
static size_t wsel_ws_bytes(int rows, int k) {
  return align256((size_t)rows * WSEL_REC * 4) + 2 * (align256((size_t)rows * k * 4) + align256((size_t)rows * k * 8));
}
int dprhot_topk_wide_workspace_bytes(int rows, int k, size_t* h_out) {
  REQUIRE(h_out != nullptr && rows > 0 && k > 0, "bad argument");
  *h_out = wsel_ws_bytes(rows, k);
  return DPRHOT_OK;
}

int dprhot_topk_update_wide(const float* S, int rows, int cols, int64_t ld, int64_t col_offset, int k, float* values, int64_t* indices, int first,
                            void* workspace, size_t workspace_bytes, void* stream) {
  REQUIRE(S && values && indices && workspace, "NULL pointer");
  REQUIRE(rows > 0 && cols > 0 && k > 0 && ld >= cols, "bad shape rows=%d cols=%d k=%d ld=%lld", rows, cols, k, (long long)ld);
  REQUIRE((long long)k + cols < (1ll << 31), "k + cols must fit 31 bits");
  if (workspace_bytes < wsel_ws_bytes(rows, k)) return fail(DPRHOT_E_WORKSPACE, "topk_update_wide needs %zu workspace bytes, got %zu", wsel_ws_bytes(rows, k), workspace_bytes);
  REQUIRE(aligned16(workspace), "workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  unsigned* rec = reinterpret_cast<unsigned*>(ws);
  size_t off = align256((size_t)rows * WSEL_REC * 4);
  float* Av = reinterpret_cast<float*>(ws + off); off += align256((size_t)rows * k * 4);
  int64_t* Ai = reinterpret_cast<int64_t*>(ws + off); off += align256((size_t)rows * k * 8);
  float* Bv = reinterpret_cast<float*>(ws + off); off += align256((size_t)rows * k * 4);
  int64_t* Bi = reinterpret_cast<int64_t*>(ws + off);
  WselArgs a{S, rows, cols, (long long)ld, (long long)col_offset, k, values, indices, first, rec, Av, Ai};
  if (int rc = launch<wsel_select_kernel>(dim3((unsigned)rows), dim3(WSEL_THREADS), 0, st, a)) return rc;
  if (int rc = launch<wsel_collect_kernel>(dim3((unsigned)rows), dim3(WSEL_THREADS), 0, st, a)) return rc;
  const int nblk = cdiv(k, WSEL_BLOCK);
  if (int rc = launch<wsel_sort_kernel>(dim3((unsigned)rows, (unsigned)nblk), dim3(WSEL_THREADS), (size_t)WSEL_BLOCK * 12, st, Av, Ai, k)) return rc;
  int passes = 0;
  for (long long L = WSEL_BLOCK; L < k; L <<= 1) ++passes;
  const dim3 mgrid((unsigned)cdiv(k, WSEL_THREADS), (unsigned)rows);
  const float* sv = Av;
  const int64_t* si = Ai;
  if (passes == 0)  // one block: the sorted block IS the new state (a merge pass against an empty partner run copies it)
    return launch<wsel_merge_kernel>(mgrid, dim3(WSEL_THREADS), 0, st, sv, si, values, indices, k, WSEL_BLOCK, rec);
  long long L = WSEL_BLOCK;
  for (int j = 0; j < passes; ++j, L <<= 1) {
    const bool last = j == passes - 1;
    float* dv = last ? values : ((j & 1) == 0 ? Bv : Av);
    int64_t* di = last ? indices : ((j & 1) == 0 ? Bi : Ai);
    if (int rc = launch<wsel_merge_kernel>(mgrid, dim3(WSEL_THREADS), 0, st, sv, si, dv, di, k, (int)L, last ? rec : nullptr)) return rc;
    sv = dv;
    si = di;
  }
  return DPRHOT_OK;
}

int dprhot_search_workspace_bytes(int nq, int chunk, size_t* h_out) {
  REQUIRE(h_out != nullptr, "NULL out pointer");
  REQUIRE(nq > 0 && chunk > 0 && chunk % 8 == 0, "bad shape nq=%d chunk=%d", nq, chunk);
  *h_out = search_ws_bytes(nq, chunk);
  return DPRHOT_OK;
}

// ---- the plan of dprhot_search: every host decision of a call in one place ---------------------------------------------------------
// The form code of a launch (include/dprhot.h, dprhot_search_plan): 0..5 a register-staged tile of gemm_bf16.h, 6 the 256 x 256
// gemm256_kernel, 7 the phase-interleaved gemm8p_kernel, 8 tile 0 on LDS-DMA (gemm128d.h).  Derived from the same SimGemm and the same
// g128d_takes that the launch reads.
static int gemm_form(const SimGemm& g, int M, int N, int K) {
  if (g.g8) return 7;
  if (g.tile == kBigTile) return 6;
  const GemmArgs a{nullptr, nullptr, M, N, K, K, K, g.kchunk};
  return (g.tile == 0 && g128d_takes<true, true>(a)) ? 8 : g.tile;
}
struct SearchStep {
  int64_t j0;  // first row of the shard
  int cols;
  bool head;   // scores stored and selected from (dprhot_sim_fwd + dprhot_topk_update); else filtered in the GEMM epilogue and merged
  SimGemm g;
};
static int check_search_shape(int nq, int64_t n_ctx, int d, int k, int chunk) {
  REQUIRE(nq > 0 && n_ctx > 0 && d > 0 && d % 8 == 0, "bad shape nq=%d n_ctx=%lld d=%d", nq, (long long)n_ctx, d);
  REQUIRE(n_ctx % 8 == 0 && chunk > 0 && chunk % 8 == 0, "n_ctx=%lld and chunk=%d must be multiples of 8", (long long)n_ctx, chunk);
  REQUIRE(k > 0 && k <= TK_KMAX, "k=%d out of range (1..%d)", k, TK_KMAX);
  return DPRHOT_OK;
}
// Calls f(step) for every launch pair of a search over n_ctx rows, in order; stops at the first non-zero return and passes it on.
// An empty state is started from a SHORT head (its scores are materialised and selected from: cost proportional to the head), the
// filtered chunks behind it may be as long as the workspace allows: every chunk costs one merge launch, and a merge rewrites the
// whole state (k = 1000: 57 us each; 31 chunks of 65536 spent 1.7 ms of a 5.6 ms search merging)
// Behind the head every chunk is as long as everything scored before it (doubling, up to `chunk`): a chunk that covers the
// fraction f of the corpus behind a prefix s leaves ~k f / s candidates per row against the threshold of its start -- f = s keeps
// that at ~k (the merge's fast path holds 2048), f = 4 s left 4 k and a 790 us merge.
extern "C++" {
template <class F>
int search_plan(int nq, int64_t n_ctx, int d, int chunk, int first, F&& f) {
  const int head = chunk < 65536 ? chunk : 65536;
  for (int64_t j0 = 0, step = 0; j0 < n_ctx; j0 += step) {
    step = (first && j0 == 0) ? head : (first ? (j0 < chunk ? (j0 / 8 * 8 > head ? j0 / 8 * 8 : head) : chunk) : chunk);
    if (step > chunk) step = chunk;
    const int cols = (int)((n_ctx - j0 < step) ? (n_ctx - j0) : step);
    if (int rc = f(SearchStep{j0, cols, first && j0 == 0, sim_gemm(nq, cols, d)})) return rc;
  }
  return DPRHOT_OK;
}
}  // extern "C++"

int dprhot_search_plan(int nq, int64_t n_ctx, int d, int k, int chunk, int first, int64_t* h_steps, int capacity, int* h_count) {
  REQUIRE(h_count != nullptr && capacity >= 0 && (h_steps != nullptr || capacity == 0), "NULL pointer");
  if (int rc = check_search_shape(nq, n_ctx, d, k, chunk)) return rc;
  int n = 0;
  (void)search_plan(nq, n_ctx, d, chunk, first, [&](const SearchStep& s) {
    if (n < capacity) {
      int64_t* e = h_steps + (size_t)n * 4;
      e[0] = s.j0;
      e[1] = s.cols;
      e[2] = s.head ? 1 : 0;
      e[3] = gemm_form(s.g, nq, s.cols, d);
    }
    ++n;
    return DPRHOT_OK;
  });
  *h_count = n;
  REQUIRE(n <= capacity, "search plan has %d steps, capacity %d", n, capacity);
  return DPRHOT_OK;
}

int dprhot_search(const dprhot_bf16* Q, int nq, const dprhot_bf16* C, int64_t n_ctx, int d, int64_t id_offset, int k, int chunk,
                  float* values, int64_t* indices, int first, void* workspace, size_t workspace_bytes, void* stream) {
  REQUIRE(Q && C && values && indices, "NULL pointer");
  if (int rc = check_search_shape(nq, n_ctx, d, k, chunk)) return rc;
  REQUIRE(id_offset >= 0, "negative id_offset");
  REQUIRE(aligned16(Q) && aligned16(C), "pointers must be 16-byte aligned");
  const size_t need = search_ws_bytes(nq, chunk);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(DPRHOT_E_WORKSPACE, "search needs %zu workspace bytes (dprhot_search_workspace_bytes), got %zu", need, workspace_bytes);
  REQUIRE(aligned16(workspace), "workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* S = static_cast<float*>(workspace);
  int* cand_j = reinterpret_cast<int*>(static_cast<char*>(workspace) + (size_t)nq * chunk * 4);
  int* cnt = reinterpret_cast<int*>(static_cast<char*>(workspace) + (size_t)nq * chunk * 8);
  if (int rc = zero_words(cnt, (size_t)nq, st)) return rc;
  return search_plan(nq, n_ctx, d, chunk, first, [&](const SearchStep& s) -> int {
    const int cols = s.cols;
    const int64_t j0 = s.j0;
    const dprhot_bf16* Cj = C + (size_t)j0 * d;
    if (s.head) {
      // nothing to filter against yet: materialise this chunk's scores and select from them (the forward makes the same sim_gemm choice)
      if (int rc = dprhot_sim_fwd(Q, nq, Cj, cols, d, nullptr, 1.0f, S, stream)) return rc;
      return dprhot_topk_update(S, nq, cols, cols, id_offset + j0, k, values, indices, 1, stream);
    }
    // scores that cannot enter the top-k never leave the GEMM tile; one merge per chunk, at most `cols` candidates per row and chunk,
    // is what the workspace is sized for
    if (s.g.g8) {  // the phase-interleaved kernel (gemm8p.h); thresholds arrive with the tile's input words
      const Epi8Filter e8{values, indices, k, nq, cols, (long long)(id_offset + j0), cnt, S, cand_j, Q, 0};
      GemmArgs a8{Q, Cj, nq, cols, d, d, d, d};
      if (int rc = launch_g8(a8, e8, st)) return rc;
    } else {
      GemmArgs a{Q, Cj, nq, cols, d, d, d, s.g.kchunk};
      EpiFilter epi{values, indices, k, nq, cols, (long long)(id_offset + j0), cnt, S, cand_j};
      if (int rc = launch_gemm<true, true>(s.g.tile, a, epi, 1, st)) return rc;
    }
    TopkArgs p{S, nq, cols, (long long)cols, (long long)(id_offset + j0), k, values, indices, 0, cand_j, cnt};
    return launch_topk(p, nq, st);
  });
}

// ---- the training step: check the arguments, derive the plan once, claim the workspace, run the body with a default context ----
int dprhot_sim_stats(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                     const uint8_t* colmask, float inv_T, float* S_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_sim_stats(Q, C, y, S_out, B, Nc, d)) return rc;
  const StepPlan p = step_plan(B, Nc, d);
  char* ws;
  if (int rc = claim_ws("sim_stats", p.wl, workspace, workspace_bytes, true, true, &ws)) return rc;
  return sim_stats_body(PackedSpec{}, Q, B, C, Nc, d, y, y_offset, colmask, inv_T, S_out, p, ws, (hipStream_t)stream);
}

int dprhot_sim_stats_f32(const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d, const int64_t* y,
                         int64_t y_offset, const uint8_t* colmask, float inv_T, float* S_out, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (int rc = check_sim_stats_f32(q, c, Qb, Cb, y, S_out, B, Nc, d)) return rc;
  const StepPlan p = step_plan(B, Nc, d);
  char* ws;
  if (int rc = claim_ws("sim_stats", p.wl, workspace, workspace_bytes, true, true, &ws)) return rc;
  return sim_stats_f32_body(PackedSpec{}, q, c, Qb, Cb, B, Nc, d, y, y_offset, colmask, inv_T, S_out, p, ws, (hipStream_t)stream);
}

int dprhot_softmax_finish(const float* S_in, int B, int Nc, int d, const int64_t* y, int64_t y_offset, float grad_scale,
                          float* row_loss, float* row_lse, float* loss_sum, dprhot_bf16* G, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (int rc = check_softmax_finish(S_in, y, loss_sum, G, B, Nc, d)) return rc;
  const StepPlan p = step_plan(B, Nc, d);
  char* ws;
  if (int rc = claim_ws("softmax_finish", p.wl, workspace, workspace_bytes, true, false, &ws)) return rc;
  if (S_in == nullptr && p.nl && G != nullptr)
    return fail(DPRHOT_E_UNSUPPORTED, "softmax_finish: no logits at B=%d Nc=%d d=%d (no-logits forward): G comes from dprhot_dscores", B, Nc, d);
  return softmax_finish_body(StepCtx{}, S_in, B, Nc, d, y, y_offset, grad_scale, row_loss, row_lse, loss_sum, G, p, ws, (hipStream_t)stream);
}

// row_lse: the rows' logsumexp, or NULL to use the values dprhot_softmax_finish left in the workspace.
int dprhot_dscores(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                   const uint8_t* colmask, float inv_T, float grad_scale, const float* row_lse, dprhot_bf16* G, void* workspace,
                   size_t workspace_bytes, void* stream) {
  REQUIRE(Q && C && y && G, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  REQUIRE(aligned16(Q) && aligned16(C) && aligned16(G), "pointers must be 16-byte aligned");
  const StepPlan p = step_plan(B, Nc, d);
  if (!p.nl) return fail(DPRHOT_E_UNSUPPORTED, "dscores: B=%d Nc=%d d=%d is not a no-logits shape (use dprhot_softmax_finish)", B, Nc, d);
  char* ws;
  if (int rc = claim_ws("dscores", p.wl, workspace, workspace_bytes, row_lse == nullptr, false, &ws)) return rc;
  if (row_lse == nullptr) row_lse = reinterpret_cast<const float*>(ws + p.wl.lse);
  return dscores_body(PackedSpec{}, Q, B, C, Nc, d, y, y_offset, colmask, inv_T, grad_scale, row_lse, G, (hipStream_t)stream);
}

// Rank of every row's gold column in the stable descending order of its scores (dpr_task.py:235-246) straight from the
// embeddings: at no-logits shapes the score matrix is never written (gold logits from a gathered mini GEMM, then a count-greater
// epilogue inside the similarity GEMM); smaller problems materialise S in the workspace and count there.
int dprhot_sim_rank(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                    const uint8_t* colmask, float inv_T, int64_t* rank, void* workspace, size_t workspace_bytes, void* stream) {
  REQUIRE(Q && C && y && rank, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  REQUIRE(aligned16(Q) && aligned16(C), "pointers must be 16-byte aligned");
  const WsLayout wl = step_plan(B, Nc, d).wl;
  char* ws;
  if (int rc = claim_ws("sim_rank", wl, workspace, workspace_bytes, true, true, &ws)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!nl_ok(B, Nc, d)) {
    float* S = reinterpret_cast<float*>(ws + wl.logits);
    if (int rc = dprhot_sim_fwd(Q, B, C, Nc, d, colmask, inv_T, S, stream)) return rc;
    return dprhot_rank_of_gold(S, B, Nc, y, y_offset, rank, stream);
  }
  float* gold = reinterpret_cast<float*>(ws + wl.lse);
  int* count = reinterpret_cast<int*>(ws + wl.rloss);
  Epi8Count epi;
  static_cast<Epi8Base&>(epi) = g8_base(PackedSpec{}, Q, B, Nc, y, y_offset, colmask, inv_T, nullptr);
  epi.gold_val = gold;
  epi.count = count;
  if (int rc = launch<g8_gold_kernel>(dim3(cdiv(B, 32)), dim3(64), 0, st, Q, C, B, Nc, d, y, y_offset, epi.sim, inv_T, gold)) return rc;
  if (int rc = zero_words(count, (size_t)B, st)) return rc;
  GemmArgs a8{Q, C, B, Nc, d, d, d, d};
  if (int rc = launch_g8(a8, epi, st)) return rc;
  return launch<g8_rank_finish_kernel>(dim3(cdiv(B, 256)), dim3(256), 0, st, count, B, rank);
}

// compute_rank_metrics AND the cross-entropy of the same scores (dpr_task.py:224-227, :296-299) in one call: at no-logits shapes ONE
// pass of the similarity GEMM whose epilogue counts and keeps the strip statistics (Epi8CountStats); elsewhere the scores go to the
// workspace once and both readers stream them.
int dprhot_sim_rank_loss(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                         const uint8_t* colmask, float inv_T, int64_t* rank, float* row_loss, float* row_lse, float* loss_sum,
                         void* workspace, size_t workspace_bytes, void* stream) {
  REQUIRE(Q && C && y && rank && loss_sum, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  REQUIRE(aligned16(Q) && aligned16(C), "pointers must be 16-byte aligned");
  const WsLayout wl = step_plan(B, Nc, d).wl;
  char* ws;
  if (int rc = claim_ws("sim_rank_loss", wl, workspace, workspace_bytes, true, true, &ws)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!nl_ok(B, Nc, d)) {
    if (int rc = dprhot_sim_rank(Q, B, C, Nc, d, y, y_offset, colmask, inv_T, rank, workspace, workspace_bytes, stream)) return rc;
    return dprhot_inbatch_fwd(Q, B, C, Nc, d, y, y_offset, colmask, inv_T, 1.0f, nullptr, row_loss, row_lse, loss_sum, nullptr, workspace,
                              workspace_bytes, stream);
  }
  float* gold = reinterpret_cast<float*>(ws + wl.gold);
  int* count = reinterpret_cast<int*>(ws + wl.rloss);  // (the row losses take this place once the ranks have been read out of it)
  Epi8CountStats epi;
  static_cast<Epi8Base&>(epi) = g8_base(PackedSpec{}, Q, B, Nc, y, y_offset, colmask, inv_T, nullptr);
  epi.gold_val = gold;
  epi.count = count;
  epi.part_m = reinterpret_cast<float*>(ws + wl.part_m);
  epi.part_s = reinterpret_cast<float*>(ws + wl.part_s);
  epi.npart = cdiv(Nc, G2_B) * 4;
  if (int rc = launch<g8_gold_kernel>(dim3(cdiv(B, 32)), dim3(64), 0, st, Q, C, B, Nc, d, y, y_offset, epi.sim, inv_T, gold)) return rc;
  if (int rc = zero_words(count, (size_t)B, st)) return rc;
  GemmArgs a8{Q, C, B, Nc, d, d, d, d};
  if (int rc = launch_g8(a8, epi, st)) return rc;
  if (int rc = launch<g8_rank_finish_kernel>(dim3(cdiv(B, 256)), dim3(256), 0, st, count, B, rank)) return rc;
  if (int rc = launch<g8_lse_kernel>(dim3(cdiv(B, 4)), dim3(256), 0, st, epi.part_m, epi.part_s, epi.npart, gold, B, reinterpret_cast<float*>(ws + wl.lse),
                                     row_lse, row_loss, reinterpret_cast<float*>(ws + wl.rloss)))
    return rc;
  return launch_loss_sum(reinterpret_cast<const float*>(ws + wl.rloss), B, 1.0f, loss_sum, st, nullptr);
}

int dprhot_inbatch_fwd(const dprhot_bf16* Q, int B, const dprhot_bf16* C, int Nc, int d, const int64_t* y, int64_t y_offset,
                       const uint8_t* colmask, float inv_T, float grad_scale, float* S_out, float* row_loss, float* row_lse,
                       float* loss_sum, dprhot_bf16* G, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_sim_stats(Q, C, y, S_out, B, Nc, d)) return rc;
  if (int rc = check_softmax_finish(S_out, y, loss_sum, G, B, Nc, d)) return rc;
  const StepPlan p = step_plan(B, Nc, d);
  char* ws;
  if (int rc = claim_ws("inbatch_fwd", p.wl, workspace, workspace_bytes, true, true, &ws)) return rc;
  return inbatch_fwd_body(StepCtx{}, Q, B, C, Nc, d, y, y_offset, colmask, inv_T, grad_scale, S_out, row_loss, row_lse, loss_sum, G, p, ws,
                          (hipStream_t)stream);
}

int dprhot_inbatch_fwd_f32(const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d, const int64_t* y,
                           int64_t y_offset, const uint8_t* colmask, float inv_T, float grad_scale, float* S_out, float* row_loss,
                           float* row_lse, float* loss_sum, dprhot_bf16* G, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_sim_stats_f32(q, c, Qb, Cb, y, S_out, B, Nc, d)) return rc;
  if (int rc = check_softmax_finish(S_out, y, loss_sum, G, B, Nc, d)) return rc;
  const StepPlan p = step_plan(B, Nc, d);
  char* ws;
  if (int rc = claim_ws("inbatch_fwd", p.wl, workspace, workspace_bytes, true, true, &ws)) return rc;
  return inbatch_fwd_f32_body(StepCtx{}, q, c, Qb, Cb, B, Nc, d, y, y_offset, colmask, inv_T, grad_scale, S_out, row_loss, row_lse, loss_sum, G, p,
                              ws, (hipStream_t)stream);
}

int dprhot_inbatch_bwd(const dprhot_bf16* G, const dprhot_bf16* Q, const dprhot_bf16* C, int B, int Nc, int d, float h_scale,
                       const float* d_scale, float* dQ, float* dC_part, void* workspace, size_t workspace_bytes, void* stream) {
  REQUIRE(G && Q && C, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  // (an operand is read only by the product it belongs to: Q by dC, C by dQ)
  REQUIRE((dQ == nullptr && dC_part == nullptr) ||
              (aligned16(G) && aligned16(dQ) && aligned16(dC_part) && (dC_part == nullptr || aligned16(Q)) && (dQ == nullptr || aligned16(C))),
          "pointers must be 16-byte aligned");
  const StepPlan p = step_plan(B, Nc, d);
  const BwdPlan bp = bwd_plan(B, Nc, d, p.sk, dQ != nullptr && dC_part != nullptr, false);
  char* ws;
  if (int rc = claim_ws("inbatch_bwd", p.wl, workspace, workspace_bytes, dQ != nullptr && bp.slabs > 1, bp.kind == BWD_APART, &ws)) return rc;
  return inbatch_bwd_body(StepCtx{}, bp, G, Q, C, B, Nc, d, h_scale, d_scale, dQ, dC_part, p, ws, (hipStream_t)stream);
}

int dprhot_step_wants_g(int B, int Nc, int d, int* h_wants) {
  REQUIRE(h_wants != nullptr, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  *h_wants = step_plan(B, Nc, d).fz.ok ? 0 : 1;  // 0 where the few-rows plan takes the fused-dScores form
  return DPRHOT_OK;
}

int dprhot_fwd_one_pass(int B, int Nc, int d, int* h_kind) {
  REQUIRE(h_kind != nullptr, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  const FwdKind k = step_plan(B, Nc, d).fwd(false, true);
  *h_kind = k == FWD_ONE_PASS_128 ? 2 : (k == FWD_ONE_PASS_256 ? 1 : 0);
  return DPRHOT_OK;
}

int dprhot_fwd_no_logits(int B, int Nc, int d, int* h_nl) {
  REQUIRE(h_nl != nullptr, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  *h_nl = step_plan(B, Nc, d).nl ? 1 : 0;
  return DPRHOT_OK;
}

int dprhot_train_dq_slabs(int B, int Nc, int d, int* h_nslabs) {
  REQUIRE(h_nslabs != nullptr, "NULL pointer");
  if (int rc = check_shape(B, Nc, d)) return rc;
  *h_nslabs = step_plan(B, Nc, d).dq_slabs();
  return DPRHOT_OK;
}

int dprhot_inbatch_step_f32(const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d, const int64_t* y,
                            int64_t y_offset, const uint8_t* colmask, float inv_T, float grad_scale, float h_scale, const float* d_scale,
                            float* S_out, float* row_loss, float* row_lse, float* loss_sum, dprhot_bf16* G, float* dQ, float* dC_part,
                            void* workspace, size_t workspace_bytes, void* stream) {
  StepPlan p;
  if (int rc = step_admit(GC_FP32, nullptr, B, Nc, d, &p)) return rc;
  return run_step(StepCtx{}, p, q, c, Qb, Cb, B, Nc, d, y, y_offset, colmask, inv_T, grad_scale, h_scale, d_scale, S_out, row_loss, row_lse, loss_sum,
                  G, dQ, dC_part, workspace, workspace_bytes, (hipStream_t)stream);
}

// World size > 1, everything after the all-gather in ONE call: the column mask is read from the packed buffer (no
// unpack launch) and this rank's loss numerator rides in dC_part (no loss all-reduce): see include/dprhot.h.
int dprhot_inbatch_step_packed_f32(const float* q, const dprhot_bf16* gathered, dprhot_bf16* Qb, int B, int W, int rank, int n_ctx,
                                   int d, const int64_t* y, float inv_T, float grad_scale, float h_scale, const float* d_scale,
                                   float* row_loss, float* row_lse, float* loss_sum, dprhot_bf16* G, float* dQ, float* dC_part,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  StepCtx cx;
  int rows_c = 0;
  if (int rc = packed_spec(q, gathered, Qb, y, loss_sum, W, rank, n_ctx, d, &cx.packed, &rows_c)) return rc;
  StepPlan p;
  if (int rc = step_admit(GC_FP32, nullptr, B, W * rows_c, d, &p)) return rc;
  // the gathered buffer IS the context matrix: [W * rows_c, d] bf16, mask rows = always-masked columns
  return run_step(cx, p, q, nullptr, Qb, const_cast<dprhot_bf16*>(gathered), B, W * rows_c, d, y, (int64_t)rank * rows_c, nullptr, inv_T, grad_scale,
                  h_scale, d_scale, nullptr, row_loss, row_lse, loss_sum, G, dQ, dC_part, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- gradient all-reduce of the towers (reference hook: dpr_task.py:90-92) -------------------------------
static int gc_blocks(size_t groups) {
  const size_t want = (groups + 255) / 256;
  return (int)(want < 1 ? 1 : (want > (size_t)kNumCU * 8 ? (size_t)kNumCU * 8 : want));
}

// ---- the step as the autograd operator runs it ----------------------------------------------------------------------------------
int dprhot_train_step_f32(const float* q, const float* c, dprhot_bf16* Qb, dprhot_bf16* Cb, int B, int Nc, int d, const int64_t* y,
                          int64_t y_offset, const uint8_t* colmask, float inv_T, float grad_scale, float loss_scale, const float* d_scale,
                          float* row_loss, float* row_lse, float* loss_out, dprhot_bf16* G, float* dQ, float* dq_part, void* dC_part,
                          int dc_kind, void* workspace, size_t workspace_bytes, void* stream) {
  StepPlan p;
  if (int rc = step_admit(dc_kind, dq_part, B, Nc, d, &p)) return rc;
  StepCtx cx{PackedSpec{}, loss_scale, dc_kind == GC_BF16, dq_part};
  return run_step(cx, p, q, c, Qb, Cb, B, Nc, d, y, y_offset, colmask, inv_T, grad_scale, 1.0f, d_scale, nullptr, row_loss, row_lse, loss_out, G, dQ,
                  static_cast<float*>(dC_part), workspace, workspace_bytes, (hipStream_t)stream);
}

int dprhot_train_step_packed_f32(const float* q, const dprhot_bf16* gathered, dprhot_bf16* Qb, int B, int W, int rank, int n_ctx, int d,
                                 const int64_t* y, float inv_T, float grad_scale, float loss_scale, const float* d_scale, float* row_loss,
                                 float* row_lse, float* loss_out, dprhot_bf16* G, float* dQ, float* dq_part, void* dC_part, int dc_kind,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  REQUIRE(W > 0 && n_ctx > 0 && d > 0 && d % 8 == 0, "bad argument W=%d n_ctx=%d d=%d", W, n_ctx, d);
  int rows_c = 0;
  if (int rc = dprhot_packed_rows(n_ctx, d, &rows_c)) return rc;
  StepPlan p;
  if (int rc = step_admit(dc_kind, dq_part, B, W * rows_c, d, &p)) return rc;
  StepCtx cx{PackedSpec{}, loss_scale, dc_kind == GC_BF16, dq_part};
  if (int rc = packed_spec(q, gathered, Qb, y, loss_out, W, rank, n_ctx, d, &cx.packed, &rows_c)) return rc;
  return run_step(cx, p, q, nullptr, Qb, const_cast<dprhot_bf16*>(gathered), B, W * rows_c, d, y, (int64_t)rank * rows_c, nullptr, inv_T, grad_scale,
                  1.0f, d_scale, nullptr, row_loss, row_lse, loss_out, G, dQ, static_cast<float*>(dC_part), workspace, workspace_bytes,
                  (hipStream_t)stream);
}

int dprhot_rescale_grads(float* dQ, size_t n_dq, const float* dq_part, int nslabs, void* dC, size_t n_dc, int dc_kind, const float* go,
                         const float* used, float* out2, void* stream) {
  REQUIRE(go && used && out2, "NULL pointer");
  REQUIRE(out2 != go && out2 != used && out2 + 1 != go && out2 + 1 != used, "out2 must not alias go / used");
  REQUIRE((dQ != nullptr || n_dq == 0) && (dC != nullptr || n_dc == 0), "NULL gradient with a non-zero count");
  REQUIRE(n_dq % 8 == 0 && n_dc % 8 == 0, "counts must be multiples of 8 (n_dq=%zu n_dc=%zu)", n_dq, n_dc);
  REQUIRE(dc_kind == GC_FP32 || dc_kind == GC_BF16, "dc_kind=%d (2 fp32, 0 bf16)", dc_kind);
  REQUIRE(nslabs >= 0 && (nslabs == 0 || (dq_part != nullptr && n_dq > 0)), "nslabs=%d needs dq_part and dQ", nslabs);
  REQUIRE(aligned16(dQ) && aligned16(dC) && aligned16(dq_part), "pointers must be 16-byte aligned");
  // the common case leaves after two scalar loads: as few workgroups as still stream at full rate when the scale did change
  const size_t groups = (n_dq + n_dc) / 8;
  int nb = gc_blocks(groups / 4 + 1);
  if (nb > 2 * kNumCU) nb = 2 * kNumCU;
  int nqb = 0;
  if (nslabs > 0) {  // one 16-byte group of dQ per thread: the slab loads of a group are the latency chain
    nqb = (int)((n_dq / 8 + 255) / 256);
    nb += nqb;
  }
  const dim3 grid(nb), block(256);
  if (dc_kind == GC_FP32)
    return launch<rescale_grads_kernel<GC_FP32>>(grid, block, 0, (hipStream_t)stream, dQ, n_dq / 8, dq_part, nslabs, nqb, dC, n_dc / 8, go, used, out2);
  return launch<rescale_grads_kernel<GC_BF16>>(grid, block, 0, (hipStream_t)stream, dQ, n_dq / 8, dq_part, nslabs, nqb, dC, n_dc / 8, go, used, out2);
}

int dprhot_grad_pack(const float* bucket, size_t n, float scale, int wire, void* send, size_t n_padded, void* stream) {
  REQUIRE(bucket && send, "NULL pointer");
  REQUIRE(n > 0 && n_padded >= n && n_padded % 8 == 0, "bad sizes n=%zu n_padded=%zu (n_padded %% 8 == 0, >= n)", n, n_padded);
  REQUIRE(wire >= GC_BF16 && wire <= GC_FP32, "wire=%d (0 bf16, 1 fp16, 2 fp32)", wire);
  REQUIRE(aligned16(bucket) && aligned16(send), "pointers must be 16-byte aligned");
  const size_t tiles = (n_padded / 4 + 256 * GC_UT - 1) / (256 * GC_UT);
  REQUIRE(tiles < (1ull << 31), "n_padded=%zu", n_padded);
  const dim3 grid((unsigned)tiles), block(256);  // one workgroup per contiguous tile (gradcomm.h)
  hipStream_t st = (hipStream_t)stream;
  if (wire == GC_BF16) return launch<grad_pack_kernel<GC_BF16>>(grid, block, 0, st, bucket, n, scale, send, n_padded);
  if (wire == GC_FP16) return launch<grad_pack_kernel<GC_FP16>>(grid, block, 0, st, bucket, n, scale, send, n_padded);
  return launch<grad_pack_kernel<GC_FP32>>(grid, block, 0, st, bucket, n, scale, send, n_padded);
}

int dprhot_grad_sum_shards(const void* recv, int W, size_t shard, int wire, int out_kind, void* out, void* stream) {
  REQUIRE(recv && out, "NULL pointer");
  REQUIRE(W > 0 && shard > 0 && shard % 8 == 0, "bad sizes W=%d shard=%zu (shard %% 8 == 0)", W, shard);
  REQUIRE(wire >= GC_BF16 && wire <= GC_FP32 && (out_kind == wire || out_kind == GC_FP32), "wire=%d out_kind=%d (out = wire kind or fp32)", wire,
          out_kind);
  REQUIRE(aligned16(recv) && aligned16(out), "pointers must be 16-byte aligned");
  const dim3 grid(gc_blocks(shard / 8)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (wire == GC_BF16 && out_kind == GC_BF16) return launch<grad_sum_shards_kernel<GC_BF16, GC_BF16>>(grid, block, 0, st, recv, W, shard, out);
  if (wire == GC_BF16) return launch<grad_sum_shards_kernel<GC_BF16, GC_FP32>>(grid, block, 0, st, recv, W, shard, out);
  if (wire == GC_FP16 && out_kind == GC_FP16) return launch<grad_sum_shards_kernel<GC_FP16, GC_FP16>>(grid, block, 0, st, recv, W, shard, out);
  if (wire == GC_FP16) return launch<grad_sum_shards_kernel<GC_FP16, GC_FP32>>(grid, block, 0, st, recv, W, shard, out);
  return launch<grad_sum_shards_kernel<GC_FP32, GC_FP32>>(grid, block, 0, st, recv, W, shard, out);
}

int dprhot_grad_unpack(const void* full, int kind, float* bucket, size_t n, void* stream) {
  REQUIRE(full && bucket && n > 0, "bad argument");
  REQUIRE(kind >= GC_BF16 && kind <= GC_FP32, "kind=%d (0 bf16, 1 fp16, 2 fp32)", kind);
  REQUIRE(aligned16(full) && aligned16(bucket), "pointers must be 16-byte aligned");
  const size_t tiles = (n / 4 + 256 * GC_UT - 1) / (256 * GC_UT);
  REQUIRE(tiles < (1ull << 31), "n=%zu", n);
  const dim3 grid((unsigned)(tiles > 0 ? tiles : 1)), block(256);  // one workgroup per contiguous tile (gradcomm.h)
  hipStream_t st = (hipStream_t)stream;
  if (kind == GC_BF16) return launch<grad_unpack_kernel<GC_BF16>>(grid, block, 0, st, full, bucket, n);
  if (kind == GC_FP16) return launch<grad_unpack_kernel<GC_FP16>>(grid, block, 0, st, full, bucket, n);
  return launch<grad_unpack_kernel<GC_FP32>>(grid, block, 0, st, full, bucket, n);
}

}  // extern "C"

// ---- optional communicator: the path's collectives issued straight on the caller's stream ----
// torch.distributed wraps every collective in a stream hand-over (event to RCCL's stream and back) and ~17 us of host
// work; the path's three collectives are tiny and sit on the critical path of a ~10 us step.  RCCL is taken from the
// process (the librccl.so PyTorch already loaded) with dlopen/dlsym -- no link-time dependency, and the selftest and
// single-GPU users never touch it.
namespace {
struct RcclUniqueId { char internal[128]; };
typedef void* RcclComm;
struct RcclApi {
  int (*GetUniqueId)(RcclUniqueId*);
  int (*CommInitRank)(RcclComm*, int, RcclUniqueId, int);
  int (*CommDestroy)(RcclComm);
  int (*AllGather)(const void*, void*, size_t, int, RcclComm, hipStream_t);
  int (*ReduceScatter)(const void*, void*, size_t, int, int, RcclComm, hipStream_t);
  int (*AllReduce)(const void*, void*, size_t, int, int, RcclComm, hipStream_t);
  const char* (*GetErrorString)(int);
  int (*Send)(const void*, size_t, int, int, RcclComm, hipStream_t);
  int (*Recv)(void*, size_t, int, int, RcclComm, hipStream_t);
  int (*GroupStart)();
  int (*GroupEnd)();
  bool ok, p2p;
};
constexpr int kRcclInt8 = 0, kRcclFloat16 = 6, kRcclFloat32 = 7, kRcclBfloat16 = 9, kRcclSum = 0;

const RcclApi& rccl() {
  static const RcclApi api = []() {
    RcclApi a{};
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so", RTLD_NOW);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW);
    if (!h) return a;
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(h, "ncclAllGather"));
    a.ReduceScatter = reinterpret_cast<decltype(a.ReduceScatter)>(dlsym(h, "ncclReduceScatter"));
    a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(h, "ncclAllReduce"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    a.Send = reinterpret_cast<decltype(a.Send)>(dlsym(h, "ncclSend"));
    a.Recv = reinterpret_cast<decltype(a.Recv)>(dlsym(h, "ncclRecv"));
    a.GroupStart = reinterpret_cast<decltype(a.GroupStart)>(dlsym(h, "ncclGroupStart"));
    a.GroupEnd = reinterpret_cast<decltype(a.GroupEnd)>(dlsym(h, "ncclGroupEnd"));
    a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllGather && a.ReduceScatter && a.AllReduce && a.GetErrorString;
    a.p2p = a.ok && a.Send && a.Recv && a.GroupStart && a.GroupEnd;
    return a;
  }();
  return api;
}
struct DprhotComm { RcclComm comm; int W, rank; };
#define RCCL_TRY(expr)                                                                              \
  do {                                                                                              \
    const int r_ = (expr);                                                                          \
    if (r_ != 0) return fail(DPRHOT_E_HIP, "%s: %s", #expr, rccl().GetErrorString(r_));             \
  } while (0)
}  // namespace

extern "C" {

int dprhot_comm_unique_id(void* id128) {
  REQUIRE(id128 != nullptr, "NULL pointer");
  if (!rccl().ok) return fail(DPRHOT_E_UNSUPPORTED, "librccl.so (ncclGetUniqueId ...) not found in this process");
  RCCL_TRY(rccl().GetUniqueId(static_cast<RcclUniqueId*>(id128)));
  return DPRHOT_OK;
}

int dprhot_comm_init(const void* id128, int W, int rank, void** h_out) {
  REQUIRE(id128 && h_out && W > 0 && rank >= 0 && rank < W, "bad argument");
  if (!rccl().ok) return fail(DPRHOT_E_UNSUPPORTED, "librccl.so not found in this process");
  RcclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  RcclComm c = nullptr;
  RCCL_TRY(rccl().CommInitRank(&c, W, id, rank));  // collective over all W ranks, on the current HIP device
  *h_out = new DprhotComm{c, W, rank};
  return DPRHOT_OK;
}

int dprhot_comm_destroy(void* h) {
  if (h == nullptr) return DPRHOT_OK;
  DprhotComm* c = static_cast<DprhotComm*>(h);
  const int r = rccl().CommDestroy(c->comm);
  delete c;
  if (r != 0) return fail(DPRHOT_E_HIP, "ncclCommDestroy: %s", rccl().GetErrorString(r));
  return DPRHOT_OK;
}

int dprhot_allgather_ctx(void* h, const void* send, void* recv, size_t bytes_per_rank, void* stream) {
  REQUIRE(h && send && recv && bytes_per_rank > 0, "bad argument");
  DprhotComm* c = static_cast<DprhotComm*>(h);
  RCCL_TRY(rccl().AllGather(send, recv, bytes_per_rank, kRcclInt8, c->comm, (hipStream_t)stream));
  return DPRHOT_OK;
}

int dprhot_reducescatter_dc(void* h, const float* send, float* recv, size_t count_per_rank, void* stream) {
  REQUIRE(h && send && recv && count_per_rank > 0, "bad argument");
  DprhotComm* c = static_cast<DprhotComm*>(h);
  RCCL_TRY(rccl().ReduceScatter(send, recv, count_per_rank, kRcclFloat32, kRcclSum, c->comm, (hipStream_t)stream));
  return DPRHOT_OK;
}

int dprhot_reducescatter_rows(void* h, const void* send, void* recv, size_t count_per_rank, int kind, void* stream) {
  REQUIRE(h && send && recv && count_per_rank > 0, "bad argument");
  REQUIRE(kind >= GC_BF16 && kind <= GC_FP32, "kind=%d (0 bf16, 1 fp16, 2 fp32)", kind);
  DprhotComm* c = static_cast<DprhotComm*>(h);
  const int dt = kind == GC_BF16 ? kRcclBfloat16 : (kind == GC_FP16 ? kRcclFloat16 : kRcclFloat32);
  RCCL_TRY(rccl().ReduceScatter(send, recv, count_per_rank, dt, kRcclSum, c->comm, (hipStream_t)stream));
  return DPRHOT_OK;
}

int dprhot_allreduce_sum(void* h, float* buf, size_t count, void* stream) {
  REQUIRE(h && buf && count > 0, "bad argument");
  DprhotComm* c = static_cast<DprhotComm*>(h);
  RCCL_TRY(rccl().AllReduce(buf, buf, count, kRcclFloat32, kRcclSum, c->comm, (hipStream_t)stream));
  return DPRHOT_OK;
}

// ---- the same two collectives as direct all-pairs exchanges (SURVEY.md section 8(e) "Topology") ---------------------------------
// One RCCL group of W sends and W receives (the self pair included: a device copy): every peer's transfer is its own point-to-point
// operation, so on the fully connected node the W - 1 transfers of a rank travel over W - 1 different xGMI links at once.
int dprhot_comm_has_allpairs(void* h) {
  REQUIRE(h != nullptr, "bad argument");
  return rccl().p2p ? 1 : 0;
}

int dprhot_allgather_allpairs(void* h, const void* send, void* recv, size_t bytes_per_rank, void* stream) {
  REQUIRE(h && send && recv && bytes_per_rank > 0, "bad argument");
  if (!rccl().p2p) return fail(DPRHOT_E_UNSUPPORTED, "ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd not found in this process's librccl.so");
  DprhotComm* c = static_cast<DprhotComm*>(h);
  hipStream_t st = (hipStream_t)stream;
  RCCL_TRY(rccl().GroupStart());
  int rc = 0;
  for (int k = 0; k < c->W && rc == 0; ++k) {
    rc = rccl().Send(send, bytes_per_rank, kRcclInt8, k, c->comm, st);
    if (rc == 0) rc = rccl().Recv(static_cast<char*>(recv) + (size_t)k * bytes_per_rank, bytes_per_rank, kRcclInt8, k, c->comm, st);
  }
  const int rc2 = rccl().GroupEnd();  // (always closed: an open group would swallow the caller's next collective)
  if (rc != 0) return fail(DPRHOT_E_HIP, "ncclSend / ncclRecv: %s", rccl().GetErrorString(rc));
  if (rc2 != 0) return fail(DPRHOT_E_HIP, "ncclGroupEnd: %s", rccl().GetErrorString(rc2));
  return DPRHOT_OK;
}

int dprhot_reducescatter_allpairs(void* h, const void* send, void* tmp, void* recv, size_t count_per_rank, int kind, int out_kind, void* stream) {
  REQUIRE(h && send && tmp && recv && count_per_rank > 0, "bad argument");
  REQUIRE(kind >= GC_BF16 && kind <= GC_FP32 && (out_kind == kind || out_kind == GC_FP32), "kind=%d out_kind=%d (0 bf16, 1 fp16, 2 fp32; out = kind or fp32)", kind, out_kind);
  REQUIRE(count_per_rank % 8 == 0, "count_per_rank=%zu must be a multiple of 8", count_per_rank);
  if (!rccl().p2p) return fail(DPRHOT_E_UNSUPPORTED, "ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd not found in this process's librccl.so");
  DprhotComm* c = static_cast<DprhotComm*>(h);
  hipStream_t st = (hipStream_t)stream;
  const size_t es = kind == GC_FP32 ? 4 : 2;
  const int dt = kind == GC_BF16 ? kRcclBfloat16 : (kind == GC_FP16 ? kRcclFloat16 : kRcclFloat32);
  RCCL_TRY(rccl().GroupStart());
  int rc = 0;
  for (int k = 0; k < c->W && rc == 0; ++k) {
    rc = rccl().Send(static_cast<const char*>(send) + (size_t)k * count_per_rank * es, count_per_rank, dt, k, c->comm, st);
    if (rc == 0) rc = rccl().Recv(static_cast<char*>(tmp) + (size_t)k * count_per_rank * es, count_per_rank, dt, k, c->comm, st);
  }
  const int rc2 = rccl().GroupEnd();
  if (rc != 0) return fail(DPRHOT_E_HIP, "ncclSend / ncclRecv: %s", rccl().GetErrorString(rc));
  if (rc2 != 0) return fail(DPRHOT_E_HIP, "ncclGroupEnd: %s", rccl().GetErrorString(rc2));
  return dprhot_grad_sum_shards(tmp, c->W, count_per_rank, kind, out_kind, recv, stream);  // fp32 accumulation, rank order
}

int dprhot_maxsim_workspace_bytes(int Nq, int LQ, int KQ, int Ny, int has_weights, size_t* bytes) {
  REQUIRE(bytes, "NULL pointer");
  size_t off[4];
  return ms_ws_layout(Nq, LQ, KQ, Ny, has_weights != 0, off, bytes);
}

int dprhot_maxsim_fwd(const void* q_tok, const void* c_tok, int Nq, int LQ, int Nc, int LD, int dp, const int* q_ids, const int* c_ids,
                      const float* q_w, const float* c_w, int KQ, int KD, int pool, int M, const uint8_t* mask, float* S, void* ws,
                      size_t ws_bytes, void* stream) {
  MsArgs p;
  const int rc = ms_setup(p, q_tok, c_tok, Nq, LQ, Nc, LD, dp, q_ids, c_ids, q_w, c_w, KQ, KD, pool, M, mask, ws, ws_bytes);
  if (rc) return rc;
  REQUIRE(S, "NULL pointer (S)");
  p.S = S;
  hipStream_t st = (hipStream_t)stream;
  const long ntiles = M > 0 ? (long)Nq * ((LQ + MS_BM - 1) / MS_BM) : ((long)Nq * LQ + MS_BM - 1) / MS_BM;
  const unsigned blocks = (unsigned)(ntiles * p.Ny);
  const int r1 = KQ == 1 ? ms_launch_fwd<1>(p, blocks, st) : KQ == 2 ? ms_launch_fwd<2>(p, blocks, st)
               : KQ <= 4 ? ms_launch_fwd<4>(p, blocks, st) : ms_launch_fwd<8>(p, blocks, st);
  if (r1) return r1;
  return launch<ms_pool_kernel>(dim3((unsigned)(((long)Nq * p.Ny + 3) / 4)), dim3(256), 0, st, p);
}

int dprhot_maxsim_score(const void* q_tok, const void* c_tok, int Nq, int LQ, int Nc, int LD, int dp, const int* q_ids, const int* c_ids,
                        const float* q_w, const float* c_w, int KQ, int KD, int pool, int M, const uint8_t* mask, float* S, void* stream) {
  REQUIRE(Nq >= 0 && Nc >= 0 && LQ > 0 && LD > 0, "bad shape Nq=%d LQ=%d Nc=%d LD=%d", Nq, LQ, Nc, LD);
  REQUIRE(LQ <= DPRHOT_MAXSIM_MAX_LEN && LD <= DPRHOT_MAXSIM_MAX_LEN, "LQ=%d LD=%d: token counts are limited to %d", LQ, LD,
          DPRHOT_MAXSIM_MAX_LEN);
  REQUIRE(dp >= 32 && dp % 32 == 0, "dp=%d must be a positive multiple of 32 (zero-pad the features)", dp);
  REQUIRE(KQ >= 1 && KQ <= MS_KMAX && KD >= 1 && KD <= MS_KMAX, "KQ=%d KD=%d: expert slots per token are limited to 1..%d", KQ, KD,
          MS_KMAX);
  REQUIRE((q_ids == nullptr) == (c_ids == nullptr), "expert ids are required on both sides or on neither");
  REQUIRE((q_w == nullptr) == (c_w == nullptr), "expert weights are required on both sides or on neither");
  REQUIRE(q_ids || (KQ == 1 && KD == 1), "KQ=%d KD=%d without expert ids (ColBERT has one slot per token)", KQ, KD);
  REQUIRE(pool == DPRHOT_POOL_SUM || pool == DPRHOT_POOL_MAX, "pool=%d (0 sum, 1 max)", pool);
  REQUIRE(M >= 1 && (long)Nq * M == (long)Nc, "pairwise: M=%d must be at least 1 and Nc=%d equal Nq * M = %d * %d", M, Nc, Nq, M);
  if (Nc == 0) return DPRHOT_OK;
  REQUIRE(q_tok && c_tok && S, "NULL pointer (q_tok, c_tok and S are required)");
  REQUIRE(((uintptr_t)q_tok & 15) == 0 && ((uintptr_t)c_tok & 15) == 0, "token rows must be 16-byte aligned");
  REQUIRE((long)Nq * LQ * KQ <= 0x7fffffffL && (long)Nc * LD * KD <= 0x7fffffffL, "too many token slots");
  const MsArgs p{(const uint16_t*)q_tok, (const uint16_t*)c_tok, q_ids, c_ids, q_w, c_w, mask, Nq, LQ, Nc, LD, dp, KQ, KD, M, M, pool,
                 nullptr, nullptr, nullptr, nullptr, S};
  hipStream_t st = (hipStream_t)stream;
  return KQ == 1 ? ms_launch_score<1>(p, st) : KQ == 2 ? ms_launch_score<2>(p, st)
       : KQ <= 4 ? ms_launch_score<4>(p, st) : ms_launch_score<8>(p, st);
}

int dprhot_maxsim_bwd(const float* dS, const void* q_tok, const void* c_tok, int Nq, int LQ, int Nc, int LD, int dp, const int* q_ids,
                      const int* c_ids, const float* q_w, const float* c_w, int KQ, int KD, int pool, int M, const uint8_t* mask,
                      const void* ws, size_t ws_bytes, float* dq, float* dc, float* dwq, float* dwc, void* stream) {
  MsArgs p;
  const int rc = ms_setup(p, q_tok, c_tok, Nq, LQ, Nc, LD, dp, q_ids, c_ids, q_w, c_w, KQ, KD, pool, M, mask, ws, ws_bytes);
  if (rc) return rc;
  REQUIRE(dS, "NULL pointer (dS)");
  REQUIRE(!(dwq || dwc) || q_w, "weight gradients need the expert weights");
  MsBwd g{dS, dq, dc, q_w ? dwq : nullptr, q_w ? dwc : nullptr};
  if (!(dq || dc || g.dwq || g.dwc)) return DPRHOT_OK;
  hipStream_t st = (hipStream_t)stream;
  if (q_ids && q_w) return ms_launch_bwd<true, true>(p, g, st);
  if (q_ids) return ms_launch_bwd<true, false>(p, g, st);
  if (q_w) return ms_launch_bwd<false, true>(p, g, st);
  return ms_launch_bwd<false, false>(p, g, st);
}

// ---- CITADEL / SPLADE router head (csrc/router_head.h): entry points ----
int dprhot_router_head_workspace_bytes(int B, int T, int V, int k, int want_softmax, size_t* bytes) {
  REQUIRE(bytes != nullptr, "NULL out pointer");
  REQUIRE(T >= 1, "T=%d: at least one token row", T);
  const int rc = rh_check_shape(B, T, V, 0, k);
  if (rc) return rc;
  *bytes = want_softmax ? align256((size_t)B * (size_t)T * 4) : 0;
  return DPRHOT_OK;
}

int dprhot_router_head_fwd(const void* logits, int dtype, int B, int T1, int V, int64_t stride_b, int64_t stride_t, const uint8_t* mask,
                           int skip, int k, int want_softmax, void* router_repr, int32_t* argmax, void* expert_weights,
                           int32_t* expert_ids, void* router_mask, void* softmax_sum, void* workspace, size_t workspace_bytes,
                           void* stream) {
  int rc = rh_check_shape(B, T1, V, skip, k);
  if (rc) return rc;
  if ((rc = rh_check_dtype(dtype))) return rc;
  REQUIRE(logits && mask && router_repr && argmax, "NULL pointer (logits, mask, router_repr and argmax are required)");
  REQUIRE(k == 0 || (expert_weights && expert_ids && router_mask), "NULL pointer (k > 0 needs expert_weights, expert_ids and router_mask)");
  REQUIRE(!want_softmax || softmax_sum, "NULL pointer (softmax_sum)");
  REQUIRE(stride_t >= V && stride_b >= 0, "strides: stride_t=%lld must be at least V=%d", (long long)stride_t, V);
  const int T = T1 - skip;
  const size_t need = want_softmax ? align256((size_t)B * (size_t)T * 4) : 0;
  if (need > 0 && (workspace == nullptr || workspace_bytes < need))
    return fail(DPRHOT_E_WORKSPACE, "workspace of %zu bytes, %zu needed (dprhot_router_head_workspace_bytes)", workspace_bytes, need);
  RhArgs a{};
  a.x = logits; a.mask = mask; a.B = B; a.T1 = T1; a.T = T; a.V = V; a.skip = skip; a.k = k; a.want_soft = want_softmax != 0;
  a.sb = stride_b; a.st = stride_t;
  a.repr = router_repr; a.arg = argmax; a.w = expert_weights; a.ids = expert_ids; a.rmask = router_mask; a.ssum = softmax_sum;
  a.lse = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == RH_FP32) return rh_launch_fwd<RH_FP32>(a, st);
  if (dtype == RH_BF16) return rh_launch_fwd<RH_BF16>(a, st);
  return rh_launch_fwd<RH_FP16>(a, st);
}

int dprhot_router_head_bwd(const void* logits, int dtype, int B, int T1, int V, int64_t stride_b, int64_t stride_t, const uint8_t* mask,
                           int skip, int k, const int32_t* argmax, const int32_t* expert_ids, const void* workspace,
                           size_t workspace_bytes, const float* g_router_repr, const float* g_expert_weights, const float* g_softmax_sum,
                           void* dlogits, void* stream) {
  int rc = rh_check_shape(B, T1, V, skip, k);
  if (rc) return rc;
  if ((rc = rh_check_dtype(dtype))) return rc;
  REQUIRE(logits && mask && dlogits, "NULL pointer (logits, mask and dlogits are required)");
  REQUIRE(!g_router_repr || argmax, "NULL pointer (g_router_repr needs the forward's argmax)");
  REQUIRE(!g_expert_weights || (k > 0 && expert_ids), "g_expert_weights needs k > 0 and the forward's expert_ids");
  REQUIRE(stride_t >= V && stride_b >= 0, "strides: stride_t=%lld must be at least V=%d", (long long)stride_t, V);
  const int T = T1 - skip;
  if (g_softmax_sum) {
    const size_t need = align256((size_t)B * (size_t)T * 4);
    if (workspace == nullptr || workspace_bytes < need)
      return fail(DPRHOT_E_WORKSPACE, "workspace of %zu bytes, %zu needed (the forward's, with want_softmax)", workspace_bytes, need);
  }
  RhArgs a{};
  a.x = logits; a.mask = mask; a.B = B; a.T1 = T1; a.T = T; a.V = V; a.skip = skip; a.k = k;
  a.sb = stride_b; a.st = stride_t;
  a.arg = const_cast<int*>(argmax); a.ids = const_cast<int*>(expert_ids); a.lse = (float*)const_cast<void*>(workspace);
  a.g_repr = g_router_repr; a.g_w = g_expert_weights; a.g_soft = g_softmax_sum; a.dx = dlogits;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == RH_FP32) return rh_launch_bwd<RH_FP32>(a, st);
  if (dtype == RH_BF16) return rh_launch_bwd<RH_BF16>(a, st);
  return rh_launch_bwd<RH_FP16>(a, st);
}

// ---- inverted-index retrieval (csrc/ivf.h) ----
constexpr int IVF_MAX_ENTRIES_PER_QUERY = 4096;

// one chunk's score buffer, nq x chunk fp32: the workspace of every chunked search up to k = TK_KWIDE
static size_t chunk_ws_bytes(int nq, int chunk) { return align256((size_t)nq * (size_t)chunk * 4); }

// the output window of the *_score entry points: S [nq, ld] takes doc ids doc_begin .. doc_begin + cols, which end at or below `limit`
// (corpus_len where the index knows it, 2^31 where it does not)
static int check_score_window(const float* S, int cols, int64_t ld, int64_t doc_begin, int64_t limit) {
  REQUIRE(S != nullptr, "NULL pointer (S)");
  REQUIRE(cols > 0 && ld >= cols, "bad shape cols=%d ld=%lld", cols, (long long)ld);
  if (limit == (1ll << 31)) {
    REQUIRE(doc_begin >= 0 && doc_begin + cols < limit, "doc ids %lld .. +%d must stay below 2^31", (long long)doc_begin, cols);
  } else {
    REQUIRE(doc_begin >= 0 && doc_begin + cols <= limit, "doc ids %lld .. +%d outside the corpus of %lld", (long long)doc_begin, cols,
            (long long)limit);
  }
  return DPRHOT_OK;
}

extern "C++" {
// The one chunked top-k search ("The chunk driver"): walks the doc ids [id_begin, id_end) in chunks, has
// fill(j0, cols, S, ld) write the scores of doc ids j0 .. j0 + cols into S [nq, ld] and folds them into the running top-k, with the
// HBM-resident selection above k = TK_KWIDE.  The workspace is one chunk's scores, then the wide selection's state.  `who` names the
// caller in the workspace error.
template <class Fill>
static int topk_search_chunks(const char* who, Fill fill, int nq, int64_t corpus_len, int64_t id_begin, int64_t id_end, int k, int chunk,
                              float* values, int64_t* indices, int first, void* workspace, size_t workspace_bytes, void* stream) {
  REQUIRE(values && indices, "NULL pointer");
  REQUIRE(corpus_len > 0 && corpus_len < (1ll << 31), "corpus_len=%lld out of range (1 .. 2^31 - 1)", (long long)corpus_len);
  REQUIRE(k >= 1 && k <= corpus_len, "topk=%d out of range (1 .. corpus_len=%lld)", k, (long long)corpus_len);
  REQUIRE(0 <= id_begin && id_begin < id_end && id_end <= corpus_len, "bad doc-id range [%lld, %lld) of %lld", (long long)id_begin,
          (long long)id_end, (long long)corpus_len);
  REQUIRE(chunk > 0 && chunk % 8 == 0, "chunk=%d must be a positive multiple of 8", chunk);
  const bool wide = k > TK_KWIDE;
  const size_t s_bytes = chunk_ws_bytes(nq, chunk);
  const size_t need = s_bytes + (wide ? wsel_ws_bytes(nq, k) : 0);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(DPRHOT_E_WORKSPACE, "%s_search needs %zu workspace bytes (dprhot_%s_workspace_bytes%s), got %zu", who, need, who,
                wide ? " + dprhot_topk_wide_workspace_bytes" : "", workspace_bytes);
  REQUIRE(aligned16(workspace), "workspace must be 16-byte aligned");
  float* S = static_cast<float*>(workspace);
  void* wide_ws = static_cast<char*>(workspace) + s_bytes;
  for (int64_t j0 = id_begin; j0 < id_end; j0 += chunk) {
    const int cols = (int)(id_end - j0 < chunk ? id_end - j0 : chunk);
    const int ld = (cols + 7) / 8 * 8;  // (<= chunk: chunk is a multiple of 8)
    if (int rc = fill(j0, cols, S, ld)) return rc;
    const int f = (first && j0 == id_begin) ? 1 : 0;
    if (wide) {
      if (int rc = dprhot_topk_update_wide(S, nq, cols, ld, j0, k, values, indices, f, wide_ws, workspace_bytes - s_bytes, stream)) return rc;
    } else {
      if (int rc = dprhot_topk_update(S, nq, cols, ld, j0, k, values, indices, f, stream)) return rc;
    }
  }
  return DPRHOT_OK;
}
}  // extern "C++"

static int ivf_check_batch(int nq, int n_entries, int n_bexp, const void* ent_vec, const void* ent_q, const void* bexp, const void* bexp_off) {
  REQUIRE(nq > 0, "bad shape nq=%d", nq);
  REQUIRE(n_entries >= 0 && n_bexp >= 0 && n_bexp <= n_entries, "bad batch n_entries=%d n_bexp=%d", n_entries, n_bexp);
  REQUIRE((long long)n_entries <= (long long)nq * IVF_MAX_ENTRIES_PER_QUERY, "n_entries=%d: at most %d entries per query", n_entries,
          IVF_MAX_ENTRIES_PER_QUERY);
  REQUIRE(n_entries == 0 || n_bexp > 0, "entries without a batch expert list");
  REQUIRE(n_entries == 0 || (ent_vec && ent_q && bexp && bexp_off), "NULL pointer (query batch)");
  REQUIRE(n_entries == 0 || aligned16(ent_vec), "entry vectors must be 16-byte aligned");
  return DPRHOT_OK;
}

// the postings' frame, shared by the dense and the product-quantised index: `rows` is post_vec or post_code
static int ivf_check_postings(const void* rows, const void* post_doc, const void* exp_off, int64_t n_postings, int n_experts) {
  REQUIRE(n_postings >= 0 && n_postings < (1ll << 40), "n_postings=%lld out of range (< 2^40)", (long long)n_postings);
  REQUIRE(n_experts > 0 && exp_off, "bad index: n_experts=%d", n_experts);
  REQUIRE(n_postings == 0 || (rows && post_doc), "NULL pointer (postings)");
  return DPRHOT_OK;
}

static int ivf_check_index(const void* post_vec, const void* post_doc, const void* exp_off, int64_t n_postings, int n_experts, int dp) {
  if (int rc = ivf_check_postings(post_vec, post_doc, exp_off, n_postings, n_experts)) return rc;
  REQUIRE(dp > 0 && dp % 32 == 0, "dp=%d must be a positive multiple of 32 (pad with zeros)", dp);
  REQUIRE(n_postings == 0 || aligned16(post_vec), "posting vectors must be 16-byte aligned");
  return DPRHOT_OK;
}

// the CLS part of an IVF search: both sides or neither, cls_doc with its zero rows behind the last doc id searched
static int ivf_check_cls(const dprhot_bf16* cls_q, const dprhot_bf16* cls_doc, int dc, int64_t cls_rows, int64_t id_end) {
  if (cls_q == nullptr && cls_doc == nullptr) return DPRHOT_OK;
  REQUIRE(cls_q && cls_doc, "CLS vectors of one side only");
  REQUIRE(dc > 0 && dc % 8 == 0, "dc=%d must be a positive multiple of 8 (pad with zeros)", dc);
  REQUIRE(cls_rows >= 7 && cls_rows - 7 >= id_end, "cls_doc has %lld rows; %lld needed (corpus_len + 7, zero rows behind the corpus)",
          (long long)cls_rows, (long long)((unsigned long long)id_end + 7));
  REQUIRE(aligned16(cls_q) && aligned16(cls_doc), "CLS vectors must be 16-byte aligned");
  return DPRHOT_OK;
}

int dprhot_ivf_workspace_bytes(int nq, int n_entries, int chunk, int has_cls, size_t* bytes) {
  REQUIRE(bytes != nullptr, "NULL out pointer");
  REQUIRE(nq > 0 && chunk > 0 && chunk % 8 == 0, "bad shape nq=%d chunk=%d (chunk: a positive multiple of 8)", nq, chunk);
  REQUIRE(n_entries >= 0 && (long long)n_entries <= (long long)nq * IVF_MAX_ENTRIES_PER_QUERY, "n_entries=%d: at most %d entries per query",
          n_entries, IVF_MAX_ENTRIES_PER_QUERY);
  (void)has_cls;  // the CLS scores are written straight into the chunk's score buffer
  *bytes = chunk_ws_bytes(nq, chunk);
  return DPRHOT_OK;
}

int dprhot_ivf_score(const dprhot_bf16* post_vec, const int32_t* post_doc, const int64_t* exp_off, int64_t n_postings, int n_experts, int dp,
                     const dprhot_bf16* ent_vec, const int32_t* ent_q, int n_entries, const int32_t* bexp, const int32_t* bexp_off,
                     int n_bexp, int nq, int64_t doc_begin, int cols, float* S, int64_t ld, void* stream) {
  if (int rc = ivf_check_index(post_vec, post_doc, exp_off, n_postings, n_experts, dp)) return rc;
  if (int rc = ivf_check_batch(nq, n_entries, n_bexp, ent_vec, ent_q, bexp, bexp_off)) return rc;
  if (int rc = check_score_window(S, cols, ld, doc_begin, 1ll << 31)) return rc;
  if (n_entries == 0 || n_postings == 0) return DPRHOT_OK;
  IvfArgs a{reinterpret_cast<const uint16_t*>(post_vec), post_doc, reinterpret_cast<const long long*>(exp_off), n_experts, dp,
            reinterpret_cast<const uint16_t*>(ent_vec), ent_q, bexp, bexp_off, n_bexp, nq, (long long)doc_begin, cols, S, (long long)ld};
  const unsigned blocks = (unsigned)cdiv(cdiv(cols, IVF_T), IVF_WAVES);
  return launch<ivf_score_kernel>(dim3(blocks), dim3(64 * IVF_WAVES), 0, (hipStream_t)stream, a);
}

extern "C++" {
// dprhot_ivf_search and dprhot_ivf_pq_search behind their index and batch checks: the chunk driver over a fill that starts S from the
// CLS scores of the chunk's doc ids (zeros without CLS vectors) and has score(j0, cols, S, ld) add the expert part
template <class Score>
static int ivf_search_with(Score score, int nq, const dprhot_bf16* cls_q, const dprhot_bf16* cls_doc, int dc, int64_t cls_rows,
                           int64_t corpus_len, int64_t id_begin, int64_t id_end, int k, int chunk, float* values, int64_t* indices,
                           int first, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = ivf_check_cls(cls_q, cls_doc, dc, cls_rows, id_end)) return rc;
  auto fill = [&](int64_t j0, int cols, float* S, int ld) {
    if (cls_q) {
      if (int rc = dprhot_sim_fwd(cls_q, nq, cls_doc + (size_t)j0 * dc, ld, dc, nullptr, 1.0f, S, stream)) return rc;
    } else {
      if (int rc = zero_words(S, (size_t)nq * ld, (hipStream_t)stream)) return rc;
    }
    return score(j0, cols, S, ld);
  };
  return topk_search_chunks("ivf", fill, nq, corpus_len, id_begin, id_end, k, chunk, values, indices, first, workspace, workspace_bytes,
                            stream);
}
}  // extern "C++"

int dprhot_ivf_search(const dprhot_bf16* post_vec, const int32_t* post_doc, const int64_t* exp_off, int64_t n_postings, int n_experts, int dp,
                      const dprhot_bf16* ent_vec, const int32_t* ent_q, int n_entries, const int32_t* bexp, const int32_t* bexp_off,
                      int n_bexp, int nq, const dprhot_bf16* cls_q, const dprhot_bf16* cls_doc, int dc, int64_t cls_rows,
                      int64_t corpus_len, int64_t id_begin, int64_t id_end, int k, int chunk, float* values, int64_t* indices, int first,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = ivf_check_index(post_vec, post_doc, exp_off, n_postings, n_experts, dp)) return rc;
  if (int rc = ivf_check_batch(nq, n_entries, n_bexp, ent_vec, ent_q, bexp, bexp_off)) return rc;
  auto score = [&](int64_t j0, int cols, float* S, int ld) {
    return dprhot_ivf_score(post_vec, post_doc, exp_off, n_postings, n_experts, dp, ent_vec, ent_q, n_entries, bexp, bexp_off, n_bexp, nq, j0,
                            cols, S, ld, stream);
  };
  return ivf_search_with(score, nq, cls_q, cls_doc, dc, cls_rows, corpus_len, id_begin, id_end, k, chunk, values, indices, first, workspace,
                         workspace_bytes, stream);
}

// ---- product-quantised postings (csrc/ivf_pq.h) ----
static int pq_check_shape(int dp, int dsub) {
  REQUIRE(dsub == 2 || dsub == 4 || dsub == 8, "dsub=%d: sub-vectors of 2, 4 or 8 features", dsub);
  REQUIRE(dp > 0 && dp % 32 == 0, "dp=%d must be a positive multiple of 32 (pad with zeros)", dp);
  if (dp > 64) return fail(DPRHOT_E_UNSUPPORTED, "dp=%d: product-quantised postings are built for dp = 32 and 64", dp);
  return DPRHOT_OK;
}

static int ivf_pq_check_index(const void* post_code, const void* codebook, int dsub, const void* post_doc, const void* exp_off,
                              int64_t n_postings, int n_experts, int dp) {
  if (int rc = ivf_check_postings(post_code, post_doc, exp_off, n_postings, n_experts)) return rc;
  REQUIRE(codebook != nullptr, "NULL pointer (codebook)");
  if (int rc = pq_check_shape(dp, dsub)) return rc;
  REQUIRE(aligned16(codebook) && (n_postings == 0 || aligned16(post_code)), "codes and codebook must be 16-byte aligned");
  return DPRHOT_OK;
}

extern "C++" {
template <int DSUB>
static int ivf_pq_launch(int dp, unsigned blocks, hipStream_t st, const IvfPqArgs& a) {
  if (dp == 32) return launch<ivf_pq_score_kernel<DSUB, 32>>(dim3(blocks), dim3(64 * IVF_WAVES), 0, st, a);
  return launch<ivf_pq_score_kernel<DSUB, 64>>(dim3(blocks), dim3(64 * IVF_WAVES), 0, st, a);
}
}  // extern "C++"

// dprhot_pq_encode and dprhot_colbert_pq_encode: the same rule and kernel behind each entry's own limit on dp (`check_shape`)
static int pq_encode_with(int (*check_shape)(int, int), const dprhot_bf16* vec, int64_t n, int dp, const dprhot_bf16* codebook, int dsub,
                          uint8_t* codes, void* stream) {
  REQUIRE(n >= 0 && n < (1ll << 40), "n=%lld out of range (0 .. 2^40 - 1)", (long long)n);
  REQUIRE(codebook != nullptr, "NULL pointer (codebook)");
  REQUIRE(n == 0 || (vec && codes), "NULL pointer (vec, codes)");
  if (int rc = check_shape(dp, dsub)) return rc;
  if (n == 0) return DPRHOT_OK;
  PqEncodeArgs a{reinterpret_cast<const uint16_t*>(vec), (long long)n, dp, reinterpret_cast<const uint16_t*>(codebook), codes};
  const long long want = (n + PQ_ENC_THREADS - 1) / PQ_ENC_THREADS;
  const dim3 grid((unsigned)(want < 65536 ? want : 65536), (unsigned)(dp / dsub)), block(PQ_ENC_THREADS);  // (rows beyond: grid stride)
  hipStream_t st = (hipStream_t)stream;
  if (dsub == 2) return launch<pq_encode_kernel<2>>(grid, block, 0, st, a);
  if (dsub == 4) return launch<pq_encode_kernel<4>>(grid, block, 0, st, a);
  return launch<pq_encode_kernel<8>>(grid, block, 0, st, a);
}

int dprhot_pq_encode(const dprhot_bf16* vec, int64_t n, int dp, const dprhot_bf16* codebook, int dsub, uint8_t* codes, void* stream) {
  return pq_encode_with(pq_check_shape, vec, n, dp, codebook, dsub, codes, stream);
}

int dprhot_ivf_pq_score(const uint8_t* post_code, const dprhot_bf16* codebook, int dsub, const int32_t* post_doc, const int64_t* exp_off,
                        int64_t n_postings, int n_experts, int dp, const dprhot_bf16* ent_vec, const int32_t* ent_q, int n_entries,
                        const int32_t* bexp, const int32_t* bexp_off, int n_bexp, int nq, int64_t doc_begin, int cols, float* S, int64_t ld,
                        void* stream) {
  if (int rc = ivf_pq_check_index(post_code, codebook, dsub, post_doc, exp_off, n_postings, n_experts, dp)) return rc;
  if (int rc = ivf_check_batch(nq, n_entries, n_bexp, ent_vec, ent_q, bexp, bexp_off)) return rc;
  if (int rc = check_score_window(S, cols, ld, doc_begin, 1ll << 31)) return rc;
  if (n_entries == 0 || n_postings == 0) return DPRHOT_OK;
  IvfPqArgs a{post_code, reinterpret_cast<const uint16_t*>(codebook), post_doc, reinterpret_cast<const long long*>(exp_off), n_experts,
              reinterpret_cast<const uint16_t*>(ent_vec), ent_q, bexp, bexp_off, n_bexp, nq, (long long)doc_begin, cols, S, (long long)ld};
  const unsigned blocks = (unsigned)cdiv(cdiv(cols, IVF_T), IVF_WAVES);
  hipStream_t st = (hipStream_t)stream;
  if (dsub == 2) return ivf_pq_launch<2>(dp, blocks, st, a);
  if (dsub == 4) return ivf_pq_launch<4>(dp, blocks, st, a);
  return ivf_pq_launch<8>(dp, blocks, st, a);
}

int dprhot_ivf_pq_search(const uint8_t* post_code, const dprhot_bf16* codebook, int dsub, const int32_t* post_doc, const int64_t* exp_off,
                         int64_t n_postings, int n_experts, int dp, const dprhot_bf16* ent_vec, const int32_t* ent_q, int n_entries,
                         const int32_t* bexp, const int32_t* bexp_off, int n_bexp, int nq, const dprhot_bf16* cls_q,
                         const dprhot_bf16* cls_doc, int dc, int64_t cls_rows, int64_t corpus_len, int64_t id_begin, int64_t id_end, int k,
                         int chunk, float* values, int64_t* indices, int first, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = ivf_pq_check_index(post_code, codebook, dsub, post_doc, exp_off, n_postings, n_experts, dp)) return rc;
  if (int rc = ivf_check_batch(nq, n_entries, n_bexp, ent_vec, ent_q, bexp, bexp_off)) return rc;
  auto score = [&](int64_t j0, int cols, float* S, int ld) {
    return dprhot_ivf_pq_score(post_code, codebook, dsub, post_doc, exp_off, n_postings, n_experts, dp, ent_vec, ent_q, n_entries, bexp,
                               bexp_off, n_bexp, nq, j0, cols, S, ld, stream);
  };
  return ivf_search_with(score, nq, cls_q, cls_doc, dc, cls_rows, corpus_len, id_begin, id_end, k, chunk, values, indices, first, workspace,
                         workspace_bytes, stream);
}

// ---- postings and query batches from encoder outputs (csrc/ivf_pack.h) ----
int dprhot_ivf_compact(const int32_t* expert_ids, const float* weights, const uint8_t* att, const int32_t* row_ids, int B, int L, int K,
                       int test_weight, float min_weight, int32_t* seq_off, int32_t* out_expert, int32_t* out_row, int32_t* out_slot,
                       float* out_weight, int64_t capacity, void* stream) {
  REQUIRE(K >= 1 && K <= 8, "K=%d out of range (1 .. 8)", K);
  REQUIRE(L >= 1, "L=%d: at least one token", L);
  REQUIRE(B >= 1 && B <= 65535, "B=%d out of range (1 .. 65535)", B);
  REQUIRE((long long)B * L * K < (1ll << 31), "B L K = %lld must stay below 2^31", (long long)B * L * K);
  REQUIRE(expert_ids && att && row_ids, "NULL pointer (expert_ids, att and row_ids are required)");
  REQUIRE(seq_off && out_expert && out_row && out_slot && out_weight, "NULL pointer (outputs)");
  REQUIRE(capacity >= 0, "capacity=%lld", (long long)capacity);
  IvfCompactArgs a{expert_ids, weights, att, row_ids, B, L, K, test_weight != 0, min_weight, seq_off, out_expert, out_row, out_slot,
                   out_weight, (long long)capacity};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(B, IVFP_WAVES)), block(64 * IVFP_WAVES);
  if (int rc = launch<ivf_count_kernel>(grid, block, 0, st, a)) return rc;
  if (int rc = launch<ivf_scan_kernel>(dim3(1), dim3(256), 0, st, seq_off, B)) return rc;
  return launch<ivf_emit_kernel>(grid, block, 0, st, a);
}

int dprhot_ivf_gather(const float* repr, int64_t repr_ld, int64_t n_rows, const float* weights, const int32_t* slot, const int64_t* perm,
                      int64_t n, int d, int K, int prod_round, int entry_round, int out_kind, void* out, int64_t out_ld, void* stream) {
  REQUIRE(d >= 1 && out_ld >= d && repr_ld >= d, "bad shape d=%d out_ld=%lld repr_ld=%lld", d, (long long)out_ld, (long long)repr_ld);
  REQUIRE(K >= 1 && K <= 8, "K=%d out of range (1 .. 8)", K);
  REQUIRE(n >= 0 && n < (1ll << 31), "n=%lld out of range (0 .. 2^31 - 1)", (long long)n);
  REQUIRE(n_rows >= 1, "n_rows=%lld", (long long)n_rows);
  REQUIRE(prod_round == IVFP_FP32 || prod_round == IVFP_BF16 || prod_round == IVFP_FP16, "unknown prod_round %d", prod_round);
  REQUIRE(entry_round == 0 || entry_round == 1, "unknown entry_round %d", entry_round);
  REQUIRE(out_kind == IVFP_FP32 || out_kind == IVFP_BF16, "unknown out_kind %d", out_kind);
  if (n == 0) return DPRHOT_OK;
  REQUIRE(repr && slot && out, "NULL pointer (repr, slot and out are required)");
  const long long blocks = (n * out_ld + 255) / 256;
  REQUIRE(blocks <= 0x7fffffffLL, "n=%lld rows of %lld columns: too many elements for one launch", (long long)n, (long long)out_ld);
  IvfGatherArgs a{repr, (long long)repr_ld, (long long)n_rows, weights, slot, reinterpret_cast<const long long*>(perm), (long long)n, d, K,
                  prod_round, entry_round, out, (long long)out_ld};
  if (out_kind == IVFP_BF16) return launch<ivf_gather_kernel<IVFP_BF16>>(dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return launch<ivf_gather_kernel<IVFP_FP32>>(dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
}

// ---- exhaustive ColBERT search (csrc/colbert.h) ----
static int cb_check(const void* tok, const void* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const void* q_tok, int nq, int LQ,
                    int pool) {
  REQUIRE(corpus_len > 0 && corpus_len < (1ll << 31), "corpus_len=%lld out of range (1 .. 2^31 - 1)", (long long)corpus_len);
  REQUIRE(n_blk >= 0 && n_blk < (1ll << 36), "n_blk=%lld out of range (< 2^36)", (long long)n_blk);
  REQUIRE(dp > 0 && dp % 32 == 0, "dp=%d must be a positive multiple of 32 (pad with zeros)", dp);
  REQUIRE(LQ >= 1 && LQ <= DPRHOT_MAXSIM_MAX_LEN, "LQ=%d out of range (1 .. %d)", LQ, DPRHOT_MAXSIM_MAX_LEN);
  REQUIRE(nq > 0, "bad shape nq=%d", nq);
  REQUIRE(pool == DPRHOT_POOL_SUM || pool == DPRHOT_POOL_MAX, "unknown pool %d", pool);
  REQUIRE(doc_blk && q_tok && (n_blk == 0 || tok), "NULL pointer (tok, doc_blk and q_tok are required)");
  REQUIRE(aligned16(tok) && aligned16(q_tok), "token rows must be 16-byte aligned");
  if (dp > CB_MAX_DP) return fail(DPRHOT_E_UNSUPPORTED, "dp=%d: the ColBERT search is built for dp <= %d", dp, CB_MAX_DP);
  return DPRHOT_OK;
}

int dprhot_colbert_workspace_bytes(int nq, int chunk, size_t* bytes) {
  REQUIRE(bytes != nullptr, "NULL out pointer");
  REQUIRE(nq > 0 && chunk > 0 && chunk % 8 == 0, "bad shape nq=%d chunk=%d (chunk: a positive multiple of 8)", nq, chunk);
  *bytes = chunk_ws_bytes(nq, chunk);
  return DPRHOT_OK;
}

int dprhot_colbert_score(const dprhot_bf16* tok, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok,
                         int nq, int LQ, int pool, int64_t doc_begin, int cols, float* S, int64_t ld, void* stream) {
  if (int rc = cb_check(tok, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool)) return rc;
  if (int rc = check_score_window(S, cols, ld, doc_begin, corpus_len)) return rc;
  const int FQ = cdiv(LQ, 16);
  const int QPW = FQ >= CB_FPP ? 1 : CB_FPP / FQ;  // whole queries per workgroup: QPW * FQ <= max(CB_FPP, FQ) <= CB_FMAX fragments
  const int rowb = dp * 2 + 16;
  const int TB = CB_TILE_BYTES / (16 * rowb);
  REQUIRE(cdiv(nq, QPW) <= 65535, "nq=%d: too many queries for one launch", nq);
  CbArgs a{reinterpret_cast<const uint16_t*>(tok), reinterpret_cast<const long long*>(doc_blk), (long long)n_blk, dp,
           reinterpret_cast<const uint16_t*>(q_tok), nq, LQ, pool, (long long)doc_begin, cols, S, (long long)ld, FQ, QPW, TB};
  const dim3 grid((unsigned)cdiv(cols, CB_RUNP), (unsigned)cdiv(nq, QPW)), block(256);
  const size_t lds = (size_t)TB * 16 * rowb + (size_t)CB_RUNP * (QPW * FQ * 16 + 1) * sizeof(float);  // the tile, then the term table
  hipStream_t st = (hipStream_t)stream;
  switch (dp) {
    case 32: return launch<cb_score_kernel<1>>(grid, block, lds, st, a);
    case 64: return launch<cb_score_kernel<2>>(grid, block, lds, st, a);
    case 96: return launch<cb_score_kernel<3>>(grid, block, lds, st, a);
    case 128: return launch<cb_score_kernel<4>>(grid, block, lds, st, a);
    default: return launch<cb_score_kernel<0>>(grid, block, lds, st, a);
  }
}

int dprhot_colbert_search(const dprhot_bf16* tok, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok,
                          int nq, int LQ, int pool, int64_t id_begin, int64_t id_end, int k, int chunk, float* values, int64_t* indices,
                          int first, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = cb_check(tok, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool)) return rc;
  auto fill = [&](int64_t j0, int cols, float* S, int ld) {
    return dprhot_colbert_score(tok, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool, j0, cols, S, ld, stream);
  };
  return topk_search_chunks("colbert", fill, nq, corpus_len, id_begin, id_end, k, chunk, values, indices, first, workspace, workspace_bytes,
                            stream);
}

// ---- MaxSim over candidate lists (csrc/colbert_cand.h) ----
static int cbc_check(const void* cand_off, const void* cand_doc, int64_t n_cand, int nq) {
  REQUIRE(n_cand >= 0 && n_cand < (1ll << 40), "n_cand=%lld out of range (< 2^40)", (long long)n_cand);
  REQUIRE(cand_off && (n_cand == 0 || cand_doc), "NULL pointer (cand_off and cand_doc are required)");
  REQUIRE(nq <= 65535, "nq=%d: too many queries for one launch", nq);
  return DPRHOT_OK;
}

int dprhot_colbert_cand_workspace_bytes(int nq, int chunk, size_t* bytes) { return dprhot_colbert_workspace_bytes(nq, chunk, bytes); }

int dprhot_colbert_cand_score(const dprhot_bf16* tok, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok,
                              int nq, int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t pos_begin,
                              int cols, float* S, int64_t ld, void* stream) {
  if (int rc = cb_check(tok, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool)) return rc;
  if (int rc = cbc_check(cand_off, cand_doc, n_cand, nq)) return rc;
  if (int rc = check_score_window(S, cols, ld, pos_begin, 1ll << 31)) return rc;  // candidate positions, not doc ids: below 2^31
  const int FQ = cdiv(LQ, 16);
  CbcArgs a{reinterpret_cast<const uint16_t*>(tok), reinterpret_cast<const long long*>(doc_blk), (long long)n_blk, (long long)corpus_len, dp,
            reinterpret_cast<const uint16_t*>(q_tok), nq, LQ, pool, reinterpret_cast<const long long*>(cand_off), cand_doc, (long long)n_cand,
            (long long)pos_begin, cols, S, (long long)ld, FQ};
  const dim3 grid((unsigned)cdiv(cols, CBC_RUNP), (unsigned)nq), block(256);
  const size_t lds = (size_t)CBC_RUNP * (FQ * 16 + 1) * sizeof(float);  // the term table
  hipStream_t st = (hipStream_t)stream;
  switch (dp) {
    case 32: return launch<cbc_score_kernel<1>>(grid, block, lds, st, a);
    case 64: return launch<cbc_score_kernel<2>>(grid, block, lds, st, a);
    case 96: return launch<cbc_score_kernel<3>>(grid, block, lds, st, a);
    case 128: return launch<cbc_score_kernel<4>>(grid, block, lds, st, a);
    default: return launch<cbc_score_kernel<0>>(grid, block, lds, st, a);
  }
}

extern "C++" {
// dprhot_colbert_cand_search and dprhot_colbert_cen_search behind their own checks: the chunk driver over candidate POSITIONS
// [0, max_count), fill(j0, cols, S, ld) scoring a window of them, then the one launch from positions to doc ids
template <class Fill>
static int cbc_search_with(const char* who, Fill fill, int nq, int64_t corpus_len, const int64_t* cand_off, const int32_t* cand_doc,
                           int64_t n_cand, int64_t max_count, int k, int chunk, float* values, int64_t* indices, void* workspace,
                           size_t workspace_bytes, void* stream) {
  REQUIRE(max_count > 0 && max_count < (1ll << 31), "max_count=%lld out of range (1 .. 2^31 - 1)", (long long)max_count);
  REQUIRE(k >= 1 && k <= corpus_len, "topk=%d out of range (1 .. corpus_len=%lld)", k, (long long)corpus_len);
  REQUIRE((long long)nq * k <= 0x7fffffffLL * 256, "nq=%d k=%d: too many result cells for one launch", nq, k);
  // the driver's id space is the longer of the corpus and the longest list
  if (int rc = topk_search_chunks(who, fill, nq, max_count > corpus_len ? max_count : corpus_len, 0, max_count, k, chunk, values, indices, 1,
                                  workspace, workspace_bytes, stream))
    return rc;
  const long long cells = (long long)nq * k;
  return launch<cbc_map_kernel>(dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                                reinterpret_cast<const long long*>(cand_off), cand_doc, (long long)n_cand, nq, k,
                                reinterpret_cast<long long*>(indices));
}
}  // extern "C++"

int dprhot_colbert_cand_search(const dprhot_bf16* tok, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok,
                               int nq, int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t max_count,
                               int k, int chunk, float* values, int64_t* indices, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = cb_check(tok, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool)) return rc;
  if (int rc = cbc_check(cand_off, cand_doc, n_cand, nq)) return rc;
  auto fill = [&](int64_t j0, int cols, float* S, int ld) {
    return dprhot_colbert_cand_score(tok, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool, cand_off, cand_doc, n_cand, j0, cols, S, ld,
                                     stream);
  };
  return cbc_search_with("colbert_cand", fill, nq, corpus_len, cand_off, cand_doc, n_cand, max_count, k, chunk, values, indices, workspace,
                         workspace_bytes, stream);
}

// ---- centroid interaction: approximate scores over candidate lists (csrc/colbert_cen.h) ----
static int cbi_check_query(int nq, int LQ, int C) {
  REQUIRE(LQ >= 1 && LQ <= DPRHOT_MAXSIM_MAX_LEN, "LQ=%d out of range (1 .. %d)", LQ, DPRHOT_MAXSIM_MAX_LEN);
  REQUIRE(C >= 1, "C=%d out of range (1 .. 2^31 - 1)", C);
  REQUIRE(nq > 0 && nq <= 65535, "bad shape nq=%d (1 .. 65535 queries in one launch)", nq);
  return DPRHOT_OK;
}

static int cbi_check(const void* doc_cen_off, const void* doc_cen, int64_t n_pairs, int64_t corpus_len, int C, const void* T, int nq, int LQ,
                     int pool) {
  REQUIRE(corpus_len > 0 && corpus_len < (1ll << 31), "corpus_len=%lld out of range (1 .. 2^31 - 1)", (long long)corpus_len);
  REQUIRE(n_pairs >= 0 && n_pairs < (1ll << 40), "n_pairs=%lld out of range (< 2^40)", (long long)n_pairs);
  if (int rc = cbi_check_query(nq, LQ, C)) return rc;
  REQUIRE(pool == DPRHOT_POOL_SUM || pool == DPRHOT_POOL_MAX, "unknown pool %d", pool);
  REQUIRE(doc_cen_off && T && (n_pairs == 0 || doc_cen), "NULL pointer (doc_cen_off, doc_cen and T are required)");
  REQUIRE(aligned16(T), "the centroid table must be 16-byte aligned");
  return DPRHOT_OK;
}

int dprhot_colbert_cen_table(const dprhot_bf16* centroids, int C, int dp, const dprhot_bf16* q_tok, int nq, int LQ, float* T, void* stream) {
  REQUIRE(dp > 0 && dp % 32 == 0, "dp=%d must be a positive multiple of 32 (pad with zeros)", dp);
  if (int rc = cbi_check_query(nq, LQ, C)) return rc;
  REQUIRE(centroids && q_tok && T, "NULL pointer (centroids, q_tok and T are required)");
  REQUIRE(aligned16(centroids) && aligned16(q_tok), "centroid and token rows must be 16-byte aligned");
  if (dp > CB_MAX_DP) return fail(DPRHOT_E_UNSUPPORTED, "dp=%d: the ColBERT search is built for dp <= %d", dp, CB_MAX_DP);
  CbiTableArgs a{reinterpret_cast<const uint16_t*>(centroids), C, dp, reinterpret_cast<const uint16_t*>(q_tok), nq, LQ, cdiv(LQ, 16), T};
  const dim3 grid((unsigned)(((long long)C + 63) / 64), (unsigned)nq), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (dp) {
    case 32: return launch<cbi_table_kernel<1>>(grid, block, 0, st, a);
    case 64: return launch<cbi_table_kernel<2>>(grid, block, 0, st, a);
    case 96: return launch<cbi_table_kernel<3>>(grid, block, 0, st, a);
    case 128: return launch<cbi_table_kernel<4>>(grid, block, 0, st, a);
    default: return launch<cbi_table_kernel<0>>(grid, block, 0, st, a);
  }
}

int dprhot_colbert_cen_workspace_bytes(int nq, int chunk, size_t* bytes) { return dprhot_colbert_workspace_bytes(nq, chunk, bytes); }

int dprhot_colbert_cen_score(const int64_t* doc_cen_off, const int32_t* doc_cen, int64_t n_pairs, int64_t corpus_len, int C, const float* T,
                             int nq, int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t pos_begin,
                             int cols, float* S, int64_t ld, void* stream) {
  if (int rc = cbi_check(doc_cen_off, doc_cen, n_pairs, corpus_len, C, T, nq, LQ, pool)) return rc;
  if (int rc = cbc_check(cand_off, cand_doc, n_cand, nq)) return rc;
  if (int rc = check_score_window(S, cols, ld, pos_begin, 1ll << 31)) return rc;  // candidate positions, not doc ids: below 2^31
  const int LT = cdiv(LQ, 16) * 16;
  CbiArgs a{reinterpret_cast<const long long*>(doc_cen_off), doc_cen, (long long)n_pairs, (long long)corpus_len, C, T, nq, LQ, pool,
            reinterpret_cast<const long long*>(cand_off), cand_doc, (long long)n_cand, (long long)pos_begin, cols, S, (long long)ld, LT};
  const dim3 grid((unsigned)cdiv(cols, CBC_RUNP), (unsigned)nq), block(256);
  const size_t lds = (size_t)CBC_RUNP * (LT + 1) * sizeof(float);  // the term table
  return launch<cbi_score_kernel>(grid, block, lds, (hipStream_t)stream, a);
}

int dprhot_colbert_cen_search(const int64_t* doc_cen_off, const int32_t* doc_cen, int64_t n_pairs, int64_t corpus_len, int C, const float* T,
                              int nq, int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t max_count,
                              int k, int chunk, float* values, int64_t* indices, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = cbi_check(doc_cen_off, doc_cen, n_pairs, corpus_len, C, T, nq, LQ, pool)) return rc;
  if (int rc = cbc_check(cand_off, cand_doc, n_cand, nq)) return rc;
  auto fill = [&](int64_t j0, int cols, float* S, int ld) {
    return dprhot_colbert_cen_score(doc_cen_off, doc_cen, n_pairs, corpus_len, C, T, nq, LQ, pool, cand_off, cand_doc, n_cand, j0, cols, S, ld,
                                    stream);
  };
  return cbc_search_with("colbert_cen", fill, nq, corpus_len, cand_off, cand_doc, n_cand, max_count, k, chunk, values, indices, workspace,
                         workspace_bytes, stream);
}

// ---- residual-compressed token index under the pruned search (csrc/colbert_res.h) ----
static int cbr_check_shape(int dp, int nbits, int C) {
  REQUIRE(nbits == 1 || nbits == 2 || nbits == 4, "nbits=%d: 1, 2 or 4 bits per feature", nbits);
  REQUIRE(C >= 1, "C=%d out of range (1 .. 2^31 - 1)", C);
  REQUIRE(dp > 0 && dp % 32 == 0, "dp=%d must be a positive multiple of 32 (pad with zeros)", dp);
  if (dp > CBR_MAX_DP) return fail(DPRHOT_E_UNSUPPORTED, "dp=%d: the residual ColBERT index is built for dp <= %d", dp, CBR_MAX_DP);
  return DPRHOT_OK;
}

static int cbr_check(const void* res_code, const void* tok_centroid, const void* centroids, int C, const void* weights, int nbits,
                     const void* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const void* q_tok, int nq, int LQ, int pool) {
  // the index's own limits first, so that a refusal names the residual index and its tensors
  if (int rc = cbr_check_shape(dp, nbits, C)) return rc;
  REQUIRE(n_blk <= 0 || (res_code && centroids && weights && tok_centroid),
          "NULL pointer (res_code, centroids, weights and tok_centroid are required)");
  REQUIRE(aligned16(res_code) && aligned16(centroids), "res_code and the centroid rows must be 16-byte aligned");
  return cb_check(res_code, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool);
}

int dprhot_colbert_res_encode(const dprhot_bf16* tok, const int32_t* tok_centroid, int64_t n_rows, int dp, const dprhot_bf16* centroids,
                              int C, const float* cutoffs, int nbits, uint8_t* res_code, void* stream) {
  REQUIRE(n_rows >= 0 && n_rows < (1ll << 40), "n_rows=%lld out of range (0 .. 2^40 - 1)", (long long)n_rows);
  if (int rc = cbr_check_shape(dp, nbits, C)) return rc;
  REQUIRE(n_rows == 0 || (tok && tok_centroid && centroids && cutoffs && res_code),
          "NULL pointer (tok, tok_centroid, centroids, cutoffs and res_code are required)");
  REQUIRE(aligned16(tok) && aligned16(centroids) && aligned16(res_code), "token rows, centroid rows and res_code must be 16-byte aligned");
  if (n_rows == 0) return DPRHOT_OK;
  CbrEncArgs a{reinterpret_cast<const uint16_t*>(tok), tok_centroid, (long long)n_rows, dp, reinterpret_cast<const uint16_t*>(centroids), C,
               cutoffs, res_code};
  const long long want = (n_rows * (dp / 8) + CBR_ENC_THREADS - 1) / CBR_ENC_THREADS;
  const dim3 grid((unsigned)(want < (1 << 20) ? want : (1 << 20))), block(CBR_ENC_THREADS);  // (pieces beyond: grid stride)
  hipStream_t st = (hipStream_t)stream;
  if (nbits == 1) return launch<cbr_encode_kernel<1>>(grid, block, 0, st, a);
  if (nbits == 2) return launch<cbr_encode_kernel<2>>(grid, block, 0, st, a);
  return launch<cbr_encode_kernel<4>>(grid, block, 0, st, a);
}

extern "C++" {
template <int NB>
static int cbr_launch(int dp, dim3 grid, size_t lds, hipStream_t st, const CbrArgs& a) {
  const dim3 block(256);
  switch (dp) {
    case 32: return launch<cbr_score_kernel<NB, 1>>(grid, block, lds, st, a);
    case 64: return launch<cbr_score_kernel<NB, 2>>(grid, block, lds, st, a);
    case 96: return launch<cbr_score_kernel<NB, 3>>(grid, block, lds, st, a);
    default: return launch<cbr_score_kernel<NB, 4>>(grid, block, lds, st, a);  // (dp = 128: cbr_check_shape)
  }
}
}  // extern "C++"

int dprhot_colbert_res_score(const uint8_t* res_code, const int32_t* tok_centroid, const dprhot_bf16* centroids, int C, const float* weights,
                             int nbits, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok, int nq,
                             int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t pos_begin, int cols,
                             float* S, int64_t ld, void* stream) {
  if (int rc = cbr_check(res_code, tok_centroid, centroids, C, weights, nbits, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool)) return rc;
  if (int rc = cbc_check(cand_off, cand_doc, n_cand, nq)) return rc;
  if (int rc = check_score_window(S, cols, ld, pos_begin, 1ll << 31)) return rc;  // candidate positions, not doc ids: below 2^31
  const int FQ = cdiv(LQ, 16);
  CbrArgs a{res_code, tok_centroid, reinterpret_cast<const uint16_t*>(centroids), C, weights, reinterpret_cast<const long long*>(doc_blk),
            (long long)n_blk, (long long)corpus_len, dp, reinterpret_cast<const uint16_t*>(q_tok), nq, LQ, pool,
            reinterpret_cast<const long long*>(cand_off), cand_doc, (long long)n_cand, (long long)pos_begin, cols, S, (long long)ld, FQ};
  const dim3 grid((unsigned)cdiv(cols, CBC_RUNP), (unsigned)nq);
  const size_t lds = (size_t)CBC_RUNP * (FQ * 16 + 1) * sizeof(float);  // the term table
  hipStream_t st = (hipStream_t)stream;
  if (nbits == 1) return cbr_launch<1>(dp, grid, lds, st, a);
  if (nbits == 2) return cbr_launch<2>(dp, grid, lds, st, a);
  return cbr_launch<4>(dp, grid, lds, st, a);
}

int dprhot_colbert_res_search(const uint8_t* res_code, const int32_t* tok_centroid, const dprhot_bf16* centroids, int C, const float* weights,
                              int nbits, const int64_t* doc_blk, int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok, int nq,
                              int LQ, int pool, const int64_t* cand_off, const int32_t* cand_doc, int64_t n_cand, int64_t max_count, int k,
                              int chunk, float* values, int64_t* indices, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = cbr_check(res_code, tok_centroid, centroids, C, weights, nbits, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool)) return rc;
  if (int rc = cbc_check(cand_off, cand_doc, n_cand, nq)) return rc;
  auto fill = [&](int64_t j0, int cols, float* S, int ld) {
    return dprhot_colbert_res_score(res_code, tok_centroid, centroids, C, weights, nbits, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool,
                                    cand_off, cand_doc, n_cand, j0, cols, S, ld, stream);
  };
  return cbc_search_with("colbert_res", fill, nq, corpus_len, cand_off, cand_doc, n_cand, max_count, k, chunk, values, indices, workspace,
                         workspace_bytes, stream);
}

// ---- product-quantised token index of the ColBERT search (csrc/colbert_pq.h) ----
static int cbpq_check_shape(int dp, int dsub) {
  REQUIRE(dsub == 2 || dsub == 4 || dsub == 8, "dsub=%d: sub-vectors of 2, 4 or 8 features", dsub);
  REQUIRE(dp > 0 && dp % 32 == 0, "dp=%d must be a positive multiple of 32 (pad with zeros)", dp);
  if (dp > CBPQ_MAX_DP) return fail(DPRHOT_E_UNSUPPORTED, "dp=%d: the product-quantised ColBERT index is built for dp <= %d", dp, CBPQ_MAX_DP);
  return DPRHOT_OK;
}

static int cbpq_check(const void* tok_code, const void* blk_rows, const void* codebook, int dsub, const void* doc_blk, int64_t n_blk,
                      int64_t corpus_len, int dp, const void* q_tok, int nq, int LQ, int pool) {
  if (int rc = cb_check(tok_code, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool)) return rc;
  REQUIRE(codebook != nullptr && (n_blk == 0 || blk_rows != nullptr), "NULL pointer (codebook and blk_rows are required)");
  REQUIRE(aligned16(codebook), "the codebook must be 16-byte aligned");
  return cbpq_check_shape(dp, dsub);
}

int dprhot_colbert_pq_encode(const dprhot_bf16* vec, int64_t n, int dp, const dprhot_bf16* codebook, int dsub, uint8_t* codes,
                             void* stream) {
  return pq_encode_with(cbpq_check_shape, vec, n, dp, codebook, dsub, codes, stream);
}

extern "C++" {
template <int DSUB>
static int cbpq_launch(int dp, dim3 grid, size_t lds, hipStream_t st, const CbPqArgs& a) {
  const dim3 block(CBPQ_THREADS);
  switch (dp) {
    case 32: return launch<cbpq_score_kernel<DSUB, 1>>(grid, block, lds, st, a);
    case 64: return launch<cbpq_score_kernel<DSUB, 2>>(grid, block, lds, st, a);
    case 96: return launch<cbpq_score_kernel<DSUB, 3>>(grid, block, lds, st, a);
    default: return launch<cbpq_score_kernel<DSUB, 4>>(grid, block, lds, st, a);  // (dp = 128: cbpq_check_shape)
  }
}
}  // extern "C++"

int dprhot_colbert_pq_score(const uint8_t* tok_code, const uint8_t* blk_rows, const dprhot_bf16* codebook, int dsub, const int64_t* doc_blk,
                            int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok, int nq, int LQ, int pool,
                            int64_t doc_begin, int cols, float* S, int64_t ld, void* stream) {
  if (int rc = cbpq_check(tok_code, blk_rows, codebook, dsub, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool)) return rc;
  if (int rc = check_score_window(S, cols, ld, doc_begin, corpus_len)) return rc;
  const int FQ = cdiv(LQ, 16);
  const int QPW = FQ >= CBPQ_FPP ? 1 : CBPQ_FPP / FQ;  // whole queries per workgroup: QPW * FQ <= CBPQ_FPP fragments, one pass
  const int blkb = 16 * (dp / dsub);
  const int TB = CBPQ_TILE_BYTES / blkb < CBPQ_TILE_BLOCKS ? CBPQ_TILE_BYTES / blkb : CBPQ_TILE_BLOCKS;
  const int gy = cdiv(nq, QPW);
  REQUIRE(gy <= 65535, "nq=%d: too many queries for one launch", nq);
  // the codebook, the code tile, the tile's row counts, then the term table
  const size_t lds = (size_t)dp * 512 + CBPQ_TILE_BYTES + CBPQ_TILE_BLOCKS + (size_t)CB_RUNP * (QPW * FQ * 16 + 1) * sizeof(float);
  if (lds + (CB_RUNP + 1) * sizeof(long long) > 160 * 1024)
    return fail(DPRHOT_E_UNSUPPORTED, "dp=%d LQ=%d needs %zu bytes of LDS", dp, LQ, lds);
  // runs per workgroup: one codebook load serves several runs once the grid fills the device a few times over
  const long long wgs = (long long)cdiv(cols, CB_RUNP) * gy;
  const int RPW = wgs / 1024 < 1 ? 1 : wgs / 1024 > CBPQ_MAX_RPW ? CBPQ_MAX_RPW : (int)(wgs / 1024);
  CbPqArgs a{tok_code, blk_rows, reinterpret_cast<const uint16_t*>(codebook), reinterpret_cast<const long long*>(doc_blk), (long long)n_blk,
             reinterpret_cast<const uint16_t*>(q_tok), nq, LQ, pool, (long long)doc_begin, cols, S, (long long)ld, FQ, QPW, TB, RPW};
  const dim3 grid((unsigned)cdiv(cdiv(cols, CB_RUNP), RPW), (unsigned)gy);
  hipStream_t st = (hipStream_t)stream;
  if (dsub == 2) return cbpq_launch<2>(dp, grid, lds, st, a);
  if (dsub == 4) return cbpq_launch<4>(dp, grid, lds, st, a);
  return cbpq_launch<8>(dp, grid, lds, st, a);
}

int dprhot_colbert_pq_search(const uint8_t* tok_code, const uint8_t* blk_rows, const dprhot_bf16* codebook, int dsub, const int64_t* doc_blk,
                             int64_t n_blk, int64_t corpus_len, int dp, const dprhot_bf16* q_tok, int nq, int LQ, int pool,
                             int64_t id_begin, int64_t id_end, int k, int chunk, float* values, int64_t* indices, int first,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = cbpq_check(tok_code, blk_rows, codebook, dsub, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool)) return rc;
  auto fill = [&](int64_t j0, int cols, float* S, int ld) {
    return dprhot_colbert_pq_score(tok_code, blk_rows, codebook, dsub, doc_blk, n_blk, corpus_len, dp, q_tok, nq, LQ, pool, j0, cols, S, ld,
                                   stream);
  };
  return topk_search_chunks("colbert_pq", fill, nq, corpus_len, id_begin, id_end, k, chunk, values, indices, first, workspace,
                            workspace_bytes, stream);
}


// ---- SPAR retrieval: two resident indexes, a grid of weights, one pass (csrc/spar.h) ----
static int spar_check(const void* Q1, const void* Q2, int nq, int d1, int d2, const void* C1, const void* C2, int64_t n_ctx, const float* lam,
                      int W) {
  REQUIRE(Q1 && Q2 && C1 && C2 && lam, "NULL pointer (Q1, Q2, C1, C2 and lam are required)");
  REQUIRE(aligned16(Q1) && aligned16(Q2) && aligned16(C1) && aligned16(C2), "operand rows must be 16-byte aligned");
  REQUIRE(d1 > 0 && d1 % 32 == 0 && d2 > 0 && d2 % 32 == 0, "d1=%d and d2=%d must be positive multiples of 32 (pad with zeros)", d1, d2);
  REQUIRE(W >= 1 && W <= SP_MAXW, "W=%d weights out of range (1 .. %d per call)", W, SP_MAXW);
  for (int w = 0; w < W; ++w) REQUIRE(lam[w] - lam[w] == 0.f, "weight %d of %d is not finite", w, W);
  REQUIRE(nq > 0 && (long long)W * nq < (1ll << 31) && nq <= 65535 * SP_B, "W * nq = %d * %d state rows out of range (1 .. 2^31 - 1)", W, nq);
  REQUIRE(n_ctx > 0 && n_ctx < (1ll << 31), "n_ctx=%lld out of range (1 .. 2^31 - 1)", (long long)n_ctx);
  return DPRHOT_OK;
}

// one launch of spar_kernel over passage ids j0 .. j0 + cols (checked by the callers)
static SparArgs spar_args(const dprhot_bf16* Q1, const dprhot_bf16* Q2, int nq, int d1, int d2, const dprhot_bf16* C1, const dprhot_bf16* C2,
                          const float* lam, int W, int64_t j0, int cols) {
  SparArgs a{};
  a.Q1 = reinterpret_cast<const uint16_t*>(Q1);
  a.Q2 = reinterpret_cast<const uint16_t*>(Q2);
  a.C1 = reinterpret_cast<const uint16_t*>(C1) + (size_t)j0 * d1;
  a.C2 = reinterpret_cast<const uint16_t*>(C2) + (size_t)j0 * d2;
  a.nq = nq; a.cols = cols; a.d1 = d1; a.d2 = d2; a.W = W;
  for (int w = 0; w < W; ++w) a.lam[w] = lam[w];
  return a;
}
static dim3 spar_grid(int nq, int cols) { return dim3((unsigned)cdiv(cols, SP_B), (unsigned)cdiv(nq, SP_B)); }

int dprhot_spar_workspace_bytes(int nq, int W, int chunk, size_t* bytes) {
  REQUIRE(bytes != nullptr, "NULL out pointer");
  REQUIRE(W >= 1 && W <= SP_MAXW, "W=%d weights out of range (1 .. %d per call)", W, SP_MAXW);
  REQUIRE(nq > 0 && (long long)W * nq < (1ll << 31), "W * nq = %d * %d state rows out of range (1 .. 2^31 - 1)", W, nq);
  REQUIRE(chunk > 0 && chunk % 8 == 0, "chunk=%d must be a positive multiple of 8", chunk);
  REQUIRE((long long)W * nq * chunk < (1ll << 40), "W * nq * chunk = %d * %d * %d candidate slots out of range (< 2^40)", W, nq, chunk);
  *bytes = search_ws_bytes(W * nq, chunk);
  return DPRHOT_OK;
}

int dprhot_spar_score(const dprhot_bf16* Q1, const dprhot_bf16* Q2, int nq, int d1, int d2, const dprhot_bf16* C1, const dprhot_bf16* C2,
                      int64_t n_ctx, const float* lam, int W, int64_t doc_begin, int cols, float* S, int64_t ld, void* stream) {
  if (int rc = spar_check(Q1, Q2, nq, d1, d2, C1, C2, n_ctx, lam, W)) return rc;
  if (int rc = check_score_window(S, cols, ld, doc_begin, n_ctx)) return rc;
  REQUIRE(ld % 8 == 0 && aligned16(S), "S must be 16-byte aligned with ld=%lld a multiple of 8", (long long)ld);
  SparArgs a = spar_args(Q1, Q2, nq, d1, d2, C1, C2, lam, W, doc_begin, cols);
  a.S = S;
  a.ld = (long long)ld;
  return launch<spar_kernel<false>>(spar_grid(nq, cols), dim3(256), 0, (hipStream_t)stream, a);
}

int dprhot_spar_search(const dprhot_bf16* Q1, const dprhot_bf16* Q2, int nq, int d1, int d2, const dprhot_bf16* C1, const dprhot_bf16* C2,
                       int64_t n_ctx, const float* lam, int W, int64_t id_begin, int64_t id_end, int k, int chunk, float* values,
                       int64_t* indices, int first, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = spar_check(Q1, Q2, nq, d1, d2, C1, C2, n_ctx, lam, W)) return rc;
  REQUIRE(values && indices, "NULL pointer");
  REQUIRE(k >= 1 && k <= n_ctx, "topk=%d out of range (1 .. n_ctx=%lld)", k, (long long)n_ctx);
  REQUIRE(0 <= id_begin && id_begin < id_end && id_end <= n_ctx, "bad passage-id range [%lld, %lld) of %lld", (long long)id_begin,
          (long long)id_end, (long long)n_ctx);
  REQUIRE(chunk > 0 && chunk % 8 == 0, "chunk=%d must be a positive multiple of 8", chunk);
  REQUIRE((long long)W * nq * chunk < (1ll << 40), "W * nq * chunk = %d * %d * %d candidate slots out of range (< 2^40)", W, nq, chunk);
  const int rows = W * nq;
  const bool wide = k > TK_KWIDE;
  const size_t need = search_ws_bytes(rows, chunk) + (wide ? wsel_ws_bytes(rows, k) : 0);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(DPRHOT_E_WORKSPACE, "spar_search needs %zu workspace bytes (dprhot_spar_workspace_bytes%s), got %zu", need,
                wide ? " + dprhot_topk_wide_workspace_bytes" : "", workspace_bytes);
  REQUIRE(aligned16(workspace), "workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (k > TK_KMAX) {  // beyond the candidate-list merge: every chunk materialised, the chunk driver's selection
    auto fill = [&](int64_t j0, int cols, float* S, int ld) {
      return dprhot_spar_score(Q1, Q2, nq, d1, d2, C1, C2, n_ctx, lam, W, j0, cols, S, ld, stream);
    };
    return topk_search_chunks("spar", fill, rows, n_ctx, id_begin, id_end, k, chunk, values, indices, first, workspace, workspace_bytes,
                              stream);
  }
  // the layout of dprhot_search for W * nq rows: scores of the first chunk / candidate values, candidate columns, candidate counts
  float* S = static_cast<float*>(workspace);
  int* cand_j = reinterpret_cast<int*>(static_cast<char*>(workspace) + (size_t)rows * chunk * 4);
  int* cnt = reinterpret_cast<int*>(static_cast<char*>(workspace) + (size_t)rows * chunk * 8);
  if (int rc = zero_words(cnt, (size_t)rows, st)) return rc;
  for (int64_t j0 = id_begin; j0 < id_end; j0 += chunk) {
    const int cols = (int)(id_end - j0 < chunk ? id_end - j0 : chunk);
    const int ld = (cols + 7) / 8 * 8;  // (<= chunk: chunk is a multiple of 8)
    SparArgs a = spar_args(Q1, Q2, nq, d1, d2, C1, C2, lam, W, j0, cols);
    if (first && j0 == id_begin) {  // nothing to filter against yet: materialise this chunk's scores and select from them
      a.S = S;
      a.ld = ld;
      if (int rc = launch<spar_kernel<false>>(spar_grid(nq, cols), dim3(256), 0, st, a)) return rc;
      if (int rc = dprhot_topk_update(S, rows, cols, ld, j0, k, values, indices, 1, stream)) return rc;
      continue;
    }
    // scores that cannot enter a row's top-k never leave the tile; at most `cols` candidates per row and chunk
    a.kth_val = values; a.kth_idx = indices; a.k = k; a.col_offset = (long long)j0;
    a.cnt = cnt; a.cand_v = S; a.cand_j = cand_j; a.ldc = ld;
    if (int rc = launch<spar_kernel<true>>(spar_grid(nq, cols), dim3(256), 0, st, a)) return rc;
    TopkArgs p{S, rows, cols, (long long)ld, (long long)j0, k, values, indices, 0, cand_j, cnt};
    if (int rc = launch_topk(p, rows, st)) return rc;
  }
  return DPRHOT_OK;
}

// ---- the fp8 dense index: e4m3fn rows, one power-of-two scale per row (csrc/dense_fp8.h) ----
int dprhot_fp8_encode(const void* rows, int is_bf16, int64_t n, int d, int dp, uint8_t* codes, float* scale, void* stream) {
  REQUIRE(rows && codes && scale, "NULL pointer (rows, codes and scale are required)");
  REQUIRE(aligned16(codes) && (reinterpret_cast<uintptr_t>(rows) & (is_bf16 ? 1u : 3u)) == 0 && (reinterpret_cast<uintptr_t>(scale) & 3u) == 0,
          "codes must be 16-byte aligned, rows and scale aligned to their elements");
  REQUIRE(dp > 0 && dp % 32 == 0, "dp=%d must be a positive multiple of 32", dp);
  REQUIRE(d > 0 && d <= dp, "d=%d out of range (1 .. dp=%d)", d, dp);
  REQUIRE(n > 0 && n < (1ll << 31), "n=%lld rows out of range (1 .. 2^31 - 1)", (long long)n);
  const dim3 grid((unsigned)((n + 3) / 4));
  if (is_bf16) return launch<fp8_encode_kernel<true>>(grid, dim3(256), 0, (hipStream_t)stream, rows, (long long)n, d, dp, codes, scale);
  return launch<fp8_encode_kernel<false>>(grid, dim3(256), 0, (hipStream_t)stream, rows, (long long)n, d, dp, codes, scale);
}

static int dfp8_check(const void* Qc, const void* qs, int nq, const void* Cc, const void* cs, int64_t n_ctx, int dp) {
  REQUIRE(Qc && qs && Cc && cs, "NULL pointer (Qc, qs, Cc and cs are required)");
  REQUIRE(aligned16(Qc) && aligned16(Cc), "code rows must be 16-byte aligned");
  REQUIRE((reinterpret_cast<uintptr_t>(qs) & 3u) == 0 && (reinterpret_cast<uintptr_t>(cs) & 3u) == 0, "scales must be 4-byte aligned");
  REQUIRE(dp > 0 && dp % 32 == 0, "dp=%d must be a positive multiple of 32 (pad with code 0)", dp);
  REQUIRE(nq > 0 && nq <= 65535 * F8_B, "nq=%d queries out of range (1 .. %d)", nq, 65535 * F8_B);
  REQUIRE(n_ctx > 0 && n_ctx < (1ll << 31), "n_ctx=%lld out of range (1 .. 2^31 - 1)", (long long)n_ctx);
  return DPRHOT_OK;
}

// one launch of dfp8_kernel over passage ids j0 .. j0 + cols (checked by the callers)
static Dfp8Args dfp8_args(const uint8_t* Qc, const float* qs, int nq, const uint8_t* Cc, const float* cs, int dp, int64_t j0, int cols) {
  Dfp8Args a{};
  a.Qc = Qc; a.qs = qs;
  a.Cc = Cc + (size_t)j0 * dp;
  a.cs = cs + j0;
  a.nq = nq; a.cols = cols; a.dp = dp;
  return a;
}
// at most F8_TM_SHORT queries: the short query tile (a score's bits do not depend on the tile)
extern "C++" {
template <bool FILTER>
static int dfp8_launch(const Dfp8Args& a, hipStream_t st) {
  if (a.nq <= F8_TM_SHORT) return launch<dfp8_kernel<FILTER, F8_TM_SHORT>>(dim3((unsigned)cdiv(a.cols, F8_B), 1), dim3(256), 0, st, a);
  return launch<dfp8_kernel<FILTER, F8_B>>(dim3((unsigned)cdiv(a.cols, F8_B), (unsigned)cdiv(a.nq, F8_B)), dim3(256), 0, st, a);
}
}  // extern "C++"

int dprhot_dense_fp8_workspace_bytes(int nq, int chunk, size_t* bytes) {
  REQUIRE(bytes != nullptr, "NULL out pointer");
  REQUIRE(nq > 0, "nq=%d queries out of range (1 .. 2^31 - 1)", nq);
  REQUIRE(chunk > 0 && chunk % 8 == 0, "chunk=%d must be a positive multiple of 8", chunk);
  REQUIRE((long long)nq * chunk < (1ll << 40), "nq * chunk = %d * %d candidate slots out of range (< 2^40)", nq, chunk);
  *bytes = search_ws_bytes(nq, chunk);
  return DPRHOT_OK;
}

int dprhot_dense_fp8_score(const uint8_t* Qc, const float* qs, int nq, const uint8_t* Cc, const float* cs, int64_t n_ctx, int dp,
                           int64_t doc_begin, int cols, float* S, int64_t ld, void* stream) {
  if (int rc = dfp8_check(Qc, qs, nq, Cc, cs, n_ctx, dp)) return rc;
  if (int rc = check_score_window(S, cols, ld, doc_begin, n_ctx)) return rc;
  REQUIRE(ld % 8 == 0 && aligned16(S), "S must be 16-byte aligned with ld=%lld a multiple of 8", (long long)ld);
  Dfp8Args a = dfp8_args(Qc, qs, nq, Cc, cs, dp, doc_begin, cols);
  a.S = S;
  a.ld = (long long)ld;
  return dfp8_launch<false>(a, (hipStream_t)stream);
}

int dprhot_dense_fp8_search(const uint8_t* Qc, const float* qs, int nq, const uint8_t* Cc, const float* cs, int64_t n_ctx, int dp,
                            int64_t id_begin, int64_t id_end, int k, int chunk, float* values, int64_t* indices, int first, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (int rc = dfp8_check(Qc, qs, nq, Cc, cs, n_ctx, dp)) return rc;
  REQUIRE(values && indices, "NULL pointer");
  REQUIRE(k >= 1 && k <= n_ctx, "topk=%d out of range (1 .. n_ctx=%lld)", k, (long long)n_ctx);
  REQUIRE(0 <= id_begin && id_begin < id_end && id_end <= n_ctx, "bad passage-id range [%lld, %lld) of %lld", (long long)id_begin,
          (long long)id_end, (long long)n_ctx);
  REQUIRE(chunk > 0 && chunk % 8 == 0, "chunk=%d must be a positive multiple of 8", chunk);
  REQUIRE((long long)nq * chunk < (1ll << 40), "nq * chunk = %d * %d candidate slots out of range (< 2^40)", nq, chunk);
  const bool wide = k > TK_KWIDE;
  const size_t need = search_ws_bytes(nq, chunk) + (wide ? wsel_ws_bytes(nq, k) : 0);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(DPRHOT_E_WORKSPACE, "dense_fp8_search needs %zu workspace bytes (dprhot_dense_fp8_workspace_bytes%s), got %zu", need,
                wide ? " + dprhot_topk_wide_workspace_bytes" : "", workspace_bytes);
  REQUIRE(aligned16(workspace), "workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (k > TK_KMAX) {  // beyond the candidate-list merge: every chunk materialised, the chunk driver's selection
    auto fill = [&](int64_t j0, int cols, float* S, int ld) {
      return dprhot_dense_fp8_score(Qc, qs, nq, Cc, cs, n_ctx, dp, j0, cols, S, ld, stream);
    };
    return topk_search_chunks("dense_fp8", fill, nq, n_ctx, id_begin, id_end, k, chunk, values, indices, first, workspace, workspace_bytes,
                              stream);
  }
  // the layout of dprhot_search: scores of the first chunk / candidate values, candidate columns, candidate counts
  float* S = static_cast<float*>(workspace);
  int* cand_j = reinterpret_cast<int*>(static_cast<char*>(workspace) + (size_t)nq * chunk * 4);
  int* cnt = reinterpret_cast<int*>(static_cast<char*>(workspace) + (size_t)nq * chunk * 8);
  if (int rc = zero_words(cnt, (size_t)nq, st)) return rc;
  for (int64_t j0 = id_begin; j0 < id_end; j0 += chunk) {
    const int cols = (int)(id_end - j0 < chunk ? id_end - j0 : chunk);
    const int ld = (cols + 7) / 8 * 8;  // (<= chunk: chunk is a multiple of 8)
    Dfp8Args a = dfp8_args(Qc, qs, nq, Cc, cs, dp, j0, cols);
    if (first && j0 == id_begin) {  // nothing to filter against yet: materialise this chunk's scores and select from them
      a.S = S;
      a.ld = ld;
      if (int rc = dfp8_launch<false>(a, st)) return rc;
      if (int rc = dprhot_topk_update(S, nq, cols, ld, j0, k, values, indices, 1, stream)) return rc;
      continue;
    }
    // scores that cannot enter a row's top-k never leave the tile; at most `cols` candidates per row and chunk
    a.kth_val = values; a.kth_idx = indices; a.k = k; a.col_offset = (long long)j0;
    a.cnt = cnt; a.cand_v = S; a.cand_j = cand_j; a.ldc = ld;
    if (int rc = dfp8_launch<true>(a, st)) return rc;
    TopkArgs p{S, nq, cols, (long long)ld, (long long)j0, k, values, indices, 0, cand_j, cnt};
    if (int rc = launch_topk(p, nq, st)) return rc;
  }
  return DPRHOT_OK;
}

}  // extern "C"

#include "colbert_union.h"  // the candidate stage of the pruned ColBERT search: kernels and the entry points of include/dprhot_union.h
