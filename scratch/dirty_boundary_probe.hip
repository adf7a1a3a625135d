// dirty_boundary_probe -- what does a kernel boundary pay for the bytes the kernel before it left dirty in the XCD L2s?  One graph of
// 100 (producer, consumer) pairs per arm.  Producer: 99 workgroups of 1024 threads (the batch-32 step's second launch's grid); the
// first 48 store as their last instructions, the rest return.  Consumer: one wave that loads one word of what the producer stored
// and stores it elsewhere (dependent, trivial).  Arms of the producer:
//   a   nothing
//   b   786 KB: each workgroup its 16-column stripe of a [256][768] fp32 matrix, each wave a 16 x 16 tile as the dC role stores it
//       today -- 4 bytes per lane, four instructions of 4 rows x 64 B, plain
//   c   the same tiles transposed: one instruction of 16 rows x 64 B, 16 bytes per lane, plain
//   d   as c through a buffer store with sc1 (write-through, the line leaves L2)
//   e   442 KB: 288 rows x 768 bf16 (Qb + Cb), six rows per workgroup, 4 bytes per lane in 64-byte row pieces, plain
//   e8  the same bytes as the copy waves store them today: 8 bytes per lane in 64-byte row pieces, plain
//   f   the same bytes, 16 bytes per lane, sc1
// Figures: us per pair (graph of 100 pairs, 20 replays per sample), the arms alternating over ROUNDS rounds, min / median / max.
// build: hipcc --offload-arch=gfx950 -O3 scratch/dirty_boundary_probe.hip -o scratch/dirty_boundary_probe
// run:   timeout -k 10 120 scratch/dirty_boundary_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>

enum { ARM_A, ARM_B, ARM_C, ARM_D, ARM_E, ARM_E8, ARM_F, N_ARMS };
static const char* const kName[N_ARMS] = {"a   nothing", "b   786 KB  4 B/lane plain", "c   786 KB 16 B/lane plain", "d   786 KB 16 B/lane sc1",
                                          "e   442 KB  4 B/lane plain", "e8  442 KB  8 B/lane plain", "f   442 KB 16 B/lane sc1"};
constexpr int ROWS = 256, D = 768, WRITERS = 48;              // fp32 matrix: 786432 bytes
constexpr int BROWS = 288, BROW_BYTES = D * 2;                // bf16 rows: 442368 bytes, 6 rows = 9216 bytes per writer
constexpr int MAT_BYTES = ROWS * D * 4, BF_BYTES = BROWS * BROW_BYTES;

template <int ARM>
__global__ __launch_bounds__(1024) void producer(float* __restrict__ mat, float seed) {
  const int wg = (int)blockIdx.x;
  if (wg >= WRITERS) return;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
  const float x = seed + (float)lane;
  if constexpr (ARM == ARM_B) {
    const int j0 = wave * 16, n0 = wg * 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) mat[(size_t)(j0 + g * 4 + r) * D + n0 + i] = x + (float)r;
  } else if constexpr (ARM == ARM_C) {
    const int j0 = wave * 16, n0 = wg * 16;
    *reinterpret_cast<float4*>(mat + (size_t)(j0 + i) * D + n0 + g * 4) = make_float4(x, x + 1.f, x + 2.f, x + 3.f);
  } else if constexpr (ARM == ARM_D) {
    const int j0 = wave * 16, n0 = wg * 16;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(mat, 0, MAT_BYTES, 0x00020000);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = {__float_as_uint(x), __float_as_uint(x + 1.f), __float_as_uint(x + 2.f), __float_as_uint(x + 3.f)};
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, ((j0 + i) * D + n0 + g * 4) * 4, 0, 16);
  } else if constexpr (ARM == ARM_E) {
    // 144 pieces of 64 B per workgroup (6 rows x 24), 16 lanes per piece, neighbouring pieces of one instruction in different rows
    char* const base = reinterpret_cast<char*>(mat) + (size_t)wg * 6 * BROW_BYTES;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int piece = (k * 16 + wave) * 4 + g;
      if (piece < 144) *reinterpret_cast<uint32_t*>(base + (piece % 6) * BROW_BYTES + (piece / 6) * 64 + i * 4) = __float_as_uint(x) + k;
    }
  } else if constexpr (ARM == ARM_E8) {
    // the same 144 pieces, 8 lanes per piece, 8 pieces per instruction
    char* const base = reinterpret_cast<char*>(mat) + (size_t)wg * 6 * BROW_BYTES;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int piece = (k * 16 + wave) * 8 + (lane >> 3);
      if (piece < 144) *reinterpret_cast<uint2*>(base + (piece % 6) * BROW_BYTES + (piece / 6) * 64 + (lane & 7) * 8) = make_uint2(__float_as_uint(x), k);
    }
  } else if constexpr (ARM == ARM_F) {
    // 16 bytes per lane, 4 lanes per 64-byte piece, 16 pieces per instruction: 9 waves cover the 144 pieces
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(mat, 0, BF_BYTES, 0x00020000);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = {__float_as_uint(x), 1u, 2u, 3u};
    const int piece = wave * 16 + (lane >> 2);
    if (piece < 144) __builtin_amdgcn_raw_buffer_store_b128(v, rs, wg * 6 * BROW_BYTES + (piece % 6) * BROW_BYTES + (piece / 6) * 64 + (lane & 3) * 16, 0, 16);
  }
}

__global__ __launch_bounds__(64) void consumer(const float* __restrict__ mat, float* __restrict__ out) {
  if (threadIdx.x == 0) out[0] = mat[0];
}

template <int ARM>
static void launch_pair(hipStream_t st, float* mat, float* out, int k) {
  hipLaunchKernelGGL(producer<ARM>, dim3(99), dim3(1024), 0, st, mat, (float)k);
  hipLaunchKernelGGL(consumer, dim3(1), dim3(64), 0, st, mat, out);
}

#define CHECK(x)                                                                   \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
  } while (0)

int main() {
  constexpr int PAIRS = 100, REPLAYS = 20, ROUNDS = 9;
  float *mat, *out;
  CHECK(hipMalloc(&mat, MAT_BYTES)); CHECK(hipMalloc(&out, 256));
  CHECK(hipMemset(mat, 0, MAT_BYTES)); CHECK(hipMemset(out, 0, 256));
  hipStream_t st; CHECK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  hipGraphExec_t ge[N_ARMS];
  for (int arm = 0; arm < N_ARMS; ++arm) {
    hipGraph_t gr;
    CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeGlobal));
    for (int k = 0; k < PAIRS; ++k) switch (arm) {
        case ARM_A: launch_pair<ARM_A>(st, mat, out, k); break;
        case ARM_B: launch_pair<ARM_B>(st, mat, out, k); break;
        case ARM_C: launch_pair<ARM_C>(st, mat, out, k); break;
        case ARM_D: launch_pair<ARM_D>(st, mat, out, k); break;
        case ARM_E: launch_pair<ARM_E>(st, mat, out, k); break;
        case ARM_E8: launch_pair<ARM_E8>(st, mat, out, k); break;
        default: launch_pair<ARM_F>(st, mat, out, k); break;
      }
    CHECK(hipStreamEndCapture(st, &gr));
    CHECK(hipGraphInstantiate(&ge[arm], gr, nullptr, nullptr, 0));
    CHECK(hipGraphDestroy(gr));
    for (int w = 0; w < 3; ++w) CHECK(hipGraphLaunch(ge[arm], st));
    CHECK(hipStreamSynchronize(st));
  }
  static float us[N_ARMS][ROUNDS];
  for (int round = 0; round < ROUNDS; ++round)
    for (int arm = 0; arm < N_ARMS; ++arm) {
      CHECK(hipGraphLaunch(ge[arm], st));
      CHECK(hipEventRecord(e0, st));
      for (int w = 0; w < REPLAYS; ++w) CHECK(hipGraphLaunch(ge[arm], st));
      CHECK(hipEventRecord(e1, st));
      CHECK(hipEventSynchronize(e1));
      float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
      us[arm][round] = ms * 1e3f / (PAIRS * REPLAYS);
    }
  printf("us per (producer, consumer) pair; graph of %d pairs, %d replays per sample, %d rounds, arms alternating\n", PAIRS, REPLAYS, ROUNDS);
  printf("%-30s %8s %8s %8s\n", "arm", "min", "median", "max");
  float med[N_ARMS], mn[N_ARMS];
  for (int arm = 0; arm < N_ARMS; ++arm) {
    std::sort(us[arm], us[arm] + ROUNDS);
    mn[arm] = us[arm][0]; med[arm] = us[arm][ROUNDS / 2];
    printf("%-30s %8.3f %8.3f %8.3f\n", kName[arm], us[arm][0], med[arm], us[arm][ROUNDS - 1]);
  }
  printf("gate (medians): (b - d) + (e - f)  = %+.3f %+.3f = %+.3f us   [copies as stored today: (e8 - f) = %+.3f]\n", med[ARM_B] - med[ARM_D],
         med[ARM_E] - med[ARM_F], med[ARM_B] - med[ARM_D] + med[ARM_E] - med[ARM_F], med[ARM_E8] - med[ARM_F]);
  printf("gate (minima):  (b - d) + (e - f)  = %+.3f %+.3f = %+.3f us   [copies as stored today: (e8 - f) = %+.3f]\n", mn[ARM_B] - mn[ARM_D],
         mn[ARM_E] - mn[ARM_F], mn[ARM_B] - mn[ARM_D] + mn[ARM_E] - mn[ARM_F], mn[ARM_E8] - mn[ARM_F]);
  for (int arm = 0; arm < N_ARMS; ++arm) CHECK(hipGraphExecDestroy(ge[arm]));
  return 0;
}
