// sim_small.h -- the similarity launch of the latency-bound training step (B <= 32 query rows, fp32 q, K-major operands,
// split-K slabs of partial logits: fwd_plan's short rows on tile 5) without the GEMM engine's machinery.
//
// At these shapes every workgroup of gemm_tile has ONE K step: its double buffer, its register stages, the hop of both operands
// through a workgroup-shared LDS image and the two barriers around it serve a loop that runs once, on 24 of 256 CUs.  Here one
// wave owns one 16 x 16 output tile of one 256-deep K chunk and shares nothing: no barrier, no workgroup-shared LDS, 96 waves at
// 32 x 256 x 768 instead of 24 workgroups, all of their first (and only) trips to memory side by side.
//
// Arithmetic is the engine's bit for bit: the same v_cvt_pk_bf16_f32 of both operands, the same v_mfma_f32_16x16x32_bf16 with
// the operand placement of load_frag<..., KMAJOR> (lane (g, i) holds row / column i, k = kk * 32 + g * 8 .. + 7), kk ascending
// inside the chunk into one accumulator, chunks never split between waves.  The slabs, Qb and Cb hold the bits the engine writes.
//
// How fp32 reaches the fragment registers (FORM), both kept for the A/B (option small_sim; step of 32 x 256 x 768 on the ten-step
// graph, engine 9.19 us):
//   SS_PATCH whole-line loads (8 rows x 128 B per instruction) rounded into a WAVE-PRIVATE bf16 patch in LDS (the engine's
//            BK = 256 swizzle), then the wave's own fragment reads: program order within the wave is all the synchronisation.
//            8.29 us: the form the launch takes.
//   SS_REG   straight to registers in fragment shape: each lane loads its own 32 contiguous bytes per kk (2 x dwordx4).  No LDS
//            at all, but an instruction touches 16 lines and half of each: 8.52 us.
// One wave per workgroup; two (the two row tiles of one column tile and chunk) measured 8.70 / 9.41 us.
// Every load of the chunk is issued back to back before anything looks at a loaded value; the waits the compiler places are then
// counted vmcnt(N) in issue order (plain loads: hipcc counts them itself), so the conversions and the MFMA chain follow the data in.
// The front -- what a lone wave per CU executes before its first operand load, at full issue latency per instruction -- is kept
// short: the tile comes from a three-dimensional block index (no division, no early return), everything the operand addresses
// are made of sits in the first 64 bytes of the kernel arguments behind ONE wait, and the mask byte, which only the epilogue looks
// at, is loaded behind the 32 operand loads (first global_load_dwordx4: instruction 45, about 195 before; step of 32 x 256 x 768
// on the ten-step graph 7.21 -> 7.05 us, profiles/step_fronts_ab.txt; asserted on the assembly by tests/test_step_fronts.py).
#pragma once
#include "gemm_bf16.h"

namespace dprhot {

constexpr int SS_REG = 1, SS_PATCH = 2;
constexpr int SMS_KC = 256;         // K chunk of a wave (tile 5's BK): 8 MFMA steps
constexpr int SMS_KK = SMS_KC / 32;
constexpr int SMS_MAXW = 2;         // most waves per workgroup
constexpr int SMS_PATCH = 16 * SMS_KC;  // bf16 elements of one operand's patch [16 rows][256 k]

inline size_t sim_small_lds(int form, bool b_f32, int wpg) {
  return form == SS_PATCH ? (size_t)wpg * SMS_PATCH * 2 * (b_f32 ? 2 : 1) : 0;
}

typedef uint32_t sms_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 sms_round(const float4& a, const float4& b) {
  const uint4 v = make_uint4(cvt_pk_bf16(a.x, a.y), cvt_pk_bf16(a.z, a.w), cvt_pk_bf16(b.x, b.y), cvt_pk_bf16(b.z, b.w));
  return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ void sms_patch_store(const float4 (&raw)[2 * SMS_KK], uint16_t* T, int lane) {
#pragma unroll
  for (int j = 0; j < 2 * SMS_KK; ++j) {
    const int row = (j & 1) * 8 + (lane >> 3), ch = (j >> 1) * 4 + ((lane & 7) >> 1);  // 16-byte chunk of the row
    const uint2 v = make_uint2(cvt_pk_bf16(raw[j].x, raw[j].y), cvt_pk_bf16(raw[j].z, raw[j].w));
    *reinterpret_cast<uint2*>(T + row * SMS_KC + kswz<SMS_KC>(row, ch) * 8 + (lane & 1) * 4) = v;
  }
}
__device__ __forceinline__ bf16x8 sms_patch_frag(const uint16_t* T, int kk, int lane) {
  const int i = lane & 15, g = lane >> 4;
  return *reinterpret_cast<const bf16x8*>(T + i * SMS_KC + kswz<SMS_KC>(i, kk * 4 + g) * 8);
}

// p.kchunk == SMS_KC and p.K % SMS_KC == 0 (the launch guard): every chunk is whole, nothing lies beyond K.
// The grid is three-dimensional and exact: blockIdx.x = row tile (times wpg waves: the waves of one workgroup are neighbouring row
// tiles of one column tile and chunk, and read the same context rows), .y = column tile, .z = K chunk.  x runs fastest in dispatch
// order, so waves start in the order the linear index gave them (row tile, then column tile, then chunk) -- but the three indices
// cost no division (three v_rcp_iflag sequences stood in front of the first load) and no early return: a wave beyond the last row
// tile (wpg = 2 at an odd number of row tiles) loads clamped rows and stores nothing, as a ragged tile's rows beyond M do.
// wpg is the first argument, in the 64 bytes of the kernel arguments that hold everything the operand addresses are made of.
//
// sms_tile is one wave's whole life, shared by the two kernels below.  COPIES: the wave also writes the bf16 copies the backward reads
// (Qb by the waves of column tile 0, Cb by those of row tile 0); without, they are sim_small_split_kernel's copy waves' to write.
template <bool B_F32, int FORM, bool COPIES>
__device__ __forceinline__ void sms_tile(uint16_t* sms_smem, int wave, int rt, int ct, int bz, const GemmArgs& p, const EpiSim& epi) {
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int m0 = rt * 16, n0 = ct * 16, kbeg = bz * SMS_KC;
  DPRHOT_TM(0);

  // ---- every global read, back to back: the chunk of both operands, then the mask byte
  const float* const Af = reinterpret_cast<const float*>(p.A);
  const int arow = min(m0 + i, p.M - 1), brow = min(n0 + i, p.N - 1);
  bf16x8 af[SMS_KK], bfr[SMS_KK];
  float4 araw[2 * SMS_KK], braw[2 * SMS_KK];
  const float* const Bf = reinterpret_cast<const float*>(p.B);
  if constexpr (FORM == SS_REG) {
    // lane (g, i): its own 8 floats of row i per kk (2 x 16 bytes); a and b of one kk next to each other, kk ascending
    const float* const ap = Af + (size_t)arow * p.lda + kbeg + g * 8;
    const float* const bp = Bf + (size_t)brow * p.ldb + kbeg + g * 8;
#pragma unroll
    for (int kk = 0; kk < SMS_KK; ++kk) {
      araw[2 * kk] = *reinterpret_cast<const float4*>(ap + kk * 32);
      araw[2 * kk + 1] = *reinterpret_cast<const float4*>(ap + kk * 32 + 4);
      if constexpr (B_F32) {
        braw[2 * kk] = *reinterpret_cast<const float4*>(bp + kk * 32);
        braw[2 * kk + 1] = *reinterpret_cast<const float4*>(bp + kk * 32 + 4);
      }
    }
  } else {
    // whole lines: instruction j covers rows (j & 1) * 8 + (lane >> 3) of k line j >> 1 (32 floats = one kk), lane & 7 = 16-byte piece
    const int ar0 = min(m0 + (lane >> 3), p.M - 1), ar1 = min(m0 + 8 + (lane >> 3), p.M - 1);
    const int br0 = min(n0 + (lane >> 3), p.N - 1), br1 = min(n0 + 8 + (lane >> 3), p.N - 1);
    const float* const ap[2] = {Af + (size_t)ar0 * p.lda + kbeg + (lane & 7) * 4, Af + (size_t)ar1 * p.lda + kbeg + (lane & 7) * 4};
    const float* const bp[2] = {Bf + (size_t)br0 * p.ldb + kbeg + (lane & 7) * 4, Bf + (size_t)br1 * p.ldb + kbeg + (lane & 7) * 4};
#pragma unroll
    for (int j = 0; j < 2 * SMS_KK; ++j) {
      araw[j] = *reinterpret_cast<const float4*>(ap[j & 1] + (j >> 1) * 32);
      if constexpr (B_F32) braw[j] = *reinterpret_cast<const float4*>(bp[j & 1] + (j >> 1) * 32);
    }
  }
  if constexpr (!B_F32) {  // gathered bf16 contexts: the fragments as they lie in memory
#pragma unroll
    for (int kk = 0; kk < SMS_KK; ++kk) bfr[kk] = *reinterpret_cast<const bf16x8*>(p.B + (size_t)brow * p.ldb + kbeg + kk * 32 + g * 8);
  }
  __builtin_amdgcn_sched_barrier(0);  // the operand loads are out before the mask byte's address is worked out
  // The mask byte: one unconditional load -- of the operand's first byte where there is no mask, dropped by the select below -- so
  // that the text up to the first use of a loaded value is one basic block.  It is the LAST load issued and only the epilogue looks
  // at it; loads return in order, so the wait it needs is the one the last operand load needs anyway.
  const int ncl = min(n0 + i, epi.N - 1);
  const bool has_mask = epi.packed != nullptr || epi.colmask != nullptr;
  const uint8_t* mptr = epi.colmask != nullptr ? epi.colmask + ncl : reinterpret_cast<const uint8_t*>(p.A);
  if (epi.packed != nullptr) {  // (EpiSim::mask_raw)
    const int r = ncl / epi.p_rows_c, j = ncl - r * epi.p_rows_c;
    mptr = epi.packed + (size_t)(r * epi.p_rows_c + epi.p_n_ctx) * epi.p_row_bytes + min(j, epi.p_n_ctx - 1);
  }
  const uint8_t mbyte = *mptr;
  __builtin_amdgcn_sched_barrier(0);  // nothing above uses a loaded value
  DPRHOT_TM(1);

  // what masks the column besides the byte, worked out under the loads (no `||` on the byte: a branch on it would wait for all 33)
  const bool mpad = (n0 + i >= epi.N) | epi.mask_pad(ncl);
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (FORM == SS_REG) {
#pragma unroll
    for (int kk = 0; kk < SMS_KK; ++kk) {
      af[kk] = sms_round(araw[2 * kk], araw[2 * kk + 1]);
      if constexpr (B_F32) bfr[kk] = sms_round(braw[2 * kk], braw[2 * kk + 1]);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], bfr[kk], acc, 0, 0, 0);
    }
  } else {
    uint16_t* const Ta = sms_smem + wave * (SMS_PATCH * (B_F32 ? 2 : 1));
    uint16_t* const Tb = Ta + SMS_PATCH;
    sms_patch_store(araw, Ta, lane);
    if constexpr (B_F32) sms_patch_store(braw, Tb, lane);
    // (wave-private patch: the wave's own reads follow its own writes in program order)
#pragma unroll
    for (int kk = 0; kk < SMS_KK; ++kk) {
      af[kk] = sms_patch_frag(Ta, kk, lane);
      if constexpr (B_F32) bfr[kk] = sms_patch_frag(Tb, kk, lane);
    }
#pragma unroll
    for (int kk = 0; kk < SMS_KK; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], bfr[kk], acc, 0, 0, 0);
  }
  // The mask byte is the load behind the last operand load, and that one the MFMA chain has already waited for.  Its counter is
  // settled HERE all the same (vmcnt(0), the other counters left alone: the one wait in this file that the compiler did not place):
  // the compiler waits where the byte is first looked at, below the copies' conditional stores, and as the same counter counts
  // stores, the slab stores of half the waves would wait for their copies to be acknowledged.
  // (Without the copies nothing stands between the chain and the slab stores but the header words' store of ONE wave, which is
  // moved behind them: the compiler's own wait for the byte is then the chain's.)
  if constexpr (COPIES) __builtin_amdgcn_s_waitcnt(0x0F70);
  DPRHOT_TM(4);

  // ---- the bf16 copies the backward reads: each operand row by exactly one wave per chunk (16-byte pieces, 16 rows x 64 B each)
  if constexpr (COPIES) {
    if (p.Acopy != nullptr && ct == 0 && m0 + i < p.M) {
#pragma unroll
      for (int kk = 0; kk < SMS_KK; ++kk)
        *reinterpret_cast<bf16x8*>(p.Acopy + (size_t)(m0 + i) * p.lda + kbeg + kk * 32 + g * 8) = af[kk];
    }
    if constexpr (B_F32) {
      if (p.Bcopy != nullptr && rt == 0 && n0 + i < p.N) {
#pragma unroll
        for (int kk = 0; kk < SMS_KK; ++kk)
          *reinterpret_cast<bf16x8*>(p.Bcopy + (size_t)(n0 + i) * p.ldb + kbeg + kk * 32 + g * 8) = bfr[kk];
      }
    }
    if (epi.zero_words != nullptr && (rt | ct | bz) == 0 && lane < epi.n_zero) epi.zero_words[lane] = 0ull;
  }

  // ---- EpiSim::finish in its slab form (statistics off): * 1/T, masked columns -> -inf, fp32 partial logits of this chunk
  float* const S = epi.S + (size_t)bz * epi.slab_stride;
  const bool masked = mpad | (has_mask & (mbyte != 0));
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + g * 4 + r;
    const float v = masked ? -INFINITY : acc[r] * epi.inv_T;
    if (m < epi.M && n0 + i < epi.N) S[(size_t)m * epi.N + n0 + i] = v;
  }
  if constexpr (!COPIES) {
    if (epi.zero_words != nullptr && (rt | ct | bz) == 0 && lane < epi.n_zero) epi.zero_words[lane] = 0ull;
  }
  DPRHOT_TM(6);
}

template <bool B_F32, int FORM>
__global__ __launch_bounds__(64 * SMS_MAXW) void sim_small_kernel(int wpg, GemmArgs p, EpiSim epi) {
  extern __shared__ __attribute__((aligned(16))) uint16_t sms_smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  sms_tile<B_F32, FORM, true>(sms_smem, wave, (int)blockIdx.x * wpg + wave, (int)blockIdx.y, (int)blockIdx.z, p, epi);
}

// The same launch with the bf16 copies on waves of their own (option small_sim_copy; SS_PATCH, one wave per workgroup).  The grid is
// (row tiles, column tiles, splits + copy layers): the waves of the first `splits` z layers are sms_tile without its copies; behind
// them in dispatch order, `splits` (or 2 x splits, where one layer of the grid has fewer waves than there are operand tiles: one row
// tile or one column tile) layers of copy waves.  A copy wave takes 16 rows of one 256-deep chunk of ONE operand: z - splits is the
// chunk (a second layer: + splits), id = (layer * column tiles + y) * row tiles + x the unit, C tiles first, then Q tiles, the rest
// return at once.  It loads whole lines as sms_tile does (instruction j: rows (j & 1) * 8 + lane / 8 of line j / 2), all 16 loads
// before the first use, rounds its four floats with the same v_cvt_pk_bf16_f32 pairing (x, y), (z, w) -- the words of Qb / Cb are
// the ones sms_tile's fragments hold -- and stores them as one 8-byte piece: 8 rows x 64 contiguous bytes per instruction.  Rows
// beyond the operand are loaded clamped and not stored.  No LDS hop, no fragment reads, no MFMA chain, half the bytes: on a CU of
// its own such a wave ends before the compute waves do, and these no longer carry 8 (16) stores between their chain and their slab.
// Everything either role's addresses are made of is in the first 64 bytes of the kernel arguments (`splits` in wpg's place).
// WT (option small_sim_copy = 1; 2 keeps the 8-byte plain stores for the A/B): the same words leave as 16-byte WRITE-THROUGH stores.  A kernel's end writes back what its stores left dirty
// in the XCD L2s, behind the last wave (profiles/dirty_boundary_probe.txt: the copies' 442 KB cost the boundary 0.2 us); an sc1
// store goes through and leaves no dirty line, and at 16 bytes per lane it costs what a plain one does -- at 8 bytes 2.7 x.  Nothing
// re-reads Qb / Cb in front of the next boundary.  A lane holds 8 bytes of row r0 and 8 of row r0 + 8 per kk; lanes 2m and 2m + 1
// (neighbouring 8-byte pieces of both rows) exchange one of them by DPP quad_perm [1, 0, 3, 2]: the even lane then owns 16 contiguous
// bytes of row r0, the odd lane 16 of row r0 + 8 -- eight stores per lane instead of sixteen, 16 rows x 64 B per instruction.
template <bool B_F32, int WT = 0>
__device__ __forceinline__ void sms_copy_wave(int zc, int splits, const GemmArgs& p) {
  DPRHOT_TM(0);
  const int lane = threadIdx.x & 63;
  const int nrt = (p.M + 15) >> 4, nct = (p.N + 15) >> 4;
  const int layer = zc >= splits ? 1 : 0, kbeg = (zc - layer * splits) * SMS_KC;
  const int id = (layer * nct + (int)blockIdx.y) * nrt + (int)blockIdx.x;
  const int ncu = B_F32 && p.Bcopy != nullptr ? nct : 0, nqu = p.Acopy != nullptr ? nrt : 0;
  if (id >= ncu + nqu) return;
  const bool is_c = id < ncu;
  const float* const src = reinterpret_cast<const float*>(is_c ? p.B : p.A);
  uint16_t* const dst = is_c ? p.Bcopy : p.Acopy;
  const int rows = is_c ? p.N : p.M, ld = is_c ? p.ldb : p.lda, r0 = (is_c ? id : id - ncu) * 16 + (lane >> 3);
  const float* const sp[2] = {src + (size_t)min(r0, rows - 1) * ld + kbeg + (lane & 7) * 4, src + (size_t)min(r0 + 8, rows - 1) * ld + kbeg + (lane & 7) * 4};
  float4 raw[2 * SMS_KK];
#pragma unroll
  for (int j = 0; j < 2 * SMS_KK; ++j) raw[j] = *reinterpret_cast<const float4*>(sp[j & 1] + (j >> 1) * 32);
  __builtin_amdgcn_sched_barrier(0);  // every load is out before anything looks at a loaded value
  DPRHOT_TM(1);
  // All sixteen are waited for in ONE place, in front of the predicated stores (the last store needs the last load anyway).  The
  // compiler lays this role's text in front of the compute role's and counts what may be in flight where the two join: with its own
  // waits inside the predicated blocks, a path around them leaves loads in flight, and the compute role's front gets waits on vmcnt.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  uint2 v[2 * SMS_KK];
#pragma unroll
  for (int j = 0; j < 2 * SMS_KK; ++j) v[j] = make_uint2(cvt_pk_bf16(raw[j].x, raw[j].y), cvt_pk_bf16(raw[j].z, raw[j].w));
  if constexpr (WT != 0) {
    const bool odd = (lane & 1) != 0;
    const int myrow = r0 + (odd ? 8 : 0);
    // (the descriptor ends with the operand's last row: the range check would drop a row beyond it even without the predicate)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(dst, 0, rows * ld * 2, 0x00020000);
    const int off = (myrow * ld + kbeg + ((lane & 7) - (odd ? 1 : 0)) * 4) * 2;
    sms_u32x4 w[SMS_KK];
#pragma unroll
    for (int kk = 0; kk < SMS_KK; ++kk) {
      const uint2 mine = odd ? v[2 * kk + 1] : v[2 * kk], give = odd ? v[2 * kk] : v[2 * kk + 1];
      const uint2 got = make_uint2((uint32_t)__builtin_amdgcn_update_dpp(0, (int)give.x, 0xB1, 0xF, 0xF, false),
                                   (uint32_t)__builtin_amdgcn_update_dpp(0, (int)give.y, 0xB1, 0xF, 0xF, false));
      w[kk] = odd ? sms_u32x4{got.x, got.y, mine.x, mine.y} : sms_u32x4{mine.x, mine.y, got.x, got.y};
    }
    if (myrow < rows) {
#pragma unroll
      for (int kk = 0; kk < SMS_KK; ++kk) __builtin_amdgcn_raw_buffer_store_b128(w[kk], rs, off + kk * 64, 0, 16);  // aux 16: sc1
    }
  } else {
    // (two predicates for sixteen stores: a lane's second row is inside the operand only if its first one is)
    if (r0 < rows) {
      uint16_t* const dp = dst + (size_t)r0 * ld + kbeg + (lane & 7) * 4;
#pragma unroll
      for (int kk = 0; kk < SMS_KK; ++kk) *reinterpret_cast<uint2*>(dp + kk * 32) = v[2 * kk];
      if (r0 + 8 < rows) {
#pragma unroll
        for (int kk = 0; kk < SMS_KK; ++kk) *reinterpret_cast<uint2*>(dp + (size_t)8 * ld + kk * 32) = v[2 * kk + 1];
      }
    }
  }
  DPRHOT_TM(6);
}

template <bool B_F32, int WT = 0>
__global__ __launch_bounds__(64) void sim_small_split_kernel(int splits, GemmArgs p, EpiSim epi) {
  extern __shared__ __attribute__((aligned(16))) uint16_t sms_smem[];
  const int bz = (int)blockIdx.z;
  if (bz < splits)
    sms_tile<B_F32, SS_PATCH, false>(sms_smem, 0, (int)blockIdx.x, (int)blockIdx.y, bz, p, epi);
  else
    sms_copy_wave<B_F32, WT>(bz - splits, splits, p);
}

}  // namespace dprhot
