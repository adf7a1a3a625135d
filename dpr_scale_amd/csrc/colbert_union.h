// colbert_union.h -- the candidate stage of the pruned ColBERT search (include/dprhot_union.h has the contract):
// per query the sorted, duplicate-free union of the inverted lists its live tokens probe, without a sort.  Included at the end of
// dprhot.hip: the entry points below use that file's fail / REQUIRE / launch.
//
// State   in the workspace, per query: a bitmap of corpus_len bits, padded to whole blocks of UN_BLK_WORDS 32-bit words (8192 doc ids),
//         then one int32 per block.  Bit (doc & 31) of word (doc >> 5) is "doc is in the set".
// Count   four launches, each needing all of the one before:
//   un_clear_kernel   zeroes the bitmaps (16-byte stores) -- the workspace arrives with anything in it
//   un_mark_kernel    one wave per (query, token, probe): is the token live, is the id in [0, C), then the list in strides of 64 entries,
//                     4-byte loads side by side, one no-return atomicOr per doc id in [0, corpus_len).  A centroid two tokens name is
//                     marked twice; OR is idempotent, so no order of arrival changes a bit
//   un_count_kernel   one workgroup per query: its 16 waves take the query's blocks in turn (a wave popcounts a block from one 16-byte
//                     load per lane), then the workgroup turns the block counts into exclusive prefixes in place and notes the set size
//   un_offsets_kernel one workgroup: the running sum of the set sizes into cand_off, (sum, max) into totals
// Fill    un_fill_kernel, one workgroup per (block, query): a word per thread, an exclusive scan of the popcounts, and the word's bits
//         become ascending doc ids at cand_off[n] + the block's prefix + the scan -- so the list is sorted because the bitmap is.
//         Positions outside [0, n_cand) are not written.
// Bounds  a list's pair of offsets is clamped to [0, n_list]; only ids in [0, C) index cen_off, only doc ids in [0, corpus_len) index
//         the bitmap; every bitmap access is below nq * stride words, every block-count access below nq * nblk.
#pragma once

#include "../../include/dprhot_union.h"

namespace dprhot {

constexpr int UN_BLK_WORDS = 256;                 // words per block of the count and the fill pass: one per thread of the fill
constexpr int UN_BLK_DOCS = UN_BLK_WORDS * 32;    // 8192 doc ids
constexpr int UN_COUNT_THREADS = 1024;

struct UnLayout {
  long long nblk;     // blocks per query
  long long stride;   // bitmap words per query (nblk * UN_BLK_WORDS)
  size_t blk_at;      // byte offset of the block prefixes int32 [nq, nblk]
  size_t cnt_at;      // byte offset of the set sizes int32 [nq]
  size_t total;
};

inline UnLayout un_layout(int nq, long long corpus_len) {
  UnLayout l;
  l.nblk = (corpus_len + UN_BLK_DOCS - 1) / UN_BLK_DOCS;
  l.stride = l.nblk * UN_BLK_WORDS;
  l.blk_at = (size_t)nq * (size_t)l.stride * 4;
  l.cnt_at = l.blk_at + (size_t)nq * (size_t)l.nblk * 4;
  l.total = (l.cnt_at + (size_t)nq * 4 + 15) / 16 * 16;
  return l;
}

__global__ __launch_bounds__(256) void un_clear_kernel(uint4* bm, long long n16) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) bm[i] = uint4{0u, 0u, 0u, 0u};
}

struct UnMarkArgs {
  const long long* cids;     // [nq, LQ, nprobe]
  const uint16_t* q;         // bf16 [nq, LQ, dp]
  int dp, LQ, nprobe, C;
  long long waves;           // nq * LQ * nprobe
  const long long* cen_off;  // [C + 1]
  const int* cen_doc;        // [n_list]
  long long n_list, corpus_len, stride;
  unsigned* bm;
};

__global__ __launch_bounds__(256) void un_mark_kernel(UnMarkArgs p) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // (n * LQ + i) * nprobe + probe
  if (w >= p.waves) return;
  const long long c = p.cids[w];
  if (c < 0 || c >= p.C) return;
  const long long tokrow = w / p.nprobe;  // n * LQ + i
  const uint16_t* row = p.q + tokrow * p.dp;
  bool nz = false;
  for (int f = lane; f < p.dp; f += 64) nz |= (row[f] & 0x7fffu) != 0;  // -0.0 is zero, a NaN is not
  if (__ballot(nz) == 0) return;
  long long lo = p.cen_off[c], hi = p.cen_off[c + 1];
  lo = lo < 0 ? 0 : lo > p.n_list ? p.n_list : lo;
  hi = hi < 0 ? 0 : hi > p.n_list ? p.n_list : hi;
  unsigned* bm = p.bm + (tokrow / p.LQ) * p.stride;
  for (long long e = lo + lane; e < hi; e += 256) {
    int doc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) doc[u] = e + u * 64 < hi ? p.cen_doc[e + u * 64] : -1;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (doc[u] >= 0 && doc[u] < p.corpus_len) atomicOr(bm + (doc[u] >> 5), 1u << (doc[u] & 31));
  }
}

// inclusive scan of one int per thread over a workgroup of NW waves; `tot` receives the workgroup's sum.  Two barriers; sw: NW ints of LDS
template <int NW>
__device__ __forceinline__ int un_block_scan(int v, int* sw, int& tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  __syncthreads();  // sw may still be read from the call before
  if (lane == 63) sw[wave] = v;
  __syncthreads();
  int before = 0;
  tot = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int s = sw[i];
    if (i < wave) before += s;
    tot += s;
  }
  return v + before;
}

__global__ __launch_bounds__(UN_COUNT_THREADS) void un_count_kernel(const unsigned* bm_all, int* blk_all, int* qcnt, long long nblk,
                                                                    long long stride) {
  __shared__ int sw[UN_COUNT_THREADS / 64];
  const int n = (int)blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned* bm = bm_all + (long long)n * stride;
  int* blk = blk_all + (long long)n * nblk;
  for (long long b = wave; b < nblk; b += UN_COUNT_THREADS / 64) {
    const uint4 v = *reinterpret_cast<const uint4*>(bm + b * UN_BLK_WORDS + lane * 4);
    int c = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if (lane == 0) blk[b] = c;
  }
  __syncthreads();  // the block counts are this workgroup's own stores: visible to it behind the barrier
  int carry = 0;
  for (long long b0 = 0; b0 < nblk; b0 += UN_COUNT_THREADS) {
    const long long b = b0 + tid;
    const int c = b < nblk ? blk[b] : 0;
    int tot;
    const int inc = un_block_scan<UN_COUNT_THREADS / 64>(c, sw, tot);
    if (b < nblk) blk[b] = carry + inc - c;
    carry += tot;
  }
  if (tid == 0) qcnt[n] = carry;
}

__global__ __launch_bounds__(1024) void un_offsets_kernel(const int* qcnt, int nq, long long* cand_off, long long* totals) {
  __shared__ long long sw[16];
  __shared__ int smax[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long carry = 0;
  int mx = 0;
  for (int n0 = 0; n0 < nq; n0 += 1024) {
    const int n = n0 + tid;
    const int c = n < nq ? qcnt[n] : 0;
    mx = c > mx ? c : mx;
    long long v = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long o = __shfl_up(v, d, 64);
      if (lane >= d) v += o;
    }
    __syncthreads();
    if (lane == 63) sw[wave] = v;
    __syncthreads();
    long long before = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long long s = sw[i];
      if (i < wave) before += s;
      tot += s;
    }
    if (n < nq) cand_off[n + 1] = carry + before + v;
    carry += tot;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int o = __shfl_xor(mx, d, 64);
    mx = o > mx ? o : mx;
  }
  if (lane == 0) smax[wave] = mx;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 16; ++i) mx = smax[i] > mx ? smax[i] : mx;
    cand_off[0] = 0;
    totals[0] = carry;
    totals[1] = mx;
  }
}

__global__ __launch_bounds__(UN_BLK_WORDS) void un_fill_kernel(const unsigned* bm_all, const int* blk_all, long long nblk, long long stride,
                                                               const long long* cand_off, int* cand_doc, long long n_cand) {
  __shared__ int sw[UN_BLK_WORDS / 64];
  const int n = (int)blockIdx.y, tid = threadIdx.x;
  const long long b = blockIdx.x;
  unsigned word = bm_all[(long long)n * stride + b * UN_BLK_WORDS + tid];
  const int c = __popc(word);
  int tot;
  const int inc = un_block_scan<UN_BLK_WORDS / 64>(c, sw, tot);
  if (tot == 0) return;
  long long pos = cand_off[n] + blk_all[(long long)n * nblk + b] + (inc - c);
  const long long doc0 = b * UN_BLK_DOCS + tid * 32;  // a set bit is a doc id below corpus_len
  while (word) {
    const int bit = __ffs(word) - 1;
    word &= word - 1;
    if (pos >= 0 && pos < n_cand) cand_doc[pos] = (int)(doc0 + bit);
    ++pos;
  }
}

}  // namespace dprhot

// ---- the entry points of include/dprhot_union.h ----
static int un_check_shape(int nq, int64_t corpus_len) {
  REQUIRE(nq >= 1 && nq <= 65535, "bad shape nq=%d (1 .. 65535 queries in one launch)", nq);
  REQUIRE(corpus_len > 0 && corpus_len < (1ll << 31), "corpus_len=%lld out of range (1 .. 2^31 - 1)", (long long)corpus_len);
  return DPRHOT_OK;
}

static int un_check_workspace(const char* who, const dprhot::UnLayout& l, const void* workspace, size_t workspace_bytes) {
  if (workspace == nullptr || workspace_bytes < l.total)
    return fail(DPRHOT_E_WORKSPACE, "%s needs %zu workspace bytes (dprhot_colbert_union_workspace_bytes), got %zu", who, l.total,
                workspace == nullptr ? (size_t)0 : workspace_bytes);
  REQUIRE(aligned16(workspace), "the workspace must be 16-byte aligned");
  return DPRHOT_OK;
}

int dprhot_colbert_union_workspace_bytes(int nq, int64_t corpus_len, size_t* bytes) {
  if (int rc = un_check_shape(nq, corpus_len)) return rc;
  REQUIRE(bytes, "NULL pointer (bytes is required)");
  *bytes = dprhot::un_layout(nq, corpus_len).total;
  return DPRHOT_OK;
}

int dprhot_colbert_union_count(const int64_t* cids, const dprhot_bf16* q_tok, int dp, int nq, int LQ, int nprobe, int C, const int64_t* cen_off,
                               const int32_t* cen_doc, int64_t n_list, int64_t corpus_len, int64_t* cand_off, int64_t* totals, void* workspace,
                               size_t workspace_bytes, void* stream) {
  using namespace dprhot;
  if (int rc = un_check_shape(nq, corpus_len)) return rc;
  REQUIRE(LQ >= 1 && LQ <= DPRHOT_MAXSIM_MAX_LEN, "LQ=%d out of range (1 .. %d)", LQ, DPRHOT_MAXSIM_MAX_LEN);
  REQUIRE(nprobe >= 1, "nprobe=%d out of range (>= 1)", nprobe);
  REQUIRE(C >= 1, "C=%d out of range (1 .. 2^31 - 1)", C);
  REQUIRE(dp > 0 && dp % 32 == 0, "dp=%d must be a positive multiple of 32 (pad with zeros)", dp);
  REQUIRE(n_list >= 0 && n_list < (1ll << 40), "n_list=%lld out of range (< 2^40)", (long long)n_list);
  REQUIRE(cids && q_tok && cen_off && cand_off && totals && (n_list == 0 || cen_doc),
          "NULL pointer (cids, q_tok, cen_off, cen_doc, cand_off and totals are required)");
  const UnLayout l = un_layout(nq, corpus_len);
  if (int rc = un_check_workspace("colbert_union_count", l, workspace, workspace_bytes)) return rc;
  const long long waves = (long long)nq * LQ * nprobe;
  if (waves >= (1ll << 33)) return fail(DPRHOT_E_UNSUPPORTED, "nq=%d LQ=%d nprobe=%d: too many (token, probe) pairs for one launch", nq, LQ, nprobe);
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  unsigned* bm = reinterpret_cast<unsigned*>(ws);
  int* blk = reinterpret_cast<int*>(ws + l.blk_at);
  int* qcnt = reinterpret_cast<int*>(ws + l.cnt_at);
  const long long n16 = (long long)nq * l.stride / 4;
  const long long clear_blocks = (n16 + 255) / 256;
  if (int rc = launch<un_clear_kernel>(dim3((unsigned)(clear_blocks < 16384 ? clear_blocks : 16384)), dim3(256), 0, st, reinterpret_cast<uint4*>(bm),
                                       n16))
    return rc;
  UnMarkArgs a{reinterpret_cast<const long long*>(cids), q_tok, dp, LQ, nprobe, C, waves, reinterpret_cast<const long long*>(cen_off), cen_doc,
               (long long)n_list, (long long)corpus_len, l.stride, bm};
  if (int rc = launch<un_mark_kernel>(dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, a)) return rc;
  if (int rc = launch<un_count_kernel>(dim3((unsigned)nq), dim3(UN_COUNT_THREADS), 0, st, (const unsigned*)bm, blk, qcnt, l.nblk, l.stride)) return rc;
  return launch<un_offsets_kernel>(dim3(1), dim3(1024), 0, st, (const int*)qcnt, nq, reinterpret_cast<long long*>(cand_off),
                                   reinterpret_cast<long long*>(totals));
}

int dprhot_colbert_union_fill(int nq, int64_t corpus_len, const int64_t* cand_off, int32_t* cand_doc, int64_t n_cand, const void* workspace,
                              size_t workspace_bytes, void* stream) {
  using namespace dprhot;
  if (int rc = un_check_shape(nq, corpus_len)) return rc;
  REQUIRE(n_cand >= 0 && n_cand < (1ll << 40), "n_cand=%lld out of range (< 2^40)", (long long)n_cand);
  REQUIRE(cand_off && (n_cand == 0 || cand_doc), "NULL pointer (cand_off and cand_doc are required)");
  const UnLayout l = un_layout(nq, corpus_len);
  if (int rc = un_check_workspace("colbert_union_fill", l, workspace, workspace_bytes)) return rc;
  if (n_cand == 0) return DPRHOT_OK;  // a capacity of nothing: nothing to write
  const char* ws = static_cast<const char*>(workspace);
  return launch<un_fill_kernel>(dim3((unsigned)l.nblk, (unsigned)nq), dim3(UN_BLK_WORDS), 0, (hipStream_t)stream,
                                reinterpret_cast<const unsigned*>(ws), reinterpret_cast<const int*>(ws + l.blk_at), l.nblk, l.stride,
                                reinterpret_cast<const long long*>(cand_off), cand_doc, (long long)n_cand);
}
