// ffpa_mla_sparse_topk.hip — the launch that MAKES the inputs of the sparse latent calls (ffpa_attn_mla_sparse_topk_slots, ffpa_capi.hip): from an indexer's float32
// score per (query token, logical key position) to the pair (indices [T, topk], topk_lens [T]) of pool slots, in one kernel.  A small TU of its own, no inline
// asm; every store is an ordinary vector store.
//
// THE RESULT — tests/kvcache_mla_sparse_topk_ref.py is the definition.  Token t is token i of sequence b (cu_seqlens_q and its binary search, or t / Sq and
// t % Sq), which has S query tokens and length L = cache_seqlens[b]; it sees the columns [0, n), n = clamp(L - (S - 1 - i), 0, N) under causal, clamp(L, 0, N)
// otherwise.  n <= topk: all of them.  Otherwise the topk largest in the order of torch.sort(descending=True, stable=True): NaN is the largest value, -0.0 equals
// +0.0, among equal scores the lower position wins.  The selected positions are written in ASCENDING position order, translated through the sequence's row of
// block_table (position p -> table[b, min(p / page_size, W - 1)] * page_size + p % page_size), then -1 up to topk; topk_lens[t] = min(n, topk).  A row at or past
// cu_seqlens_q[B] is padding: count 0, a row of -1.  The positions mode is the same kernel's last phase with "entry >= 0" as the predicate.
//
// HOW.  One workgroup of 1024 lanes per token row.
//   1. a score becomes a 32-bit key whose unsigned order is the selection's: -0.0 -> +0.0, the sign flip, every NaN -> 0xFFFFFFFF;
//   2. an MSB-first radix select, 8 bits per pass, over the first n columns finds the key of rank topk and the number of strictly larger keys: a 256-bin LDS
//      histogram of 32-bit counters per pass, over the keys that carry the prefix found so far, filled with LDS atomics.  It is kept in sixteen copies, a
//      lane adds to copy lane % 16 and the copies lie 257 words apart: the lanes of a wave that hold one digit — most of them in the first pass, all of them on
//      a row of equal scores — meet four to an address on sixteen banks.  A wave without a live key skips its atomics (the later passes).  The copies are
//      summed, every wave finds the bucket of the rank with one suffix sum over its lanes, and the select stops as soon as a bucket is taken whole;
//   3. one pass over the row in position order, 8192 columns a step, a wave on 512 consecutive ones: a column is taken if its key is above the threshold, or
//      equals it while fewer than topk - larger equal keys have been taken in front of it.  Ballots and popcounts inside a wave, one prefix over the sixteen waves'
//      counts through LDS and one barrier per step give each taken column its output index: ascending order and "lower position wins" with no sort.  The pass
//      stores POSITIONS and ends as soon as the count is reached;
//   4. the translation is a last sweep over the row's count entries with every lane busy — the block-table lookup is a per-lane load, the division by
//      page_size the kernel's longest instruction sequence (at the ordered pass's stores one lane in sixteen would run it) —; 5. the tail is filled with -1.
// The wave-uniform reads — the sequence search, the length — stand in front of the first store.  Addresses are 64-bit, stores int32.  Every index that becomes an
// address is bounded first: a column by n <= N, a table column by W - 1, an output index by topk (scores rewritten while the kernel runs give unspecified
// VALUES, never a store past the row).
#include "ffpa_mla_sparse_topk.h"

#include "ffpa_cu_seqlens_find.h"

namespace ffpa {
namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 8;                  // 64-column pieces a wave holds per step
constexpr int kSpan = kThreads * kPer;   // columns per step
constexpr int kBins = 256;
constexpr int kCopies = 16;              // copies of the histogram a wave's lanes spread over
constexpr int kCopyStride = kBins + 1;   // words between two copies: one digit of two copies lies on two banks

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// float32 -> the key whose unsigned order is that of a stable descending sort: NaN above +inf, -0.0 with +0.0
__device__ __forceinline__ uint32_t score_key(float x) {
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  if (u == 0x80000000u) u = 0u;  // (what x + 0.0f does)
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// hist[digit] += 1 for every live lane, in the lane's own copy of the histogram: sixteen copies, 257 words apart, so that the lanes of a wave that hold one digit
// — most of them in the first pass, all of them on a row of equal scores — meet four to an address on sixteen banks, not sixty-four on one.  Called by whole
// waves; a wave without a live lane does nothing (the later passes, where few keys carry the prefix).
__device__ __forceinline__ void hist_add(uint32_t* hist, bool live, uint32_t digit, int lane) {
  if (__ballot(live) == 0) return;
  if (live) atomicAdd(&hist[(lane & (kCopies - 1)) * kCopyStride + digit], 1u);
}

// exclusive prefix sum over the first 16 lanes of a wave (the other lanes hold 0)
__device__ __forceinline__ int scan16_excl(int v, int lane) {
  int s = v;
#pragma unroll
  for (int d = 1; d < kWaves; d <<= 1) {
    const int up = __shfl_up(s, d, 64);
    if (lane >= d) s += up;
  }
  return s - v;
}

__global__ __launch_bounds__(kThreads) void ffpa_mla_sparse_topk_kernel(const MlaSparseTopkArgs a) {
  __shared__ uint32_t hist[kCopies * kCopyStride];
  __shared__ uint32_t bins[kBins];
  __shared__ int wsum[2][kWaves][2];
  const int t = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint64_t below = (1ull << lane) - 1;
  const bool by_score = a.scores != nullptr;

  // ---- wave-uniform: the token's sequence, its visible length
  int b, n;
  {
    int i, S;
    if (a.cu_seqlens_q != nullptr) {
      b = cu_seqlens_find(a.cu_seqlens_q, a.B, a.cu_seqlens_q[a.B], t);
      const int lo = b < a.B ? a.cu_seqlens_q[b] : 0;
      i = t - lo, S = b < a.B ? a.cu_seqlens_q[b + 1] - lo : 0;
    } else {
      S = a.T / a.B, b = t / S, i = t % S;
    }
    const bool pad = b >= a.B;
    b = clampi(b, 0, a.B - 1);
    const int L = a.cache_seqlens[b];
    const int64_t vis = a.causal ? (int64_t)L - (S - 1 - i) : (int64_t)L;
    n = pad ? 0 : (by_score ? (int)(vis < 0 ? 0 : (vis > a.N ? a.N : vis)) : a.topk);
  }
  const float* srow = a.scores + (by_score ? (int64_t)t * a.s_row : 0);
  const int* prow = a.positions + (by_score ? 0 : (int64_t)t * a.s_row);
  const int* table = a.block_table != nullptr ? a.block_table + (int64_t)b * a.s_table : nullptr;
  int* out = a.indices + (int64_t)t * a.s_out;

  // ---- the threshold: keys >= `thr` are taken when `whole`; else keys > thr, and the first `need` keys == thr
  uint32_t thr = 0;
  bool whole = true;
  int need = 0;
  if (by_score && n > a.topk) {
    uint32_t prefix = 0, known = 0;
    int rank = a.topk;  // the rank looked for among the keys that carry `prefix`
    whole = false;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int w = tid; w < kCopies * kCopyStride; w += kThreads) hist[w] = 0;
      __syncthreads();
      for (int base = 0; base < n; base += kSpan) {
        float x[kPer];
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
          const int c = base + e * kThreads + tid;
          x[e] = c < n ? srow[c] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
          const uint32_t key = score_key(x[e]);
          hist_add(hist, base + e * kThreads + tid < n && (key & known) == prefix, (key >> shift) & 0xffu, lane);
        }
      }
      __syncthreads();
      if (tid < kBins) {
        uint32_t sum = 0;
#pragma unroll
        for (int c = 0; c < kCopies; ++c) sum += hist[c * kCopyStride + tid];
        bins[tid] = sum;
      }
      __syncthreads();
      // every wave reads the histogram and finds the digit d with count(bins > d) < rank <= count(bins >= d): lane l holds bins 4l ... 4l + 3
      const uint32_t h4[4] = {bins[4 * lane], bins[4 * lane + 1], bins[4 * lane + 2], bins[4 * lane + 3]};
      const int own = (int)(h4[0] + h4[1] + h4[2] + h4[3]);
      int from = own;  // the count of bins >= 4l
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int dn = __shfl_down(from, d, 64);
        if (lane + d < 64) from += dn;
      }
      int above = from - own, digit = 0, in_bucket = 0;
      const bool hit = above < rank && rank <= from;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        const int cnt = (int)h4[j];
        if (in_bucket == 0 && above + cnt >= rank) digit = 4 * lane + j, in_bucket = cnt;
        if (in_bucket == 0) above += cnt;
      }
      const uint64_t hits = __ballot(hit);
      const int src = hits != 0 ? __builtin_ctzll(hits) : 0;
      digit = __shfl(digit, src, 64), above = __shfl(above, src, 64), in_bucket = __shfl(in_bucket, src, 64);
      prefix |= (uint32_t)digit << shift, known |= 0xffu << shift;
      rank -= above;
      thr = prefix;
      if (in_bucket == rank) {  // the bucket is taken whole: no ties to count, no further pass
        whole = true;
        break;
      }
      need = rank;
    }
  }

  // ---- the ordered pass: a wave on 512 consecutive entries per step, one barrier per step
  const int rows = n;                                    // entries of the row that are looked at
  const int want = by_score ? min(n, a.topk) : a.topk;   // the pass ends when this many are taken
  const bool all = by_score && n <= a.topk;
  int taken_run = 0, tie_run = 0;
  for (int base = 0, par = 0; base < rows && taken_run < want; base += kSpan, par ^= 1) {
    const int seg = base + wave * (64 * kPer);
    int val[kPer];
    uint64_t m_take[kPer], m_tie[kPer];
    if (by_score && !all) {
      float x[kPer];
#pragma unroll
      for (int e = 0; e < kPer; ++e) {
        const int c = seg + e * 64 + lane;
        x[e] = c < rows ? srow[c] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < kPer; ++e) {
        const int c = seg + e * 64 + lane;
        const uint32_t key = score_key(x[e]);
        val[e] = c;
        m_take[e] = __ballot(c < rows && (whole ? key >= thr : key > thr));
        m_tie[e] = __ballot(c < rows && !whole && key == thr);
      }
    } else {
#pragma unroll
      for (int e = 0; e < kPer; ++e) {
        const int c = seg + e * 64 + lane;
        val[e] = by_score ? c : (c < rows ? prow[c] : -1);
        m_take[e] = __ballot(c < rows && val[e] >= 0);
        m_tie[e] = 0;
      }
    }
    int n_take = 0, n_tie = 0;
#pragma unroll
    for (int e = 0; e < kPer; ++e) n_take += __popcll(m_take[e]), n_tie += __popcll(m_tie[e]);
    if (lane == 0) wsum[par][wave][0] = n_take, wsum[par][wave][1] = n_tie;
    __syncthreads();
    // the waves in front of this one: their ties, and what they take (a wave takes its ties while the row's count of them is below `need`)
    const int w_take = lane < kWaves ? wsum[par][lane][0] : 0, w_tie = lane < kWaves ? wsum[par][lane][1] : 0;
    const int tie_front = scan16_excl(w_tie, lane);
    const int w_all = w_take + clampi(need - tie_run - tie_front, 0, w_tie);
    const int take_front = scan16_excl(w_all, lane);
    int tie_at = tie_run + __shfl(tie_front, wave, 64), at = taken_run + __shfl(take_front, wave, 64);
    taken_run += __shfl(take_front + w_all, kWaves - 1, 64), tie_run += __shfl(tie_front + w_tie, kWaves - 1, 64);
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const bool tie = (m_tie[e] >> lane) & 1u;
      const bool take = ((m_take[e] >> lane) & 1u) || (tie && tie_at + __popcll(m_tie[e] & below) < need);
      const uint64_t m = __ballot(take);
      const int j = at + __popcll(m & below);
      if (take && j < a.topk) out[j] = val[e];
      tie_at += __popcll(m_tie[e]), at += __popcll(m);
    }
  }
  const int count = min(taken_run, a.topk);
  // ---- the translation: one sweep over the row's `count` positions with every lane busy (the division by page_size is the kernel's longest instruction
  // sequence; at the ordered pass's stores one lane in sixteen would run it).  The positions were stored by other lanes of this workgroup: the barrier orders them.
  if (table != nullptr) {
    __syncthreads();
    const uint32_t ps = (uint32_t)a.page_size, last = (uint32_t)(a.W - 1);
    for (int j = tid; j < count; j += kThreads) {
      const uint32_t p = (uint32_t)out[j];
      out[j] = (int)((int64_t)table[min(p / ps, last)] * ps + p % ps);
    }
  }
  for (int j = count + tid; j < a.topk; j += kThreads) out[j] = -1;
  if (tid == 0) a.topk_lens[t] = count;
}

}  // namespace

int launch_mla_sparse_topk(const MlaSparseTopkArgs& a, hipStream_t stream) {
  if (a.T == 0) return 0;
  hipLaunchKernelGGL(ffpa_mla_sparse_topk_kernel, dim3((unsigned)a.T), dim3(kThreads), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace ffpa
