// ffpa_kvcache_append.h — the "prepare" launch of ffpa_attn_kvcache_append (ffpa_capi.hip): its arguments and its launcher (ffpa_kvcache_append.hip).  A header of
// its own so that the attention kernels' objects see nothing of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ffpa {

// One launch: the new K / V rows of every sequence written into its cache (K rotated), the rotated copy of q, and the post-append key lengths.
// Cache row `pos` of sequence b lives in page table[b * bt_stride + pos / page_size] (clamped to [0, num_pages)), row pos % page_size; a contiguous cache is one
// page per sequence (table == nullptr: page = b, page_size = cap) whose page stride is the batch stride.
struct KvAppendArgs {
  const void* q;   // [B, Sq, Hq, D] by sq = {batch, row, head}; read only with rd > 0
  const void* k;   // [B, Snew, Hkv, D] by sk
  const void* v;   // ... by sv
  void* kc;        // cache pools, rows / heads by skc / svc = {row, head}, pages by kc_page_stride / vc_page_stride
  void* vc;
  void* q_rot;     // [B, Sq, Hq, D] by sqr: q with its first rd dims rotated (rd > 0 only)
  int* used;       // [B] out: min(max(seqlens[b], 0) + Snew, cap)
  const int* seqlens;
  const void* cos;  // [seqlen_ro, rd / 2], q's dtype, contiguous
  const void* sin;
  const int* table;  // nullptr = contiguous cache
  int64_t bt_stride;
  int64_t kc_page_stride, vc_page_stride;
  int64_t sq[3], sk[3], sv[3], sqr[3];
  int64_t skc[2], svc[2];
  int B, Hq, Hkv, D, Sq, Snew;
  int cap;        // keys a sequence can hold: writes at pos >= cap are dropped
  int page_size;  // rows per page (contiguous: cap)
  int num_pages;  // contiguous: B
  int seqlen_ro;  // rows of cos / sin: positions are clamped to seqlen_ro - 1
  int rd;         // rotary dims (0 = none), a multiple of 16 <= D
  int causal;     // query token i at position seqlens[b] + i (else seqlens[b])
  int T;          // token rows per sequence in the grid: max(1, Snew, rd ? Sq : 0)
  int units;      // lanes per head: rd / 16 rotated pairs + (D - rd) / 8 copied chunks (NeoX), D / 8 chunks (interleaved)
  int slots;      // heads a workgroup holds side by side: 256 / units
};

// Heads one lane walks with the same cos / sin registers.
constexpr int kAppendHeadsPerLane = 4;

// grid = (B * T, y): y workgroups of `slots` x kAppendHeadsPerLane heads per token row.  Returns a hipError_t.
int launch_kv_append(int dtype, bool interleaved, const KvAppendArgs& a, unsigned grid_y, hipStream_t stream);

// The packed-token form (ffpa_attn_kvcache_append_varlen, ffpa_kvcache_append_varlen.hip): q / k / v are [total, H, D] token rows packed by cu_q, one grid row
// per token.  `a` holds what both forms share — the pools, the table, the rotary tables, the head geometry — with a.sq / sk / sv / sqr = {unused, row, head},
// a.B the sequences and a.T = total the token rows; a.Sq / a.Snew are not read (every token row is a query row and a new key).
struct KvAppendVarlenArgs {
  KvAppendArgs a;
  const int* cu_q;       // [B + 1]: token row t belongs to the sequence b with cu_q[b] <= t < cu_q[b + 1]; rows from cu_q[B] on are padding
  const int* positions;  // [total] rotary position of token row t (key AND query), or nullptr = the slot rule of the [B, S] form
};

// grid = (max(total, ceil(B / 256)), y): workgroup row t is token row t (if t < total); the first ceil(B / 256) rows of y == 0 also write used[].  Returns a hipError_t.
int launch_kv_append_varlen(int dtype, bool interleaved, const KvAppendVarlenArgs& va, unsigned grid_y, hipStream_t stream);

}  // namespace ffpa
