// ffpa_mla_index_scores_fp8.h — the FP8 index-key side of DeepSeek-V3.2's indexer (ffpa_attn_mla_index_scores_fp8 and ffpa_attn_mla_index_k_append_fp8,
// ffpa_capi.hip): the page format, the arguments of the score launch and of the quantising append, and their launchers (ffpa_mla_index_scores_fp8.hip).  A header
// of its own so that the attention kernels' objects and the 16-bit score unit see nothing of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ffpa {

// THE PAGE FORMAT (the engines' indexer cache; ffpa_attn_amd/kvcache.py: pack_index_key_pages).  A page of page_size keys is page_size * 132 bytes:
//   bytes [0, page_size * 128)                  the code plane: 128 OCP e4m3 codes per key, row-major
//   bytes [page_size * 128, page_size * 132)    the scale plane: one float32 per key,  key = scale x codes
// NOT 132 interleaved bytes per key.  Without a block table a sequence's whole capacity is one such page.
constexpr int kMlaIndexFp8Dim = 128;       // columns of an index query head / of an index key: the FP8 MFMA's whole K dimension
constexpr int kMlaIndexFp8RowBytes = 132;  // a key's share of its page

// scores[t, p] = kscale[b_t, p] * sum_h w[t, h] * max(0, sum_d q8[t, h, d] * k8[b_t, p, d]) for p < n_t, -inf for n_t <= p < N.  The token rules are
// MlaIndexScoresArgs's (ffpa_mla_index_scores.h).  Strides of q and k in BYTES (= e4m3 elements), the others in elements.
struct MlaIndexScoresFp8Args {
  const uint8_t* q;          // [T, Hi, 128] e4m3 by s_q_tok / s_q_head (multiples of 16)
  const uint8_t* k;          // [num_pages] pages of the format above, s_k_page apart (a multiple of 16)
  const float* w;            // [T, Hi] by s_w
  const int* cache_seqlens;  // [B]
  const int* cu_seqlens_q;   // [B + 1], or nullptr: token t is token t % (T / B) of sequence t / (T / B)
  const int* block_table;    // [B, W] by s_table, or nullptr: page id = b, page_size = the capacity, W = 1, num_pages = B
  float* scores;             // [T, N] by s_out
  int64_t s_q_tok, s_q_head, s_k_page, s_w, s_table, s_out;
  int T, N, B, W, page_size, num_pages, Hi, causal, chunk;  // chunk: 256 / 512 / 1024
};

int launch_mla_index_scores_fp8(const MlaIndexScoresFp8Args& a, hipStream_t stream);

// The quantising append of the step's index keys: row t of k_new — token i of sequence b, by cu_seqlens_q and its binary search (rows at and past cu_q[B] write
// nothing) or t / (T / B) and t % (T / B) — goes to cache position max(cache_seqlens[b], 0) + i, dropped at or past the capacity W * page_size;
// lens_after[b] = min(max(cache_seqlens[b], 0) + the sequence's new rows, capacity) for every b < B: the latent appends' placement rule (ffpa_mla.h).
struct MlaIndexKAppendFp8Args {
  uint8_t* k;                // the pool, pages s_k_page bytes apart
  const void* k_new;         // [T, 128] bf16 / fp16 by s_new (elements, a multiple of 8)
  const int* cache_seqlens;  // [B] lengths before the step
  const int* cu_seqlens_q;   // [B + 1] or nullptr
  const int* block_table;    // [B, W] by s_table, or nullptr
  int* lens_after;           // [B], written
  int64_t s_k_page, s_new, s_table;
  int T, B, W, page_size, num_pages, fp16;
};

int launch_mla_index_k_append_fp8(const MlaIndexKAppendFp8Args& a, hipStream_t stream);

}  // namespace ffpa
