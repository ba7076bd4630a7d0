// ffpa_mla_index_scores.h — the score launch of DeepSeek-V3.2's indexer, in front of the selection (ffpa_attn_mla_index_scores, ffpa_capi.hip): its arguments and
// its launcher (ffpa_mla_index_scores.hip).  A header of its own so that the attention kernels' objects see nothing of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ffpa {

constexpr int kMlaIndexDim = 128;        // columns of an index query head / of an index key

// scores[t, p] = sum_h w[t, h] * max(0, q[t, h, :] . k[b_t, p, :]) for p < n_t, -inf for n_t <= p < N.  Strides in elements.  Without a block_table the cache is
// one page per sequence: page id = b, page_size = the capacity, W = 1, num_pages = B.
struct MlaIndexScoresArgs {
  const void* q;             // [T, Hi, 128] by s_q_tok / s_q_head, 16-bit
  const void* k;             // [num_pages, page_size, 128] by s_k_page / s_k_row, the same type
  const float* w;            // [T, Hi] by s_w
  const int* cache_seqlens;  // [B]
  const int* cu_seqlens_q;   // [B + 1], or nullptr: token t is token t % (T / B) of sequence t / (T / B)
  const int* block_table;    // [B, W] by s_table, or nullptr
  float* scores;             // [T, N] by s_out
  int64_t s_q_tok, s_q_head, s_k_page, s_k_row, s_w, s_table, s_out;
  int T, N, B, W, page_size, num_pages, Hi, causal, fp16, chunk;  // chunk: 256 / 512 / 1024
};

int launch_mla_index_scores(const MlaIndexScoresArgs& a, hipStream_t stream);

}  // namespace ffpa
