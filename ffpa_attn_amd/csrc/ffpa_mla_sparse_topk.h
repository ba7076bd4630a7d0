// ffpa_mla_sparse_topk.h — the selection launch in front of the sparse latent calls (ffpa_attn_mla_sparse_topk_slots, ffpa_capi.hip): its arguments and its launcher
// (ffpa_mla_sparse_topk.hip).  A header of its own so that the attention kernels' objects see nothing of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ffpa {

// Exactly one of scores / positions is set.  scores [T, N] (float32): the topk largest of a token's visible columns, as pool slots in ascending position order.
// positions [T, topk] (int32): the entries >= 0, in their order, as pool slots.  Both write indices [T, topk] (-1 behind the count) and topk_lens [T].
struct MlaSparseTopkArgs {
  const float* scores;
  const int* positions;
  const int* cache_seqlens;  // [B]
  const int* cu_seqlens_q;   // [B + 1], or nullptr: token t is token t % (T / B) of sequence t / (T / B)
  const int* block_table;    // [B, W] by s_table, or nullptr: the positions themselves are written
  int* indices;
  int* topk_lens;
  int64_t s_row;    // elements: the row stride of scores / positions
  int64_t s_table;  // elements: the row stride of block_table
  int64_t s_out;    // elements: the row stride of indices
  int T, N, topk, B, W, page_size, causal;
};

int launch_mla_sparse_topk(const MlaSparseTopkArgs& a, hipStream_t stream);

}  // namespace ffpa
