// ffpa_mla_cascade_plan.h — the plan launch of shared-prefix (cascade) attention over the MLA latent cache (ffpa_attn_mla_cascade_plan, ffpa_capi.hip): its
// arguments and its launcher (ffpa_mla_cascade_plan.hip).  A header of its own so that the attention kernels' objects see nothing of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ffpa {

// B sequences cut into G groups of consecutive sequences by cu_group [G + 1] (nullptr: one group of all B).  Everything is int32; the outputs are dense.
struct MlaCascadePlanArgs {
  const int* cu_group;  // [G + 1] or nullptr
  const int* prefix;    // [G] stated prefix lengths, or nullptr: prefix_host for every group
  const int* lens;      // [B] post-append lengths, not clamped
  const int* table;     // [B, W] by bt_stride (column stride 1)
  int* cu_q_prefix;     // out [G + 1]
  int* prefix_lens;     // out [G]
  int* prefix_table;    // out [G, W]
  int* suffix_table;    // out [B, W]
  int* suffix_lens;     // out [B]
  int64_t bt_stride;
  int B, G, W, page, Sq, causal, capacity, prefix_host;
};

// grid = B + G workgroups of 64 lanes: workgroup i < B writes sequence i's suffix row and length, workgroup B + g the outputs of group g.  Returns a hipError_t.
int launch_mla_cascade_plan(const MlaCascadePlanArgs& a, hipStream_t stream);

}  // namespace ffpa
