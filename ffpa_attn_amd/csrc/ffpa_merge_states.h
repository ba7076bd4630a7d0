// ffpa_merge_states.h — the merge of two attention states (ffpa_attn_merge_states, ffpa_capi.hip): its arguments and its launcher (ffpa_merge_states.hip).  A
// header of its own so that the attention kernels' objects see nothing of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ffpa {

// Rows (token t, head h), t-major; a row is D / 8 chunks of 16 bytes.  O by {token, head} element strides, LSE by a head stride (token stride 1).
struct MergeStatesArgs {
  const void* oa;
  const void* ob;
  void* o;
  const float* la;
  const float* lb;
  float* l;  // nullptr: no output LSE
  int64_t soa[2], sob[2], so[2];
  int64_t sla, slb, sl;
  int T, H, D;
};

// grid = `blocks` workgroups of `threads` lanes (64 or 256), a grid-stride loop over the T x H x D / 8 chunks.  Returns a hipError_t.
int launch_merge_states(int dtype, const MergeStatesArgs& a, unsigned blocks, unsigned threads, hipStream_t stream);

}  // namespace ffpa
