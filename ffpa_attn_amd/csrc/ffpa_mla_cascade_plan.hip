// ffpa_mla_cascade_plan.hip — the plan launch of shared-prefix (cascade) attention over the MLA latent cache (C-ABI: ffpa_attn_mla_cascade_plan, ffpa_capi.hip):
// what the prefix pass and the suffix pass of ffpa_attn_with_kvcache_mla_cascade read, made on the device in ONE launch so that nothing crosses to the host and
// the step stays one HIP graph.  A TU of its own: the attention, append and merge objects stay exactly what they were.
//
// The batch is cut into G groups of consecutive sequences (cu_group [G + 1]; nullptr: one group).  Per group g, with len'_b = clamp(len_b, 0, capacity):
//     P_g = page * floor(clamp(min(stated_g, min over b in g of (len'_b - (Sq - 1 if causal else 0))), 0, capacity) / page)      (an empty group: 0)
// and the launch stores
//     cu_q_prefix [G + 1] = cu_group * Sq            prefix_lens [G] = P_g            prefix_table [g, :] = table [first sequence of g, :]
//     suffix_table [b, j] = table [b, min(j + P_g / page, W - 1)]                     suffix_lens [b] = len'_b - P_g
// Workgroup i < B serves sequence i, workgroup B + g group g; both recompute the group's minimum by a loop over its lengths (64 lanes, one wave reduction), so
// there are no atomics and no second launch.  The group of a sequence is a binary search of cu_group by the workgroup's index: wave-uniform.  Every index that
// becomes an address is clamped into its array first — a cu_group that breaks its contract (not non-decreasing from 0 to B) gives unspecified VALUES, never an
// out-of-bounds access.
#include "ffpa_mla_cascade_plan.h"

#include <climits>

#include "ffpa_cu_seqlens_find.h"

namespace ffpa {
namespace {

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// P of the group that holds sequences [s, e), 0 <= s <= e <= B: every lane returns it
__device__ __forceinline__ int group_prefix(const MlaCascadePlanArgs& a, int g, int s, int e) {
  if (s >= e) return 0;
  const int back = a.causal ? a.Sq - 1 : 0;
  int m = INT_MAX;
  for (int i = s + (int)threadIdx.x; i < e; i += 64) m = min(m, clampi(a.lens[i], 0, a.capacity) - back);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off, 64));
  const int stated = a.prefix != nullptr ? a.prefix[g] : a.prefix_host;
  return clampi(min(stated, m), 0, a.capacity) / a.page * a.page;
}

__global__ __launch_bounds__(64) void ffpa_mla_cascade_plan_kernel(const MlaCascadePlanArgs a) {
  const int lane = (int)threadIdx.x;
  const int blk = (int)blockIdx.x;
  if (blk < a.B) {
    // sequence blk: its suffix row and length
    const int b = blk;
    int g = 0, s = 0, e = a.B;
    if (a.cu_group != nullptr) {
      g = cu_seqlens_find(a.cu_group, a.G, a.cu_group[a.G], b);
      if (g < a.G) {
        s = clampi(a.cu_group[g], 0, a.B);
        e = clampi(a.cu_group[g + 1], s, a.B);
      } else {
        s = e = 0;  // (past cu_group[G], a broken contract: no prefix)
      }
    }
    const int P = group_prefix(a, g, s, e);
    const int shift = P / a.page;
    const int* row = a.table + (int64_t)b * a.bt_stride;
    int* out = a.suffix_table + (int64_t)b * a.W;
    for (int j = lane; j < a.W; j += 64) out[j] = row[min(j + shift, a.W - 1)];
    if (lane == 0) a.suffix_lens[b] = max(clampi(a.lens[b], 0, a.capacity) - P, 0);
  } else {
    // group g: its query boundary, its prefix length and the table row of its first sequence
    const int g = blk - a.B;
    const int lo = a.cu_group != nullptr ? a.cu_group[g] : 0;
    const int hi = a.cu_group != nullptr ? a.cu_group[g + 1] : a.B;
    const int s = clampi(lo, 0, a.B);
    const int e = clampi(hi, s, a.B);
    const int P = group_prefix(a, g, s, e);
    const int* row = a.table + (int64_t)min(s, a.B - 1) * a.bt_stride;  // (an empty group behind the last sequence reads the last row: any in-range row will do)
    int* out = a.prefix_table + (int64_t)g * a.W;
    for (int j = lane; j < a.W; j += 64) out[j] = row[j];
    if (lane == 0) {
      a.cu_q_prefix[g] = lo * a.Sq;
      a.prefix_lens[g] = P;
      if (g == a.G - 1) a.cu_q_prefix[a.G] = hi * a.Sq;
    }
  }
}

}  // namespace

int launch_mla_cascade_plan(const MlaCascadePlanArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(ffpa_mla_cascade_plan_kernel, dim3((unsigned)(a.B + a.G)), dim3(64), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace ffpa
