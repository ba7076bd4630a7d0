// ffpa_cu_seqlens_find.h — token row -> sequence of a batch packed by cu_seqlens_q, on the device: the one lookup of the ragged appends
// (ffpa_kv_append_varlen_kernel, ffpa_kvcache_append_varlen.hip; ffpa_mla_append_varlen_kernel, ffpa_mla_inst.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ffpa {

// the last b with cu_q[b] <= t: the first b in [0, B] whose cu_q[b + 1] > t (B: none — a padding row, as is every row t >= T of a grid sized for used[]).
// t is the workgroup's index, so the search is wave-uniform; a caller that runs it in front of its first store gets scalar loads, log2(B) + 1 of them.
// Empty sequences (cu_q[b + 1] == cu_q[b]) are stepped over.
__device__ __forceinline__ int cu_seqlens_find(const int* cu_q, int B, int T, int t) {
  int b = B;
  if (t < T) {
    int hi = B;
    b = 0;
    while (b < hi) {
      const int mid = (b + hi) >> 1;
      if (cu_q[mid + 1] <= t)
        b = mid + 1;
      else
        hi = mid;
    }
  }
  return b;
}

}  // namespace ffpa
