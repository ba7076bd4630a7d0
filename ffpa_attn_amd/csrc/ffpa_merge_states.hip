// ffpa_merge_states.hip — the merge of two attention states (C-ABI: ffpa_attn_merge_states, ffpa_capi.hip), the last launch of ffpa_attn_with_kvcache_cascade.
// A TU of its own: the dense, packed, paged and append objects stay exactly what they were.
//
// Per (token t, head h) row, in fp32: m = max(lse_a, lse_b), w_x = exp(lse_x - m), O = (w_a O_a + w_b O_b) / (w_a + w_b), LSE = m + ln(w_a + w_b); O is rounded
// once to the dtype.  A side of weight 0 (its LSE is -inf, or so far below the other that exp underflows) adds nothing: its O is not multiplied in, so a NaN
// behind a -inf LSE does not leak.  Both sides -inf: O = 0, LSE = -inf (the packed call's empty row).
// Memory-bound: a lane owns one 16-byte chunk of a row (8 elements) — it loads both LSEs and both chunks before any arithmetic, then stores one chunk; the lane of
// chunk 0 also stores the row's LSE.  Rows are t-major, so consecutive lanes walk consecutive bytes of a [T, H, D] tensor.  The launch side picks 64-lane
// workgroups when 256-lane ones would leave CUs idle (a decode step's few rows), and a grid-stride loop above a few workgroups per CU.
#include "ffpa_merge_states.h"

namespace ffpa {
namespace {

template <typename T>
__global__ __launch_bounds__(256) void ffpa_merge_states_kernel(const MergeStatesArgs a) {
  typedef T v8 __attribute__((ext_vector_type(8)));
  const int cpr = a.D >> 3;
  const int64_t total = (int64_t)a.T * a.H * cpr;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const int64_t row = e / cpr;
    const int c = (int)(e - row * cpr);
    const int t = (int)(row / a.H), h = (int)(row - (int64_t)t * a.H);
    const float la = a.la[h * a.sla + t], lb = a.lb[h * a.slb + t];
    const v8 xa = *(const v8*)((const T*)a.oa + t * a.soa[0] + h * a.soa[1] + c * 8);
    const v8 xb = *(const v8*)((const T*)a.ob + t * a.sob[0] + h * a.sob[1] + c * 8);
    const float m = fmaxf(la, lb);
    v8 out;
    float lse;
    if (m == -INFINITY) {
#pragma unroll
      for (int i = 0; i < 8; ++i) out[i] = (T)0.f;
      lse = -INFINITY;
    } else {
      const float wa = expf(la - m), wb = expf(lb - m);
      const float den = wa + wb;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float pa = wa > 0.f ? wa * (float)xa[i] : 0.f;
        const float pb = wb > 0.f ? wb * (float)xb[i] : 0.f;
        out[i] = (T)((pa + pb) / den);
      }
      lse = m + logf(den);
    }
    *(v8*)((T*)a.o + t * a.so[0] + h * a.so[1] + c * 8) = out;
    if (a.l != nullptr && c == 0) a.l[h * a.sl + t] = lse;
  }
}

}  // namespace

int launch_merge_states(int dtype, const MergeStatesArgs& a, unsigned blocks, unsigned threads, hipStream_t stream) {
  if (dtype == 0)
    hipLaunchKernelGGL((ffpa_merge_states_kernel<__bf16>), dim3(blocks), dim3(threads), 0, stream, a);
  else
    hipLaunchKernelGGL((ffpa_merge_states_kernel<_Float16>), dim3(blocks), dim3(threads), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace ffpa
