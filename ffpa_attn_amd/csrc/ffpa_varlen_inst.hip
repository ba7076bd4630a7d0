// ffpa_varlen_inst.hip — the packed-sequence kernel (ffpa_fwd_m16_varlen_kernel, ffpa_fwd_m16_kernel.h), one translation unit per head dim
// (compiled with -DFFPA_INST_D=<D>, D a multiple of 64 in [128, 1024]; bf16 + fp16 in the same TU).  A TU of its own so that the dense kernels'
// objects (ffpa_fwd_inst.hip) are exactly what they were before this entry point existed.  What it replaces in the reference: the CuTe-DSL
// launchers behind torch.ops.ffpa_attn._varlen_fwd_cute (src/ffpa_attn/cute/__init__.py:792-829).
#include "ffpa_fwd_kernel.h"
#include "ffpa_fwd_m16_kernel.h"
#include "ffpa_launch.h"
#include "ffpa_launch_kernel.h"

#ifndef FFPA_INST_D
#error "compile with -DFFPA_INST_D=<head dim>"
#endif

namespace ffpa {

template <typename T, int D, bool NT>
static int launch_varlen(const FwdArgs& a, const VarlenArgs& va, hipStream_t stream) {
  constexpr int BC = m16_block_keys(D, false);
  constexpr int LDS = 2 * BC * D * 2 + m16_exchange_bytes(D, 0);
  if (va.tree_tokens != 0) return launch_kernel<ffpa_fwd_m16_varlen_tree_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va);  // (under a tree mask: its own build)
  if (va.softcap_in > 0.f) return launch_kernel<ffpa_fwd_m16_varlen_softcap_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va);  // (capped scores: the window build with the cap)
  if (va.window != 0) return launch_kernel<ffpa_fwd_m16_varlen_window_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va);  // (under a sliding window: its own build)
  return launch_kernel<ffpa_fwd_m16_varlen_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va);
}

// nt: the decode-batch build (K / V pieces with the non-temporal hint: ffpa_capi.hip decides per launch)
int FFPA_CAT(launch_varlen_d, FFPA_INST_D)(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, hipStream_t stream) {
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return nt ? launch_varlen<T, FFPA_INST_D, true>(a, va, stream) : launch_varlen<T, FFPA_INST_D, false>(a, va, stream);
  });
}

}  // namespace ffpa
