// ffpa_mla_tree_fp8.h — tree-mask attention over an FP8 (OCP e4m3) MLA latent cache (ffpa_attn_varlen_mla_tree_fp8_fwd, ffpa_capi.hip): the launchers of
// ffpa_mla_tree_fp8_inst.hip.  A header of its own so that every other object sees nothing of it.  The kernels take FwdArgs / VarlenArgs / PagedArgs as the tree
// latent launch fills them (ffpa_mla_tree.h: VarlenArgs::tree_bits / tree_stride / tree_tokens set) with the cache's strides in units of TWO BYTES, and MlaFp8Args
// (ffpa_mla_fp8.h) as the FP8 latent launch fills it.  The step's new rows are written by the FP8 latent call's quantising append (launch_mla_fp8_append).
#pragma once
#include <hip/hip_runtime.h>

#include "ffpa_mla_fp8.h"

namespace ffpa {

#define FFPA_DECL(D, DV) \
  int launch_mla_tree_fp8_d##D(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaFp8Args& ma, hipStream_t stream);
FFPA_FOR_EACH_MLA_BUILD(FFPA_DECL)
#undef FFPA_DECL

}  // namespace ffpa
