// ffpa_mla_tree.h — tree-mask attention over the MLA latent cache (ffpa_attn_varlen_mla_tree_fwd, ffpa_capi.hip): the launchers of ffpa_mla_tree_inst.hip.  A header
// of its own so that every other object sees nothing of it.  The kernels take the latent kernel's four argument structs (ffpa_mla.h, ffpa_paged.h) as the latent
// launch fills them, with VarlenArgs::tree_bits / tree_stride / tree_tokens set as the two-cache tree launch sets them.
#pragma once
#include <hip/hip_runtime.h>

#include "ffpa_mla.h"

namespace ffpa {

#define FFPA_DECL(D, DV) int launch_mla_tree_d##D(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaArgs& ma, hipStream_t stream);
FFPA_FOR_EACH_MLA_BUILD(FFPA_DECL)
#undef FFPA_DECL

}  // namespace ffpa
