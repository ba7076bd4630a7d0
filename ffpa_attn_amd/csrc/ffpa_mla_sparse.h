// ffpa_mla_sparse.h — sparse (top-k indexed) attention over the MLA latent cache (ffpa_attn_varlen_mla_sparse_fwd, ffpa_capi.hip): the launchers of
// ffpa_mla_sparse_inst.hip.  A header of its own so that every other object sees nothing of it.  The kernels take the latent kernel's four argument structs
// (ffpa_mla.h, ffpa_paged.h) — PagedArgs read as an index list: table = indices, bt_stride = its row stride, cap = topk, num_pages = rows of the pool, page_size = 1
// (k_page_stride / v_page_stride / tiles_per_page are not read).
#pragma once
#include <hip/hip_runtime.h>

#include "ffpa_mla.h"

namespace ffpa {

#define FFPA_DECL(D, DV) int launch_mla_sparse_d##D(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaArgs& ma, hipStream_t stream);
FFPA_FOR_EACH_MLA_BUILD(FFPA_DECL)
#undef FFPA_DECL

}  // namespace ffpa
