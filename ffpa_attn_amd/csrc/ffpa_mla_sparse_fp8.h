// ffpa_mla_sparse_fp8.h — sparse (top-k indexed) attention over an FP8 (OCP e4m3) MLA latent pool (ffpa_attn_varlen_mla_sparse_fp8_fwd, ffpa_capi.hip): the
// launchers of ffpa_mla_sparse_fp8_inst.hip.  A header of its own so that every other object sees nothing of it.  The kernels take FwdArgs / VarlenArgs / PagedArgs
// as the sparse launch fills them (ffpa_mla_sparse.h: the index list stands where the block table stood) with the pool's strides in units of TWO BYTES, and
// MlaFp8Args (ffpa_mla_fp8.h: the value width and the per-tensor dequantisation factor) as the FP8 latent launch fills it.
#pragma once
#include <hip/hip_runtime.h>

#include "ffpa_mla_fp8.h"

namespace ffpa {

#define FFPA_DECL(D, DV) \
  int launch_mla_sparse_fp8_d##D(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaFp8Args& ma, hipStream_t stream);
FFPA_FOR_EACH_MLA_BUILD(FFPA_DECL)
#undef FFPA_DECL

}  // namespace ffpa
