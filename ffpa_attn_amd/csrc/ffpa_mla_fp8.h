// ffpa_mla_fp8.h — the FP8 (OCP e4m3) build of the MLA latent-cache call (ffpa_attn_varlen_mla_fp8_fwd, ffpa_capi.hip): what its kernels take beyond the latent
// call's structs (ffpa_mla.h) and the quantising appends' launchers (ffpa_mla_fp8_inst.hip).  The attention launchers of every variant: ffpa_mla.h.
#pragma once
#include "ffpa_mla.h"

namespace ffpa {

// What the FP8 latent kernel needs beyond FwdArgs / VarlenArgs / PagedArgs: the value width (MlaArgs::dv) and the per-tensor dequantisation factor, K = kv_scale x K8.
// The pool holds one byte per element; the kernel's text multiplies every K stride by two (it was written for 16-bit elements), so the launch side hands
// FwdArgs::sk / sv and PagedArgs::k_page_stride / v_page_stride in units of TWO BYTES (the C entry point requires rows, heads and pages that are multiples of 16
// elements).  FwdArgs::scale_log2 carries softmax_scale x kv_scale; kv_scale itself multiplies O once, in the epilogues.
struct MlaFp8Args {
  int dv;
  float kv_scale;
};

// The quantising appends: MlaAppendArgs / MlaAppendVarlenArgs as the 16-bit appends read them — kv_new in q's dtype (bf16 / fp16), the pool's strides in ELEMENTS
// of the pool, i.e. bytes — and inv = float32(1 / kv_scale), made on the host.  Every element is stored once as
//     rne_e4m3(clamp(float32(x) * inv, -448, +448)),   NaN stays NaN (+-inf saturates).
struct MlaFp8AppendArgs {
  MlaAppendArgs a;
  float inv;
};
struct MlaFp8AppendVarlenArgs {
  MlaAppendVarlenArgs va;
  float inv;
};

int launch_mla_fp8_append(int dtype, const MlaFp8AppendArgs& a, hipStream_t stream);
int launch_mla_fp8_append_varlen(int dtype, const MlaFp8AppendVarlenArgs& va, hipStream_t stream);

}  // namespace ffpa
