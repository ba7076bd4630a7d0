// ffpa_mla_tree_fp8_inst.hip — TREE-MASK attention over an FP8 MLA latent cache: the verification step of tree speculative decoding (ffpa_mla_tree_inst.hip) over
// the cache of ffpa_mla_fp8_inst.hip (OCP e4m3 codes, ONE per-tensor scale, K = kv_scale x K8).  One translation unit per (D, dv) pair of FFPA_FOR_EACH_MLA_BUILD
// (compiled with -DFFPA_INST_D=<D>, q / O in bf16 + fp16, plain + NT); a TU of its own so that every other object stays what it was.  Entry point:
// ffpa_attn_varlen_mla_tree_fp8_fwd (ffpa_capi.hip); the step's new rows are written by the FP8 latent call's quantising append in front of it.
//
// The kernel is the latent kernel's text with BOTH hooks on: FFPA_M16_VARLEN_TREE (the element test of the tiles that hold a draft key reads the row's mask word)
// and FFPA_M16_KV_FP8 (a piece is an 8-byte register load, widened exactly and written to the LDS image behind PV).  The vector-memory queue of this build holds
// compiler-counted loads only — the tile's pieces and, in a draft tile, the mask word; there is no LDS-DMA and no L2 touch — so every wait on it is the compiler's
// own count and the text's dma_wait_* statements find what the FP8 latent build's find.  The two statements of the tree unit stand around the KV loop, the second
// one restated for the fourth argument struct of this build (MlaFp8Args: the value width AND the scale are epilogue arguments).  DESIGN.md section 22.
#include "ffpa_cu_seqlens_find.h"
#include "ffpa_fwd_kernel.h"
#include "ffpa_fwd_m16_kernel.h"
#include "ffpa_launch_kernel.h"
#include "ffpa_mla_tree_fp8.h"
#include "ffpa_paged.h"

#ifndef FFPA_INST_D
#error "compile with -DFFPA_INST_D=<head dim>"
#endif

namespace ffpa {

// The kernel's argument block as the kernel below declares it (by value, in this order), read through the constant address space: uniform loads are scalar loads.
struct MlaTreeFp8KernArgsBlock {
  FwdArgs a;
  VarlenArgs va;
  PagedArgs pa;
  MlaFp8Args ma;
};
static_assert(offsetof(MlaTreeFp8KernArgsBlock, va) == sizeof(FwdArgs) && offsetof(MlaTreeFp8KernArgsBlock, pa) == sizeof(FwdArgs) + sizeof(VarlenArgs) &&
                  offsetof(MlaTreeFp8KernArgsBlock, ma) == sizeof(FwdArgs) + sizeof(VarlenArgs) + sizeof(PagedArgs) &&
                  offsetof(MlaFp8Args, kv_scale) == sizeof(int) && sizeof(MlaFp8Args) == 2 * sizeof(int),
              "the argument block has no padding between the four structs, nor inside the fourth");
using MlaTreeFp8KernArgs = __attribute__((address_space(4))) const MlaTreeFp8KernArgsBlock*;

template <typename T, int D, bool NT = false>
__global__ __launch_bounds__(256) void ffpa_fwd_m16_mla_tree_fp8_kernel(const FwdArgs a_in, const VarlenArgs va_arg, const PagedArgs pa, const MlaFp8Args ma_arg) {
  static_assert(D > 512 && D % 128 == 64, "the MLA hook lives in the un-pipelined split-D loop of the tile text");
  VarlenArgs va = va_arg;  // (copies the epilogue refreshes from the kernel's argument block: FFPA_M16_KV_LOOP_EXIT below)
  MlaFp8Args ma = ma_arg;
#define FFPA_M16_VARLEN_TREE true
#define FFPA_M16_VARLEN_WINDOW false
#define FFPA_M16_VARLEN_SOFTCAP false
#define FFPA_M16_MLA_ON true
#define FFPA_M16_O_COLS ma.dv
#define FFPA_M16_KV_FP8 true
#define FFPA_M16_KV_SCALE ma.kv_scale
#define FFPA_M16_KV_FP8_LOAD(rsrc_, voff_) buffer_load_8<NT>((rsrc_), (voff_))
// The tree unit's statement in front of the KV loop (ffpa_mla_tree_inst.hip), unchanged: every vector load the compiler knows of is waited for on every path into
// the loop.  In this build that is the Q fragments' AND the prologue's pieces of tile t0 (the commit in front of it has consumed them): the queue is empty.
#define FFPA_M16_KV_LOOP_ENTRY dma_wait_all();
// The tree unit's statement behind the KV loop, for this build's fourth struct: what the epilogue reads of the kernel's arguments is read AGAIN from the argument
// block, through a pointer the compiler cannot see through, so that none of it is alive across the loop — the value width and, here, kv_scale (the factor of the
// epilogues' 1 / l; nothing in front of the epilogue reads it: the scores' share of it rides in FwdArgs::scale_log2).
#define FFPA_M16_KV_LOOP_EXIT                                                               \
  {                                                                                         \
    MlaTreeFp8KernArgs kargs_ = (MlaTreeFp8KernArgs)__builtin_amdgcn_kernarg_segment_ptr(); \
    asm volatile("" : "+s"(kargs_));                                                        \
    va.lse_stride_h = kargs_->va.lse_stride_h, va.pack = kargs_->va.pack;                   \
    va.o_tok_stride = kargs_->va.o_tok_stride;                                              \
    va.ws_head_rows = kargs_->va.ws_head_rows, va.ws_split_rows = kargs_->va.ws_split_rows; \
    ma.dv = kargs_->ma.dv, ma.kv_scale = kargs_->ma.kv_scale;                               \
    a.ws_o = kargs_->a.ws_o, a.ws_lse = kargs_->a.ws_lse, a.lse = kargs_->a.lse;            \
    a.so[1] = kargs_->a.so[1], a.so[2] = kargs_->a.so[2];                                   \
  }
#include "ffpa_fwd_m16_paged_body.inc"
#undef FFPA_M16_KV_LOOP_EXIT
#undef FFPA_M16_KV_LOOP_ENTRY
#undef FFPA_M16_KV_FP8_LOAD
#undef FFPA_M16_KV_SCALE
#undef FFPA_M16_KV_FP8
#undef FFPA_M16_O_COLS
#undef FFPA_M16_MLA_ON
#undef FFPA_M16_VARLEN_SOFTCAP
#undef FFPA_M16_VARLEN_WINDOW
#undef FFPA_M16_VARLEN_TREE
}

template <typename T, int D, bool NT>
static int launch_mla_tree_fp8(const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaFp8Args& ma, hipStream_t stream) {
  constexpr int BC = m16_block_keys(D, true);
  constexpr int LDS = 2 * BC * D * 2 + m16_exchange_bytes(D, 0);  // (the two 16-bit images of the latent kernel: the same LDS bytes)
  return launch_kernel<ffpa_fwd_m16_mla_tree_fp8_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa, ma);
}

int FFPA_CAT(launch_mla_tree_fp8_d, FFPA_INST_D)(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaFp8Args& ma,
                                                 hipStream_t stream) {
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return nt ? launch_mla_tree_fp8<T, FFPA_INST_D, true>(a, va, pa, ma, stream) : launch_mla_tree_fp8<T, FFPA_INST_D, false>(a, va, pa, ma, stream);
  });
}

}  // namespace ffpa
