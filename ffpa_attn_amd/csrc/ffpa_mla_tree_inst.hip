// ffpa_mla_tree_inst.hip — TREE-MASK attention over the MLA latent cache: the verification step of tree speculative decoding (an MTP head driven as an EAGLE draft
// model) for the models whose cache is one latent pool.  The Sq draft nodes of a sequence are the last rows of its latent cache; node i sees the whole prefix and,
// among the draft rows, what its 64-bit mask word says.  One translation unit per (D, dv) pair of FFPA_FOR_EACH_MLA_BUILD (compiled with -DFFPA_INST_D=<D>, bf16 +
// fp16, plain + NT); a TU of its own so that ffpa_mla_d<D>.o and every other object stay exactly what they were.  Entry point: ffpa_attn_varlen_mla_tree_fwd
// (ffpa_capi.hip).
//
// The kernel is a build of the latent kernel's text (ffpa_mla_inst.hip: ffpa_fwd_m16_paged_body.inc + ffpa_fwd_m16_tile.inc under FFPA_M16_MLA_ON) with the tree
// hook on as well (FFPA_M16_VARLEN_TREE -> FFPA_M16_TREE_ON / FFPA_M16_TREE_WORD at the split-D shared-softmax masking site).  It runs under the causal flag with
// causal_offset = L - ntok per sequence, so the tile walk, the KV ranges, the compact grid, row packing in chunks and the value-column epilogue are the causal
// latent launch's; only the element test of the tiles that hold a draft key (k0 + 32 - 1 >= causal_offset: up to three 32-key tiles) or end past the last key
// differs — there the row's word is loaded (a vector load: the one entry of the vmcnt queue that is no LDS-DMA piece; the compiler's wait for it, vmcnt(0), sits
// inside that branch and drains the pieces of tile j + 1 early, which barrier B of the same step would have waited for anyway).  Two statements of this unit stand
// around the KV loop (FFPA_M16_KV_LOOP_ENTRY in front of it, FFPA_M16_KV_LOOP_EXIT behind it: below).  DESIGN.md section 18.
#include "ffpa_cu_seqlens_find.h"
#include "ffpa_fwd_kernel.h"
#include "ffpa_fwd_m16_kernel.h"
#include "ffpa_launch_kernel.h"
#include "ffpa_mla_tree.h"
#include "ffpa_paged.h"

#ifndef FFPA_INST_D
#error "compile with -DFFPA_INST_D=<head dim>"
#endif

namespace ffpa {

// The kernel's argument block as the kernel below declares it (by value, in this order: the offsets are the code object's .args offsets 0 / 376 / 496 / 544), read
// through the constant address space: uniform loads are scalar loads.
struct MlaTreeKernArgsBlock {
  FwdArgs a;
  VarlenArgs va;
  PagedArgs pa;
  MlaArgs ma;
};
static_assert(offsetof(MlaTreeKernArgsBlock, va) == sizeof(FwdArgs) && offsetof(MlaTreeKernArgsBlock, pa) == sizeof(FwdArgs) + sizeof(VarlenArgs) &&
                  offsetof(MlaTreeKernArgsBlock, ma) == sizeof(FwdArgs) + sizeof(VarlenArgs) + sizeof(PagedArgs),
              "the argument block has no padding between the four structs");
using MlaTreeKernArgs = __attribute__((address_space(4))) const MlaTreeKernArgsBlock*;

template <typename T, int D, bool NT = false>
__global__ __launch_bounds__(256) void ffpa_fwd_m16_mla_tree_kernel(const FwdArgs a_in, const VarlenArgs va_arg, const PagedArgs pa, const MlaArgs ma_arg) {
  static_assert(D > 512 && D % 128 == 64, "the MLA hook lives in the un-pipelined split-D loop of the tile text");
  VarlenArgs va = va_arg;  // (copies the epilogue refreshes from the kernel's argument block: FFPA_M16_KV_LOOP_EXIT below)
  MlaArgs ma = ma_arg;
#define FFPA_M16_VARLEN_TREE true
#define FFPA_M16_VARLEN_WINDOW false
#define FFPA_M16_VARLEN_SOFTCAP false
#define FFPA_M16_MLA_ON true
#define FFPA_M16_O_COLS ma.dv
// Every vector load the compiler knows of — the Q fragments' — is waited for IN FRONT of the KV loop on every path into it.  Without this statement the compiler
// finds a path on which they are still in flight (the one that skips the prologue: a row tile without a KV tile, which never enters the loop) and puts its own
// vmcnt(0) in front of the first QK^T MFMA of EVERY step — where the queue holds the L2 touch issued a few instructions earlier, so each step waited for a
// round trip to memory (+ 16 ... 18 % where the touch misses: DESIGN.md section 18).  Behind the prologue's dma_wait_all the queue is empty: the wait costs nothing.
#define FFPA_M16_KV_LOOP_ENTRY dma_wait_all();
// What the epilogue reads of the kernel's arguments and nothing in front of it changed — the output and LSE bases' strides, the split workspace, the LSE pointer, the
// packed-row strides, the value width — is read AGAIN from the argument block behind the KV loop, through a pointer the compiler cannot see through.  The values
// are the same; what changes is that none of them is alive across the loop, where every scalar register is taken: without this the compiler parks ten scalar values in
// lanes of a vector register in front of the loop and reads them back behind it (.sgpr_spill_count 10, the latent kernel's figure).  A handful of scalar loads per
// workgroup, behind the last MFMA.
#define FFPA_M16_KV_LOOP_EXIT                                                               \
  {                                                                                         \
    MlaTreeKernArgs kargs_ = (MlaTreeKernArgs)__builtin_amdgcn_kernarg_segment_ptr();       \
    asm volatile("" : "+s"(kargs_));                                                        \
    va.lse_stride_h = kargs_->va.lse_stride_h, va.pack = kargs_->va.pack;                   \
    va.o_tok_stride = kargs_->va.o_tok_stride;                                              \
    va.ws_head_rows = kargs_->va.ws_head_rows, va.ws_split_rows = kargs_->va.ws_split_rows; \
    ma.dv = kargs_->ma.dv;                                                                  \
    a.ws_o = kargs_->a.ws_o, a.ws_lse = kargs_->a.ws_lse, a.lse = kargs_->a.lse;            \
    a.so[1] = kargs_->a.so[1], a.so[2] = kargs_->a.so[2];                                   \
  }
#include "ffpa_fwd_m16_paged_body.inc"
#undef FFPA_M16_KV_LOOP_EXIT
#undef FFPA_M16_KV_LOOP_ENTRY
#undef FFPA_M16_O_COLS
#undef FFPA_M16_MLA_ON
#undef FFPA_M16_VARLEN_SOFTCAP
#undef FFPA_M16_VARLEN_WINDOW
#undef FFPA_M16_VARLEN_TREE
}

template <typename T, int D, bool NT>
static int launch_mla_tree(const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaArgs& ma, hipStream_t stream) {
  constexpr int BC = m16_block_keys(D, true);
  constexpr int LDS = 2 * BC * D * 2 + m16_exchange_bytes(D, 0);  // (the two images of the latent kernel: the same LDS bytes)
  return launch_kernel<ffpa_fwd_m16_mla_tree_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa, ma);
}

int FFPA_CAT(launch_mla_tree_d, FFPA_INST_D)(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaArgs& ma, hipStream_t stream) {
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return nt ? launch_mla_tree<T, FFPA_INST_D, true>(a, va, pa, ma, stream) : launch_mla_tree<T, FFPA_INST_D, false>(a, va, pa, ma, stream);
  });
}

}  // namespace ffpa
