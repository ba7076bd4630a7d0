// ffpa_mla_sparse_fp8_inst.hip — SPARSE (top-k indexed) attention over an FP8 MLA latent pool: the sparse call of ffpa_mla_sparse_inst.hip over the pool of
// ffpa_mla_fp8_inst.hip (OCP e4m3 codes, ONE per-tensor scale, K = kv_scale x K8) — DeepSeek-V3.2's top-k attention as an engine with kv_cache_dtype = "fp8" issues
// it.  One translation unit per (D, dv) pair of FFPA_FOR_EACH_MLA_BUILD (compiled with -DFFPA_INST_D=<D>, q / O in bf16 + fp16, plain + NT); a TU of its own so
// that every other object stays what it was.  Entry point: ffpa_attn_varlen_mla_sparse_fp8_fwd (ffpa_capi.hip).
//
// The kernel is the latent kernel's text with BOTH hooks on: FFPA_M16_KV_GATHER (ffpa_fwd_m16_paged_body.inc: each wave reads the eight row ids of its keys of a
// tile with scalar loads and turns them into the per-lane source offsets krel[]) and FFPA_M16_KV_FP8 (ffpa_fwd_m16_tile.inc: a piece is an 8-byte register load at
// krel[], widened exactly and written to the LDS image where the 16-bit build's LDS-DMA piece lands).  Where the two meet, the gather counts the pool in bytes: a
// slot's 8 elements are 8 bytes of the source, a head's rows span (num_rows - 1) x row bytes + D bytes (<= 2^31: the launch side), and a key at or past the
// token's count keeps bit 31 in its offset — out of the descriptor's range for the 8-byte load as it was for the DMA, so the lane reads zeros and forms no address.
// DESIGN.md section 22.
#include "ffpa_cu_seqlens_find.h"
#include "ffpa_fwd_kernel.h"
#include "ffpa_fwd_m16_kernel.h"
#include "ffpa_launch_kernel.h"
#include "ffpa_mla_sparse_fp8.h"
#include "ffpa_paged.h"

#ifndef FFPA_INST_D
#error "compile with -DFFPA_INST_D=<head dim>"
#endif

namespace ffpa {

// Every tile of a head reads through ONE descriptor over the head's rows of the whole pool: `span` bytes from `pool` (<= 2^31, so that a lane offset with bit
// 31 set — kDmaOob — is out of range and zero-filled).
__device__ __forceinline__ TileSrc gather_src(const void* pool, uint32_t span) {
  TileSrc t;
  t.base = (const char*)pool;
  t.rows = 0;
  t.rsrc = make_rsrc(pool, span);
  return t;
}

// The kernel's argument block as the kernel below declares it (by value, in this order), read through the constant address space: uniform loads are scalar loads.
struct MlaSparseFp8KernArgsBlock {
  FwdArgs a;
  VarlenArgs va;
  PagedArgs pa;
  MlaFp8Args ma;
};
static_assert(offsetof(MlaSparseFp8KernArgsBlock, va) == sizeof(FwdArgs) && offsetof(MlaSparseFp8KernArgsBlock, pa) == sizeof(FwdArgs) + sizeof(VarlenArgs) &&
                  offsetof(MlaSparseFp8KernArgsBlock, ma) == sizeof(FwdArgs) + sizeof(VarlenArgs) + sizeof(PagedArgs) &&
                  offsetof(MlaFp8Args, kv_scale) == sizeof(int) && sizeof(MlaFp8Args) == 2 * sizeof(int),
              "the argument block has no padding between the four structs, nor inside the fourth");
using MlaSparseFp8KernArgs = __attribute__((address_space(4))) const MlaSparseFp8KernArgsBlock*;

template <typename T, int D, bool NT = false>
__global__ __launch_bounds__(256) void ffpa_fwd_m16_mla_sparse_fp8_kernel(const FwdArgs a_in, const VarlenArgs va_arg, const PagedArgs pa, const MlaFp8Args ma_arg) {
  static_assert(D > 512 && D % 128 == 64, "the MLA hook lives in the un-pipelined split-D loop of the tile text");
  VarlenArgs va = va_arg;  // (copies the epilogue refreshes from the kernel's argument block: FFPA_M16_KV_LOOP_EXIT below)
  MlaFp8Args ma = ma_arg;
#define FFPA_M16_VARLEN_TREE false
#define FFPA_M16_VARLEN_WINDOW false
#define FFPA_M16_VARLEN_SOFTCAP false
#define FFPA_M16_MLA_ON true
#define FFPA_M16_O_COLS ma.dv
#define FFPA_M16_KV_GATHER 1
#define FFPA_M16_KV_FP8 true
#define FFPA_M16_KV_SCALE ma.kv_scale
#define FFPA_M16_KV_FP8_LOAD(rsrc_, voff_) buffer_load_8<NT>((rsrc_), (voff_))
// The tree unit's statement behind the KV loop (ffpa_mla_tree_inst.hip, which says why), taken by this build as well: with the eight row ids next to the FP8
// build's scalars the loop has no scalar register to spare, and without it the compiler parks epilogue arguments in lanes of a vector register in front of the
// loop.  What the epilogue reads of the kernel's arguments — kv_scale among it — is read again from the argument block behind the loop instead.
#define FFPA_M16_KV_LOOP_EXIT                                                                   \
  {                                                                                             \
    MlaSparseFp8KernArgs kargs_ = (MlaSparseFp8KernArgs)__builtin_amdgcn_kernarg_segment_ptr(); \
    asm volatile("" : "+s"(kargs_));                                                            \
    va.lse_stride_h = kargs_->va.lse_stride_h, va.pack = kargs_->va.pack;                       \
    va.o_tok_stride = kargs_->va.o_tok_stride;                                                  \
    va.ws_head_rows = kargs_->va.ws_head_rows, va.ws_split_rows = kargs_->va.ws_split_rows;     \
    ma.dv = kargs_->ma.dv, ma.kv_scale = kargs_->ma.kv_scale;                                   \
    a.ws_o = kargs_->a.ws_o, a.ws_lse = kargs_->a.ws_lse, a.lse = kargs_->a.lse;                \
    a.so[1] = kargs_->a.so[1], a.so[2] = kargs_->a.so[2];                                       \
  }
#include "ffpa_fwd_m16_paged_body.inc"
#undef FFPA_M16_KV_LOOP_EXIT
#undef FFPA_M16_KV_FP8_LOAD
#undef FFPA_M16_KV_SCALE
#undef FFPA_M16_KV_FP8
#undef FFPA_M16_KV_GATHER
#undef FFPA_M16_O_COLS
#undef FFPA_M16_MLA_ON
#undef FFPA_M16_VARLEN_SOFTCAP
#undef FFPA_M16_VARLEN_WINDOW
#undef FFPA_M16_VARLEN_TREE
}

template <typename T, int D, bool NT>
static int launch_mla_sparse_fp8(const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaFp8Args& ma, hipStream_t stream) {
  constexpr int BC = m16_block_keys(D, true);
  constexpr int LDS = 2 * BC * D * 2 + m16_exchange_bytes(D, 0);  // (the two 16-bit images of the latent kernel: the same LDS bytes)
  return launch_kernel<ffpa_fwd_m16_mla_sparse_fp8_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa, ma);
}

int FFPA_CAT(launch_mla_sparse_fp8_d, FFPA_INST_D)(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaFp8Args& ma,
                                                   hipStream_t stream) {
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return nt ? launch_mla_sparse_fp8<T, FFPA_INST_D, true>(a, va, pa, ma, stream) : launch_mla_sparse_fp8<T, FFPA_INST_D, false>(a, va, pa, ma, stream);
  });
}

}  // namespace ffpa
