// ffpa_mla_sparse_ds_inst.hip — SPARSE (top-k indexed) attention over the 656-byte FP8 latent rows of DeepSeek-V3.2 (ffpa_mla_sparse_ds.h: 512 e4m3 codes, four
// float32 scales — one per 128 columns —, 64 bf16 rotary columns): the sparse FP8 call of ffpa_mla_sparse_fp8_inst.hip over the row format in which the engines
// that serve that model keep its cache.  One translation unit per (D, dv) pair of FFPA_FOR_EACH_MLA_BUILD (compiled with -DFFPA_INST_D=<D>; bf16 ONLY — the rotary
// bytes of the pool are bf16 and are copied raw into the image —, plain + NT); a TU of its own so that every other object stays what it was.  Entry point:
// ffpa_attn_varlen_mla_sparse_ds_fwd (ffpa_capi.hip).
//
// The kernel is the sparse FP8 kernel's structure — the MLA, the gather and the FP8 hook on, FFPA_M16_KV_LOOP_EXIT as there — with one more hook for the row format,
// FFPA_M16_KV_DS:
//   * the gather (ffpa_fwd_m16_paged_body.inc) maps a lane's source slot s of the 576-wide image to the row's bytes — ds_slot_off: eight codes at 8 s, or sixteen
//     rotary bytes at 528 + 16 (s - 64) — and keeps per piece the distance from there to the slot's scale (ds_scale_delta).  The image's swizzle permutes inside
//     8-slot groups and the NoPE / rotary border (slot 64) is a group border: whether a lane handles a NoPE or a rotary slot of piece i depends on (i, lane) alone;
//   * a piece (ffpa_fwd_m16_tile.inc) is one 16-byte register load and one dword scale load per lane, both at row id x row bytes | the "no row" bit + a lane
//     constant: a key at or past the token's count forms no address on EITHER load and yields codes 0 under scale 0, i.e. zeros;
//   * the commit behind PV(j) writes one ds_write_b128 per lane and piece: a rotary lane the raw sixteen bytes, a NoPE lane ds_nope_widen of its eight codes.
// Nothing is folded into the softmax scale or the epilogue (FFPA_M16_KV_SCALE is 1): the kernel computes on unpack_latent_rows_ds(pool), to the bit.
// The descriptor spans (num_rows - 1) x row stride + 656 bytes (<= 2^31: the launch side).  DESIGN.md section 23.
#include "ffpa_cu_seqlens_find.h"
#include "ffpa_fwd_kernel.h"
#include "ffpa_fwd_m16_kernel.h"
#include "ffpa_launch_kernel.h"
#include "ffpa_mla_sparse_ds.h"
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
struct MlaSparseDsKernArgsBlock {
  FwdArgs a;
  VarlenArgs va;
  PagedArgs pa;
  MlaArgs ma;
};
static_assert(offsetof(MlaSparseDsKernArgsBlock, va) == sizeof(FwdArgs) && offsetof(MlaSparseDsKernArgsBlock, pa) == sizeof(FwdArgs) + sizeof(VarlenArgs) &&
                  offsetof(MlaSparseDsKernArgsBlock, ma) == sizeof(FwdArgs) + sizeof(VarlenArgs) + sizeof(PagedArgs),
              "the argument block has no padding between the four structs");
using MlaSparseDsKernArgs = __attribute__((address_space(4))) const MlaSparseDsKernArgsBlock*;

template <typename T, int D, bool NT = false>
__global__ __launch_bounds__(256) void ffpa_fwd_m16_mla_sparse_ds_kernel(const FwdArgs a_in, const VarlenArgs va_arg, const PagedArgs pa, const MlaArgs ma_arg) {
  static_assert(D == 576 && std::is_same_v<T, __bf16>, "the row format: 512 quantised + 64 bf16 rotary columns");
  VarlenArgs va = va_arg;  // (copies the epilogue refreshes from the kernel's argument block: FFPA_M16_KV_LOOP_EXIT below)
  MlaArgs ma = ma_arg;
#define FFPA_M16_VARLEN_TREE false
#define FFPA_M16_VARLEN_WINDOW false
#define FFPA_M16_VARLEN_SOFTCAP false
#define FFPA_M16_MLA_ON true
#define FFPA_M16_O_COLS ma.dv
#define FFPA_M16_KV_GATHER 1
#define FFPA_M16_KV_FP8 true
#define FFPA_M16_KV_SCALE 1.f
#define FFPA_M16_KV_FP8_LOAD(rsrc_, voff_) u32x2{0u, 0u}  // (not issued by this build: its pieces are the two loads below)
#define FFPA_M16_KV_DS true
#define FFPA_M16_KV_DS_ROW_BYTES kDsRowBytes
#define FFPA_M16_KV_DS_SLOT_OFF(s_) ds_slot_off(s_)
#define FFPA_M16_KV_DS_SCALE_DELTA(s_) ds_scale_delta(s_)
#define FFPA_M16_KV_DS_LOAD(rsrc_, voff_) buffer_load_16<NT>((rsrc_), (voff_))
#define FFPA_M16_KV_DS_LOAD_SCALE(rsrc_, voff_, i_) buffer_load_f32<NT>((rsrc_), (voff_) + g_sd[i_])
#define FFPA_M16_KV_DS_WIDEN(raw_, scale_) ds_nope_widen((raw_), (scale_))
// The sparse FP8 unit's statement behind the KV loop (ffpa_mla_sparse_fp8_inst.hip, which says why), taken by this build as well.
#define FFPA_M16_KV_LOOP_EXIT                                                                 \
  {                                                                                           \
    MlaSparseDsKernArgs kargs_ = (MlaSparseDsKernArgs)__builtin_amdgcn_kernarg_segment_ptr(); \
    asm volatile("" : "+s"(kargs_));                                                          \
    va.lse_stride_h = kargs_->va.lse_stride_h, va.pack = kargs_->va.pack;                     \
    va.o_tok_stride = kargs_->va.o_tok_stride;                                                \
    va.ws_head_rows = kargs_->va.ws_head_rows, va.ws_split_rows = kargs_->va.ws_split_rows;   \
    ma.dv = kargs_->ma.dv;                                                                    \
    a.ws_o = kargs_->a.ws_o, a.ws_lse = kargs_->a.ws_lse, a.lse = kargs_->a.lse;              \
    a.so[1] = kargs_->a.so[1], a.so[2] = kargs_->a.so[2];                                     \
  }
#include "ffpa_fwd_m16_paged_body.inc"
#undef FFPA_M16_KV_LOOP_EXIT
#undef FFPA_M16_KV_DS_WIDEN
#undef FFPA_M16_KV_DS_LOAD_SCALE
#undef FFPA_M16_KV_DS_LOAD
#undef FFPA_M16_KV_DS_SCALE_DELTA
#undef FFPA_M16_KV_DS_SLOT_OFF
#undef FFPA_M16_KV_DS_ROW_BYTES
#undef FFPA_M16_KV_DS
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

template <int D, bool NT>
static int launch_mla_sparse_ds(const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaArgs& ma, hipStream_t stream) {
  constexpr int BC = m16_block_keys(D, true);
  constexpr int LDS = 2 * BC * D * 2 + m16_exchange_bytes(D, 0);  // (the two 16-bit images of the latent kernel: the same LDS bytes)
  return launch_kernel<ffpa_fwd_m16_mla_sparse_ds_kernel<__bf16, D, NT>>(a.total_wg, LDS, stream, a, va, pa, ma);
}

int FFPA_CAT(launch_mla_sparse_ds_d, FFPA_INST_D)(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaArgs& ma,
                                                  hipStream_t stream) {
  if (dtype != 0) return -4;  // (bf16 only: dispatch_dtype's "no such dtype")
  return nt ? launch_mla_sparse_ds<FFPA_INST_D, true>(a, va, pa, ma, stream) : launch_mla_sparse_ds<FFPA_INST_D, false>(a, va, pa, ma, stream);
}

}  // namespace ffpa
