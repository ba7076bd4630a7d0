// ffpa_mla_variant.inc — THE SHELL of the MLA latent-cache kernels: included once by each ffpa_mla*_inst.hip behind the unit's switch list, it makes that
// variant's kernel, the exported launcher launch_<stem>_d<FFPA_INST_D> and what the two need.  The variants and what their switches mean: ffpa_mla.h
// (FFPA_FOR_EACH_MLA_VARIANT — the unit's list is checked against its row below).
//
//     #define FFPA_MLA_STEM mla_tree          the row's stem: ffpa_fwd_m16_<stem>_kernel, launch_<stem>_d<D>
//     #define FFPA_MLA_TREE 1                 the tree mask
//     #define FFPA_MLA_GATHER 0               keys through a list of pool rows, not a page table
//     #define FFPA_MLA_POOL FFPA_MLA_POOL_..  what a latent row is made of
//     #define FFPA_MLA_EXIT_REFRESH 1         the epilogue's arguments are read again behind the KV loop
//     #include "ffpa_mla_variant.inc"
//
// Every kernel is ONE text, the paged twin of the packed-sequence kernel (ffpa_fwd_m16_paged_body.inc + ffpa_fwd_m16_tile.inc) under the tile text's MLA hook
// (FFPA_M16_MLA_ON): the two LDS images of the tile, Kt and Vt, alternate as the home of ONE latent tile — tile j lives in image j & 1, QK^T(j) reads its K fragments
// there and PV(j) its V^T fragments from the same bytes; only O columns < dv are stored.  The switches turn further hooks of the two texts on; everything behind
// the fetch — the two-barrier step, row packing in chunks, KV ranges + merge, the compact grid, the value-column epilogue — is the same in all of them, and so are
// the LDS bytes (the two 16-bit images of the latent tile, whatever the pool holds).  DESIGN.md section 25; the measurements behind the notes below: sections 17, 18, 20, 22, 23.
#if !defined(FFPA_MLA_STEM) || !defined(FFPA_MLA_TREE) || !defined(FFPA_MLA_GATHER) || !defined(FFPA_MLA_POOL) || !defined(FFPA_MLA_EXIT_REFRESH)
#error "define the variant's five switches (ffpa_mla.h: FFPA_FOR_EACH_MLA_VARIANT) in front of ffpa_mla_variant.inc"
#endif
#ifndef FFPA_INST_D
#error "compile with -DFFPA_INST_D=<head dim>"
#endif

#include "ffpa_cu_seqlens_find.h"
#include "ffpa_fwd_kernel.h"
#include "ffpa_fwd_m16_kernel.h"
#include "ffpa_launch_kernel.h"
#include "ffpa_mla_fp8.h"
#include "ffpa_paged.h"
#if FFPA_MLA_POOL == FFPA_MLA_POOL_DS
#include "ffpa_mla_sparse_ds.h"
#endif

namespace ffpa {

#define FFPA_MLA_KERNEL FFPA_CAT(FFPA_CAT(ffpa_fwd_m16_, FFPA_MLA_STEM), _kernel)
static_assert(kMlaVariants[FFPA_CAT(kMlaVariant_, FFPA_MLA_STEM)].tree == (FFPA_MLA_TREE != 0) &&
                  kMlaVariants[FFPA_CAT(kMlaVariant_, FFPA_MLA_STEM)].gather == (FFPA_MLA_GATHER != 0) &&
                  kMlaVariants[FFPA_CAT(kMlaVariant_, FFPA_MLA_STEM)].pool == FFPA_MLA_POOL &&
                  kMlaVariants[FFPA_CAT(kMlaVariant_, FFPA_MLA_STEM)].exit_refresh == (FFPA_MLA_EXIT_REFRESH != 0),
              "the unit's switch list is not its row of FFPA_FOR_EACH_MLA_VARIANT (ffpa_mla.h)");

// The kernel's fourth argument struct: the value width and, for a pool under one per-tensor scale, the scale.  (The 656-byte rows carry their scales: MlaArgs.)
#if FFPA_MLA_POOL == FFPA_MLA_POOL_E4M3
#define FFPA_MLA_ARGS MlaFp8Args
#else
#define FFPA_MLA_ARGS MlaArgs
#endif

#if FFPA_MLA_GATHER
// THE GATHER (FFPA_M16_KV_GATHER, ffpa_fwd_m16_paged_body.inc): a token is a sequence of ONE query token over a paged cache whose page size is one row, its block
// table is its index row and its length the number of valid entries.  The hook replaces the page-table state and the per-tile descriptor: each wave reads the eight
// row ids of ITS keys of a tile with scalar loads (they do not enter the vmcnt queue) and turns them into the per-lane source offsets of its pieces.  The L2 touch
// of the tile after next is off.  The gather counts the pool IN BYTES: over an e4m3 pool a slot's 8 elements are 8 bytes of the source and a head's rows span
// (num_rows - 1) x row bytes + D bytes; over 656-byte rows the span is (num_rows - 1) x row stride + 656 (<= 2^31 either way: the launch side).  A key at or past
// the token's count keeps bit 31 in its offset — out of the descriptor's range for a register load as for the LDS-DMA, so the lane reads zeros and forms no address.
//   Every tile of a head reads through ONE descriptor over the head's rows of the whole pool: `span` bytes from `pool` (<= 2^31, so that a lane offset with bit
//   31 set — kDmaOob — is out of range and zero-filled).
__device__ __forceinline__ TileSrc gather_src(const void* pool, uint32_t span) {
  TileSrc t;
  t.base = (const char*)pool;
  t.rows = 0;
  t.rsrc = make_rsrc(pool, span);
  return t;
}
#endif

#if FFPA_MLA_EXIT_REFRESH
// The kernel's argument block as the kernel below declares it (by value, in this order: the offsets are the code object's .args offsets 0 / 376 / 496 / 544), read
// through the constant address space: uniform loads are scalar loads.
struct MlaKernArgsBlock {
  FwdArgs a;
  VarlenArgs va;
  PagedArgs pa;
  FFPA_MLA_ARGS ma;
};
static_assert(offsetof(MlaKernArgsBlock, va) == sizeof(FwdArgs) && offsetof(MlaKernArgsBlock, pa) == sizeof(FwdArgs) + sizeof(VarlenArgs) &&
                  offsetof(MlaKernArgsBlock, ma) == sizeof(FwdArgs) + sizeof(VarlenArgs) + sizeof(PagedArgs) && offsetof(MlaFp8Args, kv_scale) == sizeof(int) &&
                  sizeof(MlaFp8Args) == 2 * sizeof(int) && sizeof(MlaArgs) == sizeof(int),
              "the argument block has no padding between the four structs, nor inside the fourth");
using MlaKernArgs = __attribute__((address_space(4))) const MlaKernArgsBlock*;
#endif

template <typename T, int D, bool NT = false>
#if FFPA_MLA_EXIT_REFRESH
__global__ __launch_bounds__(256) void FFPA_MLA_KERNEL(const FwdArgs a_in, const VarlenArgs va_arg, const PagedArgs pa, const FFPA_MLA_ARGS ma_arg) {
#else
__global__ __launch_bounds__(256) void FFPA_MLA_KERNEL(const FwdArgs a_in, const VarlenArgs va, const PagedArgs pa, const FFPA_MLA_ARGS ma) {
#endif
#if FFPA_MLA_POOL == FFPA_MLA_POOL_DS
  static_assert(D == 576 && std::is_same_v<T, __bf16>, "the row format: 512 quantised + 64 bf16 rotary columns");
#else
  static_assert(D > 512 && D % 128 == 64, "the MLA hook lives in the un-pipelined split-D loop of the tile text");
#endif
#if FFPA_MLA_EXIT_REFRESH
  VarlenArgs va = va_arg;  // (copies the epilogue refreshes from the kernel's argument block: FFPA_M16_KV_LOOP_EXIT below)
  FFPA_MLA_ARGS ma = ma_arg;
#endif
#define FFPA_M16_VARLEN_WINDOW false
#define FFPA_M16_VARLEN_SOFTCAP false
#define FFPA_M16_MLA_ON true
#define FFPA_M16_O_COLS ma.dv

#if FFPA_MLA_TREE
// THE TREE MASK (FFPA_M16_VARLEN_TREE -> FFPA_M16_TREE_ON / FFPA_M16_TREE_WORD at the split-D shared-softmax masking site): the kernel runs under the causal flag
// with causal_offset = L - ntok per sequence, so the tile walk, the KV ranges, the compact grid, row packing in chunks and the value-column epilogue are the causal
// latent launch's; only the element test of the tiles that hold a draft key (k0 + 32 - 1 >= causal_offset: up to three 32-key tiles) or end past the last key
// differs — there the row's word is loaded (a vector load the compiler counts; its wait, vmcnt(0), sits inside that branch and drains the pieces of tile j + 1
// early, which barrier B of the same step would have waited for anyway).
#define FFPA_M16_VARLEN_TREE true
// ... and THE WAIT IN FRONT OF THE KV LOOP that goes with it: every vector load the compiler knows of — the Q fragments' and, over a pool the kernel loads into
// registers, the prologue's pieces of tile t0 (the commit in front has consumed them) — is waited for on every path into the loop.  Without this statement the
// compiler finds a path on which they are still in flight (the one that skips the prologue: a row tile without a KV tile, which never enters the loop) and puts its
// own vmcnt(0) in front of the first QK^T MFMA of EVERY step — where the queue holds the L2 touch issued a few instructions earlier, so each step waited for a
// round trip to memory (+ 16 ... 18 % where the touch misses: DESIGN.md section 18).  Behind the prologue's dma_wait_all the queue is empty: the wait costs nothing.
#define FFPA_M16_KV_LOOP_ENTRY dma_wait_all();
#else
#define FFPA_M16_VARLEN_TREE false
#endif

#if FFPA_MLA_GATHER
#define FFPA_M16_KV_GATHER 1
#endif

#if FFPA_MLA_POOL != FFPA_MLA_POOL_16BIT
// A POOL OF E4M3 CODES (FFPA_M16_KV_FP8, ffpa_fwd_m16_tile.inc).  There is no FP8 arithmetic: every e4m3 value is exactly a bf16 and exactly an fp16, so the kernel
// stages a tile's bytes in registers (8-byte loads the compiler counts: no LDS-DMA, no L2 touch), widens them and writes the EXACT 16-bit image of the tile to LDS
// where the LDS-DMA pieces of the 16-bit build land.  The one scale never touches an element: the scores are (softmax_scale x kv_scale) q.K8 — the factor rides in
// FwdArgs::scale_log2 — and O is multiplied by kv_scale once, in the epilogues' 1 / l.
#define FFPA_M16_KV_FP8 true
#endif
#if FFPA_MLA_POOL == FFPA_MLA_POOL_E4M3
#define FFPA_M16_KV_SCALE ma.kv_scale
#define FFPA_M16_KV_FP8_LOAD(rsrc_, voff_) buffer_load_8<NT>((rsrc_), (voff_))
#elif FFPA_MLA_POOL == FFPA_MLA_POOL_DS
// THE 656-BYTE ROWS (FFPA_M16_KV_DS; the format: ffpa_mla_sparse_ds.h) change three things.  The gather maps a lane's source slot s of the 576-wide image to the
// row's bytes — ds_slot_off: eight codes at 8 s, or sixteen rotary bytes at 528 + 16 (s - 64) — and keeps per piece the distance from there to the slot's scale
// (ds_scale_delta); the image's swizzle permutes inside 8-slot groups and the NoPE / rotary border (slot 64) is a group border, so whether a lane handles a NoPE or
// a rotary slot of piece i depends on (i, lane) alone.  A piece is one 16-byte register load and one dword scale load per lane, both at row id x row bytes | the
// "no row" bit + a lane constant: a key at or past the token's count forms no address on EITHER load and yields codes 0 under scale 0, i.e. zeros.  The commit
// behind PV(j) writes one ds_write_b128 per lane and piece: a rotary lane the raw sixteen bytes, a NoPE lane ds_nope_widen of its eight codes.  Nothing is folded
// into the softmax scale or the epilogue (the scale is 1): the kernel computes on unpack_latent_rows_ds(pool), to the bit.
#define FFPA_M16_KV_SCALE 1.f
#define FFPA_M16_KV_FP8_LOAD(rsrc_, voff_) u32x2{0u, 0u}  // (not issued by this build: its pieces are the two loads below)
#define FFPA_M16_KV_DS true
#define FFPA_M16_KV_DS_ROW_BYTES kDsRowBytes
#define FFPA_M16_KV_DS_SLOT_OFF(s_) ds_slot_off(s_)
#define FFPA_M16_KV_DS_SCALE_DELTA(s_) ds_scale_delta(s_)
#define FFPA_M16_KV_DS_LOAD(rsrc_, voff_) buffer_load_16<NT>((rsrc_), (voff_))
#define FFPA_M16_KV_DS_LOAD_SCALE(rsrc_, voff_, i_) buffer_load_f32<NT>((rsrc_), (voff_) + g_sd[i_])
#define FFPA_M16_KV_DS_WIDEN(raw_, scale_) ds_nope_widen((raw_), (scale_))
#endif

#if FFPA_MLA_EXIT_REFRESH
// THE REFRESH BEHIND THE KV LOOP: what the epilogue reads of the kernel's arguments and nothing in front of it changed — the output and LSE bases' strides, the split
// workspace, the LSE pointer, the packed-row strides, the value width and, under one per-tensor scale, kv_scale (the factor of the epilogues' 1 / l) — is read AGAIN
// from the argument block, through a pointer the compiler cannot see through.  The values are the same; what changes is that none of them is alive across the loop.
// Where every scalar register of the loop is taken — the tree builds; the gather's eight row ids next to a register-loaded pool's scalars — the compiler otherwise
// parks ten scalar values in lanes of a vector register in front of the loop and reads them back behind it (.sgpr_spill_count 10, the plain latent kernel's
// figure).  A handful of scalar loads per workgroup, behind the last MFMA.  On or off per variant as measured: ffpa_mla.h.
#if FFPA_MLA_POOL == FFPA_MLA_POOL_E4M3
#define FFPA_MLA_REFRESH_MA ma.dv = kargs_->ma.dv, ma.kv_scale = kargs_->ma.kv_scale
#else
#define FFPA_MLA_REFRESH_MA ma.dv = kargs_->ma.dv
#endif
#define FFPA_M16_KV_LOOP_EXIT                                                               \
  {                                                                                         \
    MlaKernArgs kargs_ = (MlaKernArgs)__builtin_amdgcn_kernarg_segment_ptr();               \
    asm volatile("" : "+s"(kargs_));                                                        \
    va.lse_stride_h = kargs_->va.lse_stride_h, va.pack = kargs_->va.pack;                   \
    va.o_tok_stride = kargs_->va.o_tok_stride;                                              \
    va.ws_head_rows = kargs_->va.ws_head_rows, va.ws_split_rows = kargs_->va.ws_split_rows; \
    FFPA_MLA_REFRESH_MA;                                                                    \
    a.ws_o = kargs_->a.ws_o, a.ws_lse = kargs_->a.ws_lse, a.lse = kargs_->a.lse;            \
    a.so[1] = kargs_->a.so[1], a.so[2] = kargs_->a.so[2];                                   \
  }
#endif

#include "ffpa_fwd_m16_paged_body.inc"
}

// The launcher: the same LDS bytes in every variant (the two 16-bit images of the latent tile); a kernel that takes MlaArgs gets the value width alone.
template <typename T, int D, bool NT>
static int launch_mla_variant(const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaFp8Args& ma, hipStream_t stream) {
  constexpr int BC = m16_block_keys(D, true);
  constexpr int LDS = 2 * BC * D * 2 + m16_exchange_bytes(D, 0);
#if FFPA_MLA_POOL == FFPA_MLA_POOL_E4M3
  return launch_kernel<FFPA_MLA_KERNEL<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa, ma);
#else
  return launch_kernel<FFPA_MLA_KERNEL<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa, MlaArgs{ma.dv});
#endif
}

int FFPA_CAT(FFPA_CAT(launch_, FFPA_MLA_STEM), FFPA_CAT(_d, FFPA_INST_D))(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa,
                                                                          const MlaFp8Args& ma, hipStream_t stream) {
#if FFPA_MLA_POOL == FFPA_MLA_POOL_DS
  if (dtype != 0) return -4;  // (bf16 only — the rotary bytes of a row reach the image as they are —: dispatch_dtype's "no such dtype")
  return nt ? launch_mla_variant<__bf16, FFPA_INST_D, true>(a, va, pa, ma, stream) : launch_mla_variant<__bf16, FFPA_INST_D, false>(a, va, pa, ma, stream);
#else
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return nt ? launch_mla_variant<T, FFPA_INST_D, true>(a, va, pa, ma, stream) : launch_mla_variant<T, FFPA_INST_D, false>(a, va, pa, ma, stream);
  });
#endif
}

// (the hooks of the two texts are this unit's alone: nothing behind the shell sees them)
#undef FFPA_M16_KV_LOOP_EXIT
#undef FFPA_MLA_REFRESH_MA
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
#undef FFPA_M16_KV_LOOP_ENTRY
#undef FFPA_M16_O_COLS
#undef FFPA_M16_MLA_ON
#undef FFPA_M16_VARLEN_SOFTCAP
#undef FFPA_M16_VARLEN_WINDOW
#undef FFPA_M16_VARLEN_TREE
#undef FFPA_MLA_ARGS
#undef FFPA_MLA_KERNEL

}  // namespace ffpa
