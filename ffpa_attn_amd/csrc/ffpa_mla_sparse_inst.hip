// ffpa_mla_sparse_inst.hip — SPARSE (top-k indexed) attention over the MLA latent cache (DeepSeek-V3.2's "DeepSeek Sparse Attention" in its absorbed decode form,
// FlashMLA's sparse decode call): every query token brings its own list of latent rows — slots of the pool, shared by all heads of the token — and attends to
// those rows only.  One translation unit per (D, dv) pair of FFPA_FOR_EACH_MLA_BUILD (compiled with -DFFPA_INST_D=<D>, bf16 + fp16, plain + NT); a TU of its
// own so that ffpa_mla_d<D>.o and every other object stay exactly what they were.  Entry point: ffpa_attn_varlen_mla_sparse_fwd (ffpa_capi.hip).
//
// The kernel is a build of the latent kernel's text (ffpa_mla_inst.hip: ffpa_fwd_m16_paged_body.inc + ffpa_fwd_m16_tile.inc under FFPA_M16_MLA_ON) with one more
// hook on, FFPA_M16_KV_GATHER: a token is a sequence of ONE query token over a paged cache whose page size is one row, its block table is its index row and its
// length the number of valid entries.  The hook replaces the page-table state and the per-tile descriptor: each wave reads the eight row ids of ITS keys of a
// tile with scalar loads and turns them into the per-lane source offsets of its LDS-DMA pieces (ffpa_fwd_m16_paged_body.inc).  Everything behind the fetch — one
// LDS image per tile, the two-barrier step and its counted waits (the id loads are scalar: they do not enter the vmcnt queue), row packing of a group wider than
// the tile, KV ranges and the merge, the value-column epilogue — is the latent kernel's text unchanged.  The L2 touch of the tile after next is off in this build.
#include "ffpa_cu_seqlens_find.h"
#include "ffpa_fwd_kernel.h"
#include "ffpa_fwd_m16_kernel.h"
#include "ffpa_launch_kernel.h"
#include "ffpa_mla_sparse.h"
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

template <typename T, int D, bool NT = false>
__global__ __launch_bounds__(256) void ffpa_fwd_m16_mla_sparse_kernel(const FwdArgs a_in, const VarlenArgs va, const PagedArgs pa, const MlaArgs ma) {
  static_assert(D > 512 && D % 128 == 64, "the MLA hook lives in the un-pipelined split-D loop of the tile text");
#define FFPA_M16_VARLEN_TREE false
#define FFPA_M16_VARLEN_WINDOW false
#define FFPA_M16_VARLEN_SOFTCAP false
#define FFPA_M16_MLA_ON true
#define FFPA_M16_O_COLS ma.dv
#define FFPA_M16_KV_GATHER 1
#include "ffpa_fwd_m16_paged_body.inc"
#undef FFPA_M16_KV_GATHER
#undef FFPA_M16_O_COLS
#undef FFPA_M16_MLA_ON
#undef FFPA_M16_VARLEN_SOFTCAP
#undef FFPA_M16_VARLEN_WINDOW
#undef FFPA_M16_VARLEN_TREE
}

template <typename T, int D, bool NT>
static int launch_mla_sparse(const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaArgs& ma, hipStream_t stream) {
  constexpr int BC = m16_block_keys(D, true);
  constexpr int LDS = 2 * BC * D * 2 + m16_exchange_bytes(D, 0);  // (the two images of the latent kernel: the same LDS bytes)
  return launch_kernel<ffpa_fwd_m16_mla_sparse_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa, ma);
}

int FFPA_CAT(launch_mla_sparse_d, FFPA_INST_D)(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaArgs& ma, hipStream_t stream) {
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return nt ? launch_mla_sparse<T, FFPA_INST_D, true>(a, va, pa, ma, stream) : launch_mla_sparse<T, FFPA_INST_D, false>(a, va, pa, ma, stream);
  });
}

}  // namespace ffpa
