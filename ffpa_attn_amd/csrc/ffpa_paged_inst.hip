// ffpa_paged_inst.hip — the paged-KV twin of the packed-sequence kernel (ffpa_fwd_m16_paged_kernel), one translation unit per head dim (compiled with
// -DFFPA_INST_D=<D>, D a multiple of 64 in [128, 1024]; bf16 + fp16 in the same TU).  A TU of its own so that the dense and packed objects
// (ffpa_fwd_inst.hip, ffpa_varlen_inst.hip) stay exactly what they were.  Entry point: ffpa_attn_varlen_paged_fwd (ffpa_capi.hip).
#include "ffpa_fwd_kernel.h"
#include "ffpa_fwd_m16_kernel.h"
#include "ffpa_launch_kernel.h"
#include "ffpa_paged.h"

#ifndef FFPA_INST_D
#error "compile with -DFFPA_INST_D=<head dim>"
#endif

namespace ffpa {

// PAGED KV CACHE (vLLM / SGLang / FlashAttention's flash_attn_with_kvcache(block_table=...)): K and V live in a pool of pages of page_size keys; sequence i's keys
// are its row of the block table, in key order.  The same kernel as ffpa_fwd_m16_varlen_kernel — the same sequence lookup (ffpa_fwd_m16_varlen_seq.inc), workgroup
// order, GQA row packing, KV splits, compact grid and NT build, the same tile text — but for where a K / V tile comes from: its descriptor's base is the tile's
// page (FFPA_M16_KV_SRC below) instead of the sequence's contiguous rows.  page_size is a multiple of 64 and the tiles here hold 64 keys (32 at D > 512: the
// packed kernel's 128-key tile of D = 256 / 320 is not taken, the choice the builds with a bias make), so a tile never straddles two pages.
//
// PAGE IDS IN SGPRs, ONE STEP AHEAD.  A step j touches three tiles: V(j), K(j + 1) and — the split-D tiles — K1(j + 2) / the L2 touch of tile j + 2.  Their page
// ids (clamped to [0, num_pages)) and tile-in-page indices sit in three scalar slots for tiles j .. j + 2, shifted by one at the top of every step
// (FFPA_M16_KV_STEP), where the id of tile j + 2 comes from the slot `nx` that was loaded at the END of step j - 1 (FFPA_M16_KV_STEP_END, in front of barrier B:
// its scalar load lands while the waves wait there).  The explicit lgkmcnt(0) at the top of a step retires it at a point where no LDS read is in flight, so the
// compiler's own waits inside the MFMA chains never have a scalar load to wait for.  Table entries past a sequence's last used page are never read (the tile
// index is clamped to its last page; tiles past the last key have an empty descriptor and move no bytes).
template <typename T, int D, bool NT = false>
__global__ __launch_bounds__(256) void ffpa_fwd_m16_paged_kernel(const FwdArgs a_in, const VarlenArgs va, const PagedArgs pa) {
#define FFPA_M16_VARLEN_TREE false
#define FFPA_M16_VARLEN_WINDOW false
#define FFPA_M16_VARLEN_SOFTCAP false
#include "ffpa_fwd_m16_paged_body.inc"
#undef FFPA_M16_VARLEN_SOFTCAP
#undef FFPA_M16_VARLEN_WINDOW
#undef FFPA_M16_VARLEN_TREE
}

// ... and under a TREE MASK (ffpa_attn_varlen_tree_fwd with a pool): a kernel of its own from the same text, as ffpa_fwd_m16_varlen_tree_kernel
template <typename T, int D, bool NT = false>
__global__ __launch_bounds__(256) void ffpa_fwd_m16_paged_tree_kernel(const FwdArgs a_in, const VarlenArgs va, const PagedArgs pa) {
#define FFPA_M16_VARLEN_TREE true
#define FFPA_M16_VARLEN_WINDOW false
#define FFPA_M16_VARLEN_SOFTCAP false
#include "ffpa_fwd_m16_paged_body.inc"
#undef FFPA_M16_VARLEN_SOFTCAP
#undef FFPA_M16_VARLEN_WINDOW
#undef FFPA_M16_VARLEN_TREE
}

// ... and under a SLIDING WINDOW (ffpa_attn_varlen_window_fwd with a pool), as ffpa_fwd_m16_varlen_window_kernel: the page lookahead starts at the row tile's
// first walked tile (FFPA_M16_KV_BEGIN takes any tile), so the pages in front of the window are never looked up
template <typename T, int D, bool NT = false>
__global__ __launch_bounds__(256) void ffpa_fwd_m16_paged_window_kernel(const FwdArgs a_in, const VarlenArgs va, const PagedArgs pa) {
#define FFPA_M16_VARLEN_TREE false
#define FFPA_M16_VARLEN_WINDOW true
#define FFPA_M16_VARLEN_SOFTCAP false
#include "ffpa_fwd_m16_paged_body.inc"
#undef FFPA_M16_VARLEN_SOFTCAP
#undef FFPA_M16_VARLEN_WINDOW
#undef FFPA_M16_VARLEN_TREE
}

// ... and with LOGIT SOFT-CAPPING (ffpa_attn_varlen_softcap_fwd with a pool), as ffpa_fwd_m16_varlen_softcap_kernel: the window build with the cap hook on
template <typename T, int D, bool NT = false>
__global__ __launch_bounds__(256) void ffpa_fwd_m16_paged_softcap_kernel(const FwdArgs a_in, const VarlenArgs va, const PagedArgs pa) {
#define FFPA_M16_VARLEN_TREE false
#define FFPA_M16_VARLEN_WINDOW true
#define FFPA_M16_VARLEN_SOFTCAP true
#include "ffpa_fwd_m16_paged_body.inc"
#undef FFPA_M16_VARLEN_SOFTCAP
#undef FFPA_M16_VARLEN_WINDOW
#undef FFPA_M16_VARLEN_TREE
}

template <typename T, int D, bool NT>
static int launch_paged(const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, hipStream_t stream) {
  constexpr int BC = m16_block_keys(D, true);
  constexpr int LDS = 2 * BC * D * 2 + m16_exchange_bytes(D, 0);
  if (va.tree_tokens != 0) return launch_kernel<ffpa_fwd_m16_paged_tree_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa);  // (under a tree mask: its own build)
  if (va.softcap_in > 0.f) return launch_kernel<ffpa_fwd_m16_paged_softcap_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa);  // (capped scores: the window build with the cap)
  if (va.window != 0) return launch_kernel<ffpa_fwd_m16_paged_window_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa);  // (under a sliding window: its own build)
  return launch_kernel<ffpa_fwd_m16_paged_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa);
}

int FFPA_CAT(launch_paged_d, FFPA_INST_D)(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, hipStream_t stream) {
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return nt ? launch_paged<T, FFPA_INST_D, true>(a, va, pa, stream) : launch_paged<T, FFPA_INST_D, false>(a, va, pa, stream);
  });
}

}  // namespace ffpa
