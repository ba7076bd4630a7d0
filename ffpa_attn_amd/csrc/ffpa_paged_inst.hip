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

// tile_src (ffpa_common.h) for a tile whose first row is `tile_base` (its page's row): the same row count and span — rows past the sequence's last key read as
// zeros, a tile at or past the end moves no bytes
template <int BC>
__device__ __forceinline__ TileSrc tile_src_at(const char* tile_base, uint32_t row_bytes, int key0, int nkv, uint32_t RB) {
  const int kc = key0 < nkv ? key0 : nkv;
  int rows = nkv - kc;
  rows = rows < BC ? rows : BC;
  const uint32_t span = (uint32_t)(rows < 1 ? rows : 1) * ((uint32_t)(rows - 1) * row_bytes + (uint32_t)RB);
  TileSrc t;
  t.base = tile_base;
  t.rows = rows;
  t.rsrc = make_rsrc(t.base, span);
  return t;
}

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
  constexpr int MK = 0;  // no attn_bias, no mask ranges
  constexpr bool DROP = false;
#define FFPA_M16_MFMA std::conditional_t<NT, Mfma16Nt<T>, Mfma16<T>>
#define FFPA_M16_DMA16 LdsDma16<NT>::template at
#define FFPA_M16_PAGED 1
#include "ffpa_fwd_m16_head.inc"
#include "ffpa_fwd_m16_varlen_seq.inc"
  static_assert(BC == m16_block_keys(D, true), "the paged build's tile: 64 keys (32 at D > 512)");
  // ---- page-table state (all wave-uniform, scalar)
  using cint_ptr = __attribute__((address_space(4))) const int*;  // (constant address space: a uniform load is a scalar load)
  const cint_ptr tbl = (cint_ptr)(pa.table + (int64_t)seq * pa.bt_stride);
  const int last_page = a.Nkv > 0 ? (a.Nkv - 1) / pa.page_size : 0;
  const uint64_t k_ps = (uint64_t)pa.k_page_stride * 2u, v_ps = (uint64_t)pa.v_page_stride * 2u;  // bytes between two pages
  const uint64_t pf_ps = ((wave & 1) == 0) ? k_ps : v_ps;  // (the L2 touch: even waves K, odd waves V — the tile text's pf_k)
  int nx_page = 0, nx_sub = 0;  // page index / tile in page of the next tile whose id is loaded
  int nx_id = 0, nx_s = 0;      // the loaded slot
  int s_id[3] = {0, 0, 0}, s_sub[3] = {0, 0, 0};
  int pg_k0 = 0;  // first key of the tile in slot 0
  auto pg_load = [&]() __attribute__((always_inline)) {
    nx_id = tbl[nx_page < last_page ? nx_page : last_page];
    nx_s = nx_sub;
    if (++nx_sub == pa.tiles_per_page) nx_sub = 0, ++nx_page;
  };
  auto pg_shift = [&]() __attribute__((always_inline)) {
    s_id[0] = s_id[1], s_sub[0] = s_sub[1];
    s_id[1] = s_id[2], s_sub[1] = s_sub[2];
    s_id[2] = nx_id, s_sub[2] = nx_s;
  };
  // byte offset of the tile starting at key0 (one of k0, k0 + BC, k0 + 2 BC of the current step: folds to a slot) from the head's base in page 0
  auto pg_off = [&](int key0, uint64_t page_bytes, uint32_t row_bytes) __attribute__((always_inline)) -> uint64_t {
    const int d = key0 == pg_k0 ? 0 : key0 == pg_k0 + BC ? 1 : 2;
    int id = d == 0 ? s_id[0] : d == 1 ? s_id[1] : s_id[2];
    const int sub = d == 0 ? s_sub[0] : d == 1 ? s_sub[1] : s_sub[2];
    id = id > 0 ? id : 0;
    id = id < pa.num_pages - 1 ? id : pa.num_pages - 1;
    return (uint64_t)(uint32_t)id * page_bytes + (uint64_t)((uint32_t)(sub * BC) * row_bytes);
  };
// the tile text's hooks: KV_BEGIN(t0) before its first K / V piece, KV_STEP(k0) at the top of a KV step, KV_STEP_END in front of barrier B, KV_SRC = a tile's
// descriptor (kind 0: K, 1: V, 2: the L2 touch of this wave)
#define FFPA_M16_KV_BEGIN(t0_)                               \
  if (nt > (t0_)) {                                          \
    nx_page = (t0_) / pa.tiles_per_page;                     \
    nx_sub = (t0_) - nx_page * pa.tiles_per_page;            \
    pg_load();                                               \
    pg_shift();                                              \
    pg_load();                                               \
    pg_shift();                                              \
    pg_load();                                               \
    pg_k0 = (t0_) * BC - BC;                                 \
  }
#define FFPA_M16_KV_STEP(k0_)                                \
  __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0) */       \
  pg_shift();                                                \
  pg_k0 = (k0_);
#define FFPA_M16_KV_STEP_END() pg_load();
#define FFPA_M16_KV_SRC(kind, slice, row_bytes, key0)                                                                                    \
  tile_src_at<BC>((const char*)(slice) + pg_off((key0), (kind) == 0 ? k_ps : (kind) == 1 ? v_ps : pf_ps, (row_bytes)), (row_bytes), (key0), \
                  a.Nkv, rb_valid)
#define FFPA_M16_TILE_DONE return
#define FFPA_M16_ROW_INV(l) ((l) > 0.f ? __builtin_amdgcn_rcpf(l) : 0.f)
#define FFPA_M16_ROW_OUT(x, rh) (l_tot[rh] > 0.f ? (T)((x) * inv[rh]) : (T)0.f)
#define FFPA_M16_LSE_INDEX(row) (va.pack ? (int64_t)(hq * va.pack + (row) / ntok) * va.lse_stride_h + q_lo + (row) % ntok : (int64_t)hq * va.lse_stride_h + q_lo + (row))
#define FFPA_M16_WS_ROW(row) ((int64_t)split * va.ws_split_rows + (va.pack ? (int64_t)(hq * va.pack + (row) / ntok) * va.ws_head_rows + q_lo + (row) % ntok : (int64_t)hq * va.ws_head_rows + q_lo + (row)))
#define FFPA_M16_Q_ROW_OFF(row) (va.pack ? (int64_t)((row) / ntok) * a.sq[2] + (int64_t)((row) % ntok) * va.q_tok_stride : (int64_t)(row) * a.sq[2])
#define FFPA_M16_O_ROW_OFF(row) (va.pack ? (int64_t)((row) / ntok) * a.so[2] + (int64_t)((row) % ntok) * va.o_tok_stride : (int64_t)(row) * a.so[2])
#include "ffpa_fwd_m16_tile.inc"
#undef FFPA_M16_O_ROW_OFF
#undef FFPA_M16_Q_ROW_OFF
#undef FFPA_M16_WS_ROW
#undef FFPA_M16_LSE_INDEX
#undef FFPA_M16_ROW_OUT
#undef FFPA_M16_ROW_INV
#undef FFPA_M16_TILE_DONE
#undef FFPA_M16_KV_SRC
#undef FFPA_M16_KV_STEP_END
#undef FFPA_M16_KV_STEP
#undef FFPA_M16_KV_BEGIN
#undef FFPA_M16_PAGED
#undef FFPA_M16_DMA16
#undef FFPA_M16_MFMA
}

template <typename T, int D, bool NT>
static int launch_paged(const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, hipStream_t stream) {
  constexpr int BC = m16_block_keys(D, true);
  constexpr int LDS = 2 * BC * D * 2 + m16_exchange_bytes(D, 0);
  return launch_kernel<ffpa_fwd_m16_paged_kernel<T, D, NT>>(a.total_wg, LDS, stream, a, va, pa);
}

int FFPA_CAT(launch_paged_d, FFPA_INST_D)(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, hipStream_t stream) {
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return nt ? launch_paged<T, FFPA_INST_D, true>(a, va, pa, stream) : launch_paged<T, FFPA_INST_D, false>(a, va, pa, stream);
  });
}

}  // namespace ffpa
