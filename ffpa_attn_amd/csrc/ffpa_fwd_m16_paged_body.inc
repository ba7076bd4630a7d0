// ffpa_fwd_m16_paged_body.inc — the body of the paged-KV twin of the packed-sequence kernel (ffpa_paged_inst.hip), included once per kernel of that family:
// ffpa_fwd_m16_paged_kernel (FFPA_M16_VARLEN_TREE false) and ffpa_fwd_m16_paged_tree_kernel (true: under a tree mask, VarlenArgs::tree_bits); ffpa_fwd_m16_paged_window_kernel has FFPA_M16_VARLEN_WINDOW true (a sliding
// window, VarlenArgs::window: the walk — and the page lookahead — start at the row tile's first windowed tile); ffpa_fwd_m16_paged_softcap_kernel is that build with
// FFPA_M16_VARLEN_SOFTCAP true (capped scores, VarlenArgs::softcap_in).  Text moved out of the
// kernel, nothing changed.
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
#define FFPA_M16_TREE_ON FFPA_M16_VARLEN_TREE
#define FFPA_M16_TREE_WORD(tok, pin) FFPA_M16_VARLEN_TREE_WORD(tok, pin)
#define FFPA_M16_WINDOW_ON FFPA_M16_VARLEN_WINDOW
#define FFPA_M16_WINDOW_SPAN va.win_span
#define FFPA_M16_SOFTCAP_ON FFPA_M16_VARLEN_SOFTCAP
#define FFPA_M16_SOFTCAP_IN va.softcap_in
#include "ffpa_fwd_m16_tile.inc"
#undef FFPA_M16_SOFTCAP_IN
#undef FFPA_M16_SOFTCAP_ON
#undef FFPA_M16_WINDOW_SPAN
#undef FFPA_M16_WINDOW_ON
#undef FFPA_M16_TREE_WORD
#undef FFPA_M16_TREE_ON
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
