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
#ifndef FFPA_M16_KV_GATHER  // (1: the keys of a tile are rows picked by an index list — ffpa_mla_sparse_inst.hip; see below)
#define FFPA_M16_KV_GATHER 0
#define FFPA_M16_PAGED_GATHER_DEFAULT
#endif
#include "ffpa_fwd_m16_head.inc"
#include "ffpa_fwd_m16_varlen_seq.inc"
  static_assert(BC == m16_block_keys(D, true), "the paged build's tile: 64 keys (32 at D > 512)");
#if FFPA_M16_KV_GATHER
  // ---- GATHERED KEYS (ffpa_mla_sparse_inst.hip): "sequence" seq is ONE query token, its block table is its row of the index list (pa.table, pa.bt_stride; pa.cap
  // = topk entries) and its page size is one row: key n of the token is pool row idx[n], clamped to [0, pa.num_pages).  There is no page-table state.  The pieces
  // of wave w cover exactly the keys 8 w .. 8 w + 7 of a tile (PPW pieces x 64 slots = 8 rows of D / 8 slots), so the wave keeps EIGHT wave-uniform row ids per
  // tile, read with scalar loads where the page ids are read in the other builds — the ids of tile j + 2 in front of barrier B of step j, waited for at the top of
  // step j + 1, where they turn into the PPW per-lane source offsets of that tile (krel[], which the pieces riding on QK^T(j + 1) read) and die:
  //     krel[i] = row id of the lane's key x row bytes + the lane's swizzled slot (g_sl[i], tile-invariant, the V map),
  // a piece spans at most two rows with a compile-time boundary lane.  A key at or past the token's count (a.Nkv) gets bit 31 — kDmaOob — instead of a row offset:
  // the descriptor spans the whole pool, at most 2^31 bytes (the launch side refuses larger ones), so such a lane is out of range, reads zeros and forms no address
  // whatever its entry holds.  Entries are read at min(n, pa.cap - 1): no read leaves the token's row of the list.
  // Over an FP8 pool (FFPA_M16_KV_FP8 of the tile text, set by ffpa_mla_sparse_fp8_inst.hip: one byte per element, the pieces are 8-byte register loads) the same
  // rule holds in the pool's bytes: a slot's 8 elements are 8 bytes of the source (g_sl: << 3), a row's D bytes end the span, and the row term is the BYTE row
  // stride — strides arrive in units of two bytes and k_row_bytes doubles them.  The sentinel is the same bit of the same 32-bit offset of the same descriptor.
  // Over the 656-byte FP8 rows of DeepSeek-V3.2 (FFPA_M16_KV_DS of the tile text, set by ffpa_mla_sparse_ds_inst.hip together with the three macros read here) a
  // row is no array of equal slots: slot s of the image lies at FFPA_M16_KV_DS_SLOT_OFF(s) bytes of the row — eight codes, or sixteen rotary bytes —, a row's
  // FFPA_M16_KV_DS_ROW_BYTES end the span, and g_sd[i] keeps what leads from the lane's slot of piece i to the scale of its 128 columns
  // (FFPA_M16_KV_DS_SCALE_DELTA; the scale load adds it to krel[i], sentinel and all).  The row term and the sentinel are the FP8 pool's.
#ifdef FFPA_M16_KV_FP8
#define FFPA_M16_GATHER_ESZ (FFPA_M16_KV_FP8 ? 1 : 2)
#else
#define FFPA_M16_GATHER_ESZ 2
#endif
#ifdef FFPA_M16_KV_DS
#define FFPA_M16_GATHER_ROW_BYTES FFPA_M16_KV_DS_ROW_BYTES
#define FFPA_M16_GATHER_SLOT_OFF(s_) FFPA_M16_KV_DS_SLOT_OFF(s_)
#else
#define FFPA_M16_GATHER_ROW_BYTES (D * FFPA_M16_GATHER_ESZ)
#define FFPA_M16_GATHER_SLOT_OFF(s_) ((s_) << (FFPA_M16_GATHER_ESZ == 1 ? 3 : 4))
#endif
  constexpr int kGSpr = D / 8;  // 16-byte slots per row (of the LDS image; 8 x FFPA_M16_GATHER_ESZ bytes of the source)
  static_assert(FFPA_M16_MLA_ON && PPW * 64 == 8 * kGSpr, "gathered keys: a wave's pieces of a tile are whole rows, eight of them");
  using cint_ptr = __attribute__((address_space(4))) const int*;  // (constant address space: a uniform load is a scalar load)
  const cint_ptr g_idx = (cint_ptr)(pa.table + (int64_t)seq * pa.bt_stride);
  const uint32_t g_span = (uint32_t)(pa.num_pages - 1) * ((uint32_t)a.sk[2] * 2u) + (uint32_t)FFPA_M16_GATHER_ROW_BYTES;  // bytes of a head's rows in the pool (<= 2^31: the launch side)
  int g_id[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the loaded row ids: this wave's keys of the tile whose offsets are formed next
  int g_next = 0;                          // first key of the tile whose ids are loaded next
  uint32_t g_sl[PPW];
#ifdef FFPA_M16_KV_DS
  uint32_t g_sd[PPW];
#endif
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int g = (wave * PPW + i) * 64 + lane;
    const int key = g / kGSpr;
    g_sl[i] = (uint32_t)FFPA_M16_GATHER_SLOT_OFF((g - key * kGSpr) ^ m16_v_swizzle<D>(key));
#ifdef FFPA_M16_KV_DS
    g_sd[i] = FFPA_M16_KV_DS_SCALE_DELTA((g - key * kGSpr) ^ m16_v_swizzle<D>(key));
#endif
  }
// (macros, not lambdas: they name krel[] and k_row_bytes of the tile text, and a lambda here would renumber the tile text's)
#define FFPA_M16_GATHER_LOAD(key0_)                                        \
  _Pragma("unroll") for (int gk_ = 0; gk_ < 8; ++gk_) {                    \
    const int ge_ = (key0_) + 8 * wave + gk_;                              \
    g_id[gk_] = g_idx[ge_ < pa.cap - 1 ? ge_ : pa.cap - 1];                \
  }
#define FFPA_M16_GATHER_FORM(key0_)                                                                        \
  {                                                                                                        \
    uint32_t g_ro_[8];                                                                                     \
    int g_left_ = a.Nkv - ((key0_) + 8 * wave); /* valid keys among the wave's eight */                    \
    _Pragma("unroll") for (int gk_ = 0; gk_ < 8; ++gk_) {                                                  \
      int id_ = g_id[gk_];                                                                                 \
      id_ = id_ > 0 ? id_ : 0;                                                                             \
      id_ = id_ < pa.num_pages - 1 ? id_ : pa.num_pages - 1;                                               \
      int oob_ = gk_ + 1 - g_left_; /* > 0: the key lies at or past the count */                           \
      oob_ = oob_ > 0 ? oob_ : 0;                                                                          \
      oob_ = oob_ < 1 ? oob_ : 1;                                                                          \
      g_ro_[gk_] = ((uint32_t)id_ * k_row_bytes) | ((uint32_t)oob_ << 31);                                 \
    }                                                                                                      \
    _Pragma("unroll") for (int gi_ = 0; gi_ < PPW; ++gi_) {                                                \
      const int lo_ = gi_ * 64 / kGSpr, hi_ = (gi_ * 64 + 63) / kGSpr;                                     \
      krel[gi_] = g_sl[gi_] + (lane < hi_ * kGSpr - gi_ * 64 ? g_ro_[lo_] : g_ro_[hi_]);                   \
    }                                                                                                      \
  }
#define FFPA_M16_KV_BEGIN(t0_)                               \
  if (nt > (t0_)) {                                          \
    FFPA_M16_GATHER_LOAD((t0_) * BC)                         \
    FFPA_M16_GATHER_FORM((t0_) * BC)                         \
    FFPA_M16_GATHER_LOAD((t0_) * BC + BC)                    \
    g_next = (t0_) * BC + 2 * BC;                            \
  }
#define FFPA_M16_KV_STEP(k0_)                                \
  __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0) */       \
  FFPA_M16_GATHER_FORM((k0_) + BC)
#define FFPA_M16_KV_STEP_END()                               \
  FFPA_M16_GATHER_LOAD(g_next)                               \
  g_next += BC;
#define FFPA_M16_KV_SRC(kind, slice, row_bytes, key0) gather_src((slice), g_span)
#else
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
#endif
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
#if FFPA_M16_KV_GATHER
#undef FFPA_M16_GATHER_FORM
#undef FFPA_M16_GATHER_LOAD
#undef FFPA_M16_GATHER_SLOT_OFF
#undef FFPA_M16_GATHER_ROW_BYTES
#undef FFPA_M16_GATHER_ESZ
#endif
#ifdef FFPA_M16_PAGED_GATHER_DEFAULT
#undef FFPA_M16_PAGED_GATHER_DEFAULT
#undef FFPA_M16_KV_GATHER
#endif
#undef FFPA_M16_KV_STEP_END
#undef FFPA_M16_KV_STEP
#undef FFPA_M16_KV_BEGIN
#undef FFPA_M16_PAGED
#undef FFPA_M16_DMA16
#undef FFPA_M16_MFMA
