// ffpa_fwd_m16_varlen_body.inc — the body of the packed-sequence kernel (ffpa_fwd_m16_kernel.h), included once per kernel of that family: ffpa_fwd_m16_varlen_kernel
// (FFPA_M16_VARLEN_TREE false: the tree hooks of the tile text fold away, the kernel is what it was) and ffpa_fwd_m16_varlen_tree_kernel (true: the element test of
// the tiles that hold a draft key reads VarlenArgs::tree_bits) and ffpa_fwd_m16_varlen_window_kernel (FFPA_M16_VARLEN_WINDOW true: the tile range, the element test and
// the KV ranges' share-out take a sliding window, VarlenArgs::window) and ffpa_fwd_m16_varlen_softcap_kernel (the window build with FFPA_M16_VARLEN_SOFTCAP true: both
// softmax sites cap the scores, VarlenArgs::softcap_in).  Text moved out of the kernel, nothing changed.
  constexpr int MK = 0;  // no attn_bias, no mask ranges: what the reference's packed entry point accepts
  constexpr bool DROP = false;
#define FFPA_M16_MFMA std::conditional_t<NT, Mfma16Nt<T>, Mfma16<T>>
#define FFPA_M16_DMA16 LdsDma16<NT>::template at
#include "ffpa_fwd_m16_head.inc"
#include "ffpa_fwd_m16_varlen_seq.inc"
#define FFPA_M16_TILE_DONE return
#define FFPA_M16_ROW_INV(l) ((l) > 0.f ? __builtin_amdgcn_rcpf(l) : 0.f)
#define FFPA_M16_ROW_OUT(x, rh) (l_tot[rh] > 0.f ? (T)((x) * inv[rh]) : (T)0.f)  // (the select BEHIND product + conversion: those stay the dense kernel's one instruction — fp16: v_fma_mixlo, one rounding — and its bits)
#define FFPA_M16_LSE_INDEX(row) (va.pack ? (int64_t)(hq * va.pack + (row) / ntok) * va.lse_stride_h + q_lo + (row) % ntok : (int64_t)hq * va.lse_stride_h + q_lo + (row))
// (the KV-split workspace of the packed call: [split, query head, token] rows — ffpa_varlen_merge_kernel reads them back by (head, token))
#define FFPA_M16_WS_ROW(row) ((int64_t)split * va.ws_split_rows + (va.pack ? (int64_t)(hq * va.pack + (row) / ntok) * va.ws_head_rows + q_lo + (row) % ntok : (int64_t)hq * va.ws_head_rows + q_lo + (row)))
// (packed rows: a.sq[2] / a.so[2] are the HEAD strides of q / o, a token is q_tok_stride / o_tok_stride further; rows are tokens: ntok-independent)
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
#undef FFPA_M16_DMA16
#undef FFPA_M16_MFMA
