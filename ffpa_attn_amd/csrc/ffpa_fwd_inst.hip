// ffpa_fwd_inst.hip — one translation unit per head dim (compiled with
// -DFFPA_INST_D=<D>); keeps hipcc invocations small and parallel.  The reference
// generates one TU per (dtype, acc, headdim, stage) from env.py:455-521; here the
// only axis is the head dim (bf16 + fp16 in the same TU).
#include "ffpa_fwd_kernel.h"
#include "ffpa_fwd_m16_kernel.h"
#include "ffpa_fwd_m16w_kernel.h"
#include "ffpa_launch.h"
#include "ffpa_launch_kernel.h"

#ifndef FFPA_INST_D
#error "compile with -DFFPA_INST_D=<head dim>"
#endif

namespace ffpa {

template <typename T, int D, int ND, bool SAFE, bool DROP = false, bool BTILE = false, int MK = 1>
static int launch_one(const FwdArgs& a, hipStream_t stream) {
  constexpr int BC = (ND == 1) ? ((D <= FFPA_BC128_MAX_D && !BTILE) ? 128 : 64) : splitd_block_keys(D, ND);
  constexpr int LDS_BASE = 2 * BC * D * 2 + splitd_exchange_bytes(D, ND);
  const int LDS = LDS_BASE + (a.bias_lds > 0 ? a.bias_lds : -a.bias_lds);  // + the key-bias row cache or the bias-tile staging area, sized by the C-ABI layer (<= 160 KiB in total)
  return launch_kernel<ffpa_fwd_split_d_kernel<T, D, ND, SAFE, DROP, BTILE, MK>>(a.total_wg, LDS, stream, a);
}

// The prefill kernel on the 16x16x32 MFMA shape (ffpa_fwd_m16_kernel.h): every prefill launch at head dims >= FFPA_M16_MIN_D.
template <typename T, int D, int MK, bool DROP = false, bool PAIR = false>
static int launch_m16(const FwdArgs& a, hipStream_t stream) {
  if constexpr (MK == 0 && !PAIR) {
    if (a.pair_tiles) return launch_m16<T, D, MK, DROP, true>(a, stream);  // (the kernel whose workgroups walk two row tiles: causal launches, ffpa_capi.hip::pick_pair_tiles)
  }
  constexpr int BC = m16_block_keys(D, MK == 1 || MK == 3);
  constexpr int LDS_BASE = 2 * BC * D * 2 + m16_exchange_bytes(D, MK);
  const int LDS = LDS_BASE + (a.bias_lds > 0 ? a.bias_lds : -a.bias_lds);  // + the key-bias row cache or the bias-tile staging areas, sized by the C-ABI layer (<= 160 KiB in total)
  if constexpr (PAIR) return launch_kernel<ffpa_fwd_m16_pair_kernel<T, D, DROP>>(a.total_wg, LDS, stream, a);
  else return launch_kernel<ffpa_fwd_m16_kernel<T, D, MK, DROP>>(a.total_wg, LDS, stream, a);
}

// The wide-row prefill tile of the head dims whose O^T leaves accumulator registers idle at 32 rows per wave (ffpa_fwd_m16w_kernel.h).
template <typename T, int D, int MK>
static int launch_m16w(const FwdArgs& a, hipStream_t stream) {
  if constexpr (m16w_available(D)) {
    return launch_kernel<ffpa_fwd_m16w_kernel<T, D, m16w_row_halves(D), m16w_block_keys(D), MK>>(a.total_wg, m16w_lds_bytes(D), stream, a);
  } else {
    return -3;
  }
}

// Which kernel a launch runs (also reported by ffpa_attn_fwd_plan: FFPA_KERNEL_* in include/ffpa_attn.h):
//   short-query tiles (variant 1)           -> ffpa_fwd_split_d_kernel<ND = 4 / 2>  (32x32x16 MFMA, split-KV)
//   prefill, head dim >= FFPA_M16_MIN_D     -> ffpa_fwd_m16_kernel<MK, DROP>        (16x16x32 MFMA): the one prefill family of the large head dims
//                                              (MK: 0 no bias, 2 boolean mask / ranges, 3 key bias from the LDS row cache, 1 any other additive bias or mask)
//   prefill, smaller head dims              -> ffpa_fwd_split_d_kernel<ND = 1>      (32x32x16 MFMA)
// (a template, so that `if constexpr` really discards the other family's instantiations)
template <int D>
static int launch_fwd_impl(int dtype, int safe, int variant, const FwdArgs& a, hipStream_t stream) {
  constexpr int ND = (D <= 512) ? 1 : 2;
  // short-query launches: D split over all 4 waves (one 32-row block per workgroup) when the D/4
  // slice is a whole number of 32-column O blocks, else over 2 waves (two row blocks)
  constexpr int NDS = (D % 128 == 0) ? 4 : 2;
  const bool drop = a.dropout_p > 0.f;
  const bool no_bias = a.bias_dtype == 0 && a.kv_bounds == nullptr;  // no attn_bias, no mask ranges: the builds without any bias path
  const bool mask_only = a.bias_dtype == 4 || a.bias_dtype == 0;     // boolean mask and / or mask ranges: the builds that carry only that path
  if (safe) {  // the register-staged twin of the prefill tiles: the test library's bf16 build, nothing else
#ifdef FFPA_INST_SAFE
    if (variant != 1 && !drop && dtype == 0) return launch_one<__bf16, D, ND, true>(a, stream);
#endif
    return -3;
  }
  if (variant == 3 && (drop || !mask_only)) return -3;  // the wide-row tile (the plan only picks it for the builds that exist: no additive bias, no dropout)
  return dispatch_dtype(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    if (variant == 1) return drop ? launch_one<T, D, NDS, false, true>(a, stream) : launch_one<T, D, NDS, false>(a, stream);
    if (variant == 3) return no_bias ? launch_m16w<T, D, 0>(a, stream) : launch_m16w<T, D, 2>(a, stream);
    if constexpr (D >= FFPA_M16_MIN_D) {
      if (drop) return no_bias ? launch_m16<T, D, 0, true>(a, stream) : launch_m16<T, D, 1, true>(a, stream);
      if (no_bias) return launch_m16<T, D, 0>(a, stream);
      if (mask_only) return launch_m16<T, D, 2>(a, stream);
      if (a.bias_lds > 0 && a.kv_bounds == nullptr) return launch_m16<T, D, 3>(a, stream);  // a key bias that fits the LDS row cache, nothing else: the lean key-bias build
      return launch_m16<T, D, 1>(a, stream);
    } else {
      if (drop) return launch_one<T, D, ND, false, true>(a, stream);
      // 16-bit bias with a row axis, staged through LDS one step ahead (the build with 64-key tiles at every head dim, so that the
      // LDS holds the bias tiles next to K and V; the plan of the C-ABI layer uses tile_config variant 2 for these launches)
      if (a.bias_tile) return launch_one<T, D, ND, false, false, true>(a, stream);
      if (no_bias) return launch_one<T, D, ND, false, false, false, 0>(a, stream);
      if (mask_only) return launch_one<T, D, ND, false, false, false, 2>(a, stream);
      return launch_one<T, D, ND, false>(a, stream);
    }
  });
}

int FFPA_CAT(launch_fwd_d, FFPA_INST_D)(int dtype, int safe, int variant, const FwdArgs& a, hipStream_t stream) {
  return launch_fwd_impl<FFPA_INST_D>(dtype, safe, variant, a, stream);
}

void FFPA_CAT(tile_config_d, FFPA_INST_D)(int variant, int* br, int* bc, int* lds) {
  constexpr int D = FFPA_INST_D;
  // variant 0: prefill tiles, 1: short-query tiles, 2: prefill tiles of the additive-bias builds (64 keys at every head dim <= 512:
  // the 16x16x32 build with any additive bias, the 32x32x16 build with LDS-staged bias tiles), 3: the wide-row prefill tile
  // (ffpa_fwd_m16w_kernel.h; *br = 0 where the head dim has none), 4: the key-bias build of the split-D tiles where it runs the softmax pipeline (the tiles of
  // variant 0; its LDS without the ring cache)
  if (variant == 3) {
    *br = m16w_available(D) ? m16w_block_rows(m16w_row_halves(D)) : 0;
    *bc = m16w_block_keys(D);
    *lds = m16w_available(D) ? m16w_lds_bytes(D) : 0;
    return;
  }
  const int ND = variant == 1 ? ((D % 128 == 0) ? 4 : 2) : ((D <= 512) ? 1 : 2);
  int BC = (ND == 1) ? ((D <= FFPA_BC128_MAX_D && variant != 2) ? 128 : 64) : splitd_block_keys(D, ND);
  if (variant != 1 && D >= FFPA_M16_MIN_D) BC = m16_block_keys(D, variant == 2);  // (the 16x16x32 kernel's own rule)
  *br = 32 * (4 / ND);
  *bc = BC;
  *lds = 2 * BC * D * 2 + (variant == 1 ? splitd_exchange_bytes(D, ND) : (D >= FFPA_M16_MIN_D ? m16_exchange_bytes(D, variant == 2 ? 1 : (variant == 4 ? 3 : 0)) : (ND > 1 ? 4 * 4096 : 0)));
}

}  // namespace ffpa
