// ffpa_mla_sparse_ds.h — sparse (top-k indexed) attention over the 656-byte FP8 latent rows of DeepSeek-V3.2 (vLLM's "fp8_ds_mla", the FP8 KV layout of FlashMLA's
// sparse decode; ffpa_attn_varlen_mla_sparse_ds_fwd, ffpa_capi.hip): the row format, the kernel's helpers for it (the hooks of the shell's 656-byte pool, ffpa_mla_variant.inc) and the store
// kernel's launcher (ffpa_mla_ds_store.hip).  A header of its own so that every other object sees nothing of it.
//
// THE ROW, kDsRowBytes = 656 bytes of one latent head of one slot:
//     bytes   0 ... 511   the 512 latent ("NoPE") columns as OCP e4m3 codes
//     bytes 512 ... 527   four float32 scales, one per 128 columns:  column c = bf16_rne(float32(code[c]) * scale[c / 128])
//     bytes 528 ... 655   the 64 rotary columns as bf16, as they are
// The attention kernels take FwdArgs / VarlenArgs / PagedArgs as the sparse launch fills them with the pool's strides in units of TWO BYTES (ffpa_mla_fp8.h)
// and MlaArgs (the value width).
#pragma once
#include <hip/hip_runtime.h>

#include "ffpa_mla.h"

namespace ffpa {

constexpr int kDsNope = 512;        // quantised columns: bytes [0, 512) of a row
constexpr int kDsTile = 128;        // columns under one scale
constexpr int kDsScaleOff = 512;    // first byte of the four float32 scales
constexpr int kDsRopeOff = 528;     // first byte of the 64 bf16 rotary columns
constexpr int kDsRowBytes = 656;

// Where 16-byte slot `s` of the 576-wide bf16 image of a row (8 columns) lies in the row's bytes: eight codes, or sixteen bytes of the rotary part.
__device__ __forceinline__ constexpr uint32_t ds_slot_off(int s) { return s < kDsNope / 8 ? (uint32_t)(8 * s) : (uint32_t)(kDsRopeOff + 16 * (s - kDsNope / 8)); }
// What a lane adds to its slot's offset to reach the scale of the slot's 128-column tile (a rotary slot: nothing — the dword it then reads lies in its own row and
// is not used).  Modulo 2^32: the sum with the slot's offset is the scale's offset.
__device__ __forceinline__ constexpr uint32_t ds_scale_delta(int s) { return s < kDsNope / 8 ? (uint32_t)(kDsScaleOff + 4 * (s >> 4)) - (uint32_t)(8 * s) : 0u; }

// The register loads of a piece: sixteen bytes at the slot (a NoPE lane uses the low eight; its over-read ends at byte 8 x 63 + 16 = 520, inside the row) and
// the dword of the scale.  The compiler's own loads (it counts vmcnt for them); the descriptor's range check returns zeros for a lane whose offset carries the
// "no row" bit.  NT: the non-temporal hint (aux bit 1).
__device__ u32x4 ffpa_raw_buffer_load_b128(u32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4i32");
__device__ float ffpa_raw_buffer_load_f32(u32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.f32");
template <bool NT>
__device__ __forceinline__ u32x4 buffer_load_16(u32x4 rsrc, uint32_t voff) {
  return ffpa_raw_buffer_load_b128(rsrc, (int)voff, 0, NT ? 2 : 0);
}
template <bool NT>
__device__ __forceinline__ float buffer_load_f32(u32x4 rsrc, uint32_t voff) {
  return ffpa_raw_buffer_load_f32(rsrc, (int)voff, 0, NT ? 2 : 0);
}

// Eight codes (the two low dwords of `w`, element 0 in the low byte) under `scale` -> eight bf16 as one 16-byte LDS slot: the conversion to float32 is exact, then
// ONE float32 multiply and ONE round-to-nearest-even to bf16 per element — unpack_latent_rows_ds (ffpa_attn_amd/kvcache.py) to the bit.
__device__ __forceinline__ u32x4 ds_nope_widen(u32x4 w, float scale) {
  Elem<__bf16>::v8 r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], true);
    r[4 * h + 0] = (__bf16)(lo[0] * scale);
    r[4 * h + 1] = (__bf16)(lo[1] * scale);
    r[4 * h + 2] = (__bf16)(hi[0] * scale);
    r[4 * h + 3] = (__bf16)(hi[1] * scale);
  }
  return __builtin_bit_cast(u32x4, r);
}

// The store kernel (ffpa_attn_mla_ds_store): row t of kv_new [T, Hkv, 576] (bf16; strides in elements) is packed into slot slots[t] of the byte pool (strides in
// bytes); a slot outside [0, num_rows) writes nothing.
struct MlaDsStoreArgs {
  const void* kv_new;
  const int* slots;
  void* pool;
  int64_t s_new[2];   // elements: token, head
  int64_t s_pool[2];  // bytes: slot, head
  int T, Hkv, num_rows;
};

int launch_mla_ds_store(const MlaDsStoreArgs& a, hipStream_t stream);

}  // namespace ffpa
