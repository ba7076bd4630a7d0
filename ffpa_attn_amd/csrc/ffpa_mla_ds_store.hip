// ffpa_mla_ds_store.hip — the kernel that WRITES the 656-byte FP8 latent rows of DeepSeek-V3.2 (ffpa_mla_sparse_ds.h; ffpa_attn_mla_ds_store, ffpa_capi.hip): new
// rows kv_new [T, Hkv, 576] (bf16) go to the pool slots slots[t], as the engines write this cache (by slot_mapping, not by sequence lengths).  A small TU of its
// own, no inline asm; every store is an ordinary vector store.
//
// THE ROW, to the byte — pack_latent_rows_ds (ffpa_attn_amd/kvcache.py) is the definition.  For each of the four 128-column tiles x of the first 512 columns:
//     a    = amax(|float32(x)|), non-finite elements counted as 0
//     s    = max(a / 448, 2^-100)                      float32, IEEE division
//     code = rne_e4m3(clamp(float32(x) / s, +-448))    IEEE division; NaN stays NaN (x's sign), +-inf saturates — the clamp / NaN rule of the FP8 appends (ffpa_mla_fp8_inst.hip)
// then codes[512] | s[4] as float32 | the 64 rotary columns' bf16 bytes as they are.  (-fhip-fp32-correctly-rounded-divide-sqrt is hipcc's default: both
// divisions are correctly rounded.)
#include "ffpa_common.h"
#include "ffpa_mla_sparse_ds.h"

namespace ffpa {

// One workgroup per (token, latent head), one wave per 128-column tile: a lane holds two columns, the amax is a wave reduction, the lane stores its two codes,
// lane 0 the tile's scale, and the first eight lanes of each wave copy 32 of the 128 rotary bytes.  The slot is read through a wave-uniform index in front of the
// first store; a slot < 0 (the engines' padding) or >= num_rows writes nothing.  Two tokens with one slot: one of them wins.
__global__ __launch_bounds__(256) void ffpa_mla_ds_store_kernel(const MlaDsStoreArgs a) {
  const int t = (int)(blockIdx.x / (unsigned)a.Hkv), h = (int)(blockIdx.x % (unsigned)a.Hkv);
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int slot = a.slots[t];
  if (slot < 0 || slot >= a.num_rows) return;
  const __bf16* src = (const __bf16*)a.kv_new + (int64_t)t * a.s_new[0] + (int64_t)h * a.s_new[1];
  uint8_t* dst = (uint8_t*)a.pool + (int64_t)slot * a.s_pool[0] + (int64_t)h * a.s_pool[1];

  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
  const bf16x2 x2 = *(const bf16x2*)(src + wave * kDsTile + 2 * lane);
  const float x[2] = {(float)x2[0], (float)x2[1]};
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float m = fabsf(x[e]);
    amax = fmaxf(amax, m < __builtin_inff() ? m : 0.f);  // (NaN and inf compare false: counted as 0)
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 64));
  const float s = fmaxf(amax / 448.f, 0x1p-100f);
  float v[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float r = x[e] / s;
    const float c = fminf(fmaxf(r, -448.f), 448.f);
    v[e] = x[e] != x[e] ? x[e] : c;  // (a max / min clamp returns its non-NaN operand: x's own NaN is selected back; x / s is NaN only then)
  }
  uint32_t p = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
#pragma unroll
  for (int e = 0; e < 2; ++e) {  // (the NaN code keeps x's sign, as the definition's conversion does; the instruction's NaN code does not)
    const uint32_t nan_code = 0x7Fu | ((__builtin_bit_cast(uint32_t, x[e]) >> 24) & 0x80u);
    if (x[e] != x[e]) p = (p & ~(0xFFu << (8 * e))) | (nan_code << (8 * e));
  }
  *(uint16_t*)(dst + wave * kDsTile + 2 * lane) = (uint16_t)p;
  if (lane == 0) *(float*)(dst + kDsScaleOff + 4 * wave) = s;
  if (lane < 8) *(uint32_t*)(dst + kDsRopeOff + 4 * (8 * wave + lane)) = *(const uint32_t*)(src + kDsNope + 2 * (8 * wave + lane));
}

int launch_mla_ds_store(const MlaDsStoreArgs& a, hipStream_t stream) {
  if (a.T == 0) return 0;
  hipLaunchKernelGGL(ffpa_mla_ds_store_kernel, dim3((unsigned)((int64_t)a.T * a.Hkv)), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace ffpa
