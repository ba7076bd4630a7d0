// ffpa_mla_fp8_inst.hip — MLA latent-cache attention over an FP8 cache: the latent pool holds OCP e4m3 codes with ONE per-tensor scale (K = kv_scale x K8), the
// form in which the serving engines keep the latent cache of DeepSeek-V2 / V3 / R1 and Kimi K2 (kv_cache_dtype = "fp8").  The plain variant of the latent kernel
// (ffpa_mla_variant.inc) over an e4m3 pool — with a power-of-two kv_scale the call returns the bits of the 16-bit latent call on the dequantised pool — and the two
// quantising appends.  Entry point: ffpa_attn_varlen_mla_fp8_fwd (ffpa_capi.hip).
#define FFPA_MLA_STEM mla_fp8
#define FFPA_MLA_TREE 0
#define FFPA_MLA_GATHER 0
#define FFPA_MLA_POOL FFPA_MLA_POOL_E4M3
#define FFPA_MLA_EXIT_REFRESH 0
#include "ffpa_mla_variant.inc"

namespace ffpa {

#if FFPA_INST_D == 576  // (one copy of the appends in the library: the first build's TU carries them)
// THE QUANTISATION of the appends, to the bit: rne_e4m3(clamp(float32(x) * inv, -448, +448)).  +-inf saturates; NaN stays NaN — a max / min (or med3) clamp returns
// its non-NaN operand, so the NaN is selected back explicitly.  The conversion instruction rounds to nearest even and keeps subnormals (down to 2^-9; +-2^-10 is a
// tie and goes to +-0); behind the clamp it never meets a value out of range.  Eight elements of T -> eight codes, element 0 in the low byte.
template <typename T>
__device__ __forceinline__ u32x2 quantize8_e4m3(u32x4 raw, float inv) {
  const typename Elem<T>::v8 x = __builtin_bit_cast(typename Elem<T>::v8, raw);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float s = (float)x[e] * inv;
    const float c = fminf(fmaxf(s, -448.f), 448.f);
    v[e] = s != s ? s : c;
  }
  u32x2 w;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int p = 0;
    p = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * h + 0], v[4 * h + 1], p, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * h + 2], v[4 * h + 3], p, true);
    w[h] = (uint32_t)p;
  }
  return w;
}

// One new row's Hkv heads, 8 elements per thread and step: ONE 16-byte load of T, ONE 8-byte vector store of codes.  (Strides of the pool are in its elements: bytes.)
template <typename T>
__device__ __forceinline__ void fp8_append_row(const MlaAppendArgs& a, const T* src, uint8_t* dst, float inv, int tid) {
  const int cpr = a.D / 8;  // 8-element chunks per head row
  for (int e = tid; e < a.Hkv * cpr; e += 256) {
    const int h = e / cpr, c = e - h * cpr;
    *(u32x2*)(dst + h * a.s_head + c * 8) = quantize8_e4m3<T>(*(const u32x4*)(src + h * a.s_new[2] + c * 8), inv);
  }
}

// THE QUANTISING LATENT APPEND (ffpa_attn_varlen_mla_fp8_fwd with kv_new): ffpa_mla_append_kernel — one workgroup per new token row, placed by the rule of
// ffpa_mla.h, used[b] written for every sequence — with the row stored as e4m3 codes.
template <typename T>
__global__ __launch_bounds__(256) void ffpa_mla_fp8_append_kernel(const MlaFp8AppendArgs fa) {
  const MlaAppendArgs& a = fa.a;
  const int S = a.Snew > 0 ? a.Snew : 1;
  const int b = blockIdx.x / S, i = blockIdx.x - b * S;
  const int tid = threadIdx.x;
  const int len = a.seqlens[b];
  const MlaAppendPlace at = mla_append_place(a, b, i, len, i < a.Snew);
  if (i == 0 && tid == 0) a.used[b] = mla_append_used(a, len, a.Snew);
  if (!at.keep) return;
  fp8_append_row<T>(a, (const T*)a.kv_new + b * a.s_new[0] + i * a.s_new[1], (uint8_t*)a.cache + at.page * a.s_page + at.row * a.s_row, fa.inv, tid);
}

int launch_mla_fp8_append(int dtype, const MlaFp8AppendArgs& fa, hipStream_t stream) {
  const int S = fa.a.Snew > 0 ? fa.a.Snew : 1;
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(ffpa_mla_fp8_append_kernel<T>, dim3((unsigned)(fa.a.B * S)), dim3(256), 0, stream, fa);
    return (int)hipGetLastError();
  });
}

// THE QUANTISING LATENT APPEND OF A RAGGED STEP (ffpa_attn_mla_fp8_append_varlen): ffpa_mla_append_varlen_kernel — one workgroup per token row t of kv_new
// [T, Hkv, D] packed by cu_q, the row's sequence by cu_seqlens_find, rows from cu_q[B] on write nothing, lane l of workgroup x writes used[256 x + l] (the grid has
// at least ceil(B / 256) workgroups), every read through a wave-uniform index in front of the first store — with the row stored as e4m3 codes.
template <typename T>
__global__ __launch_bounds__(256) void ffpa_mla_fp8_append_varlen_kernel(const MlaFp8AppendVarlenArgs fa) {
  const MlaAppendVarlenArgs& va = fa.va;
  const MlaAppendArgs& a = va.a;
  const int t = blockIdx.x, tid = threadIdx.x;
  const int b = cu_seqlens_find(va.cu_q, a.B, va.T, t);  // (a.B: a padding row)
  const bool real = b < a.B;
  const int i = real ? t - va.cu_q[b] : -1;  // (negative under a cu_q that does not ascend: the row is dropped)
  const MlaAppendPlace at = mla_append_place(a, b, i, real ? a.seqlens[b] : 0, real && i >= 0);
  const int64_t s = (int64_t)t * 256 + tid;
  if (s < a.B) a.used[s] = mla_append_used(a, a.seqlens[s], va.cu_q[s + 1] - va.cu_q[s]);
  if (!at.keep) return;
  fp8_append_row<T>(a, (const T*)a.kv_new + t * a.s_new[1], (uint8_t*)a.cache + at.page * a.s_page + at.row * a.s_row, fa.inv, tid);
}

int launch_mla_fp8_append_varlen(int dtype, const MlaFp8AppendVarlenArgs& fa, hipStream_t stream) {
  const unsigned used_wgs = (unsigned)((fa.va.a.B + 255) / 256);
  const unsigned grid = (unsigned)fa.va.T > used_wgs ? (unsigned)fa.va.T : used_wgs;
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(ffpa_mla_fp8_append_varlen_kernel<T>, dim3(grid), dim3(256), 0, stream, fa);
    return (int)hipGetLastError();
  });
}
#endif

}  // namespace ffpa
