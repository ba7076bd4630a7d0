// ffpa_mla_inst.hip — MLA latent-cache attention (DeepSeek-V2 / V3 / R1, Kimi K2 in their "absorbed" decode form): every query head has D columns, all heads of a
// group attend to ONE latent KV head, and the values are the first dv columns of the very rows that serve as keys.  The plain variant of the latent kernel
// (ffpa_mla_variant.inc: no mask, keys through the page table, a 16-bit pool; a contiguous cache runs through it with one page per sequence) and the two 16-bit
// appends.  One unit per (D, dv) pair of FFPA_FOR_EACH_MLA_BUILD (-DFFPA_INST_D=<D>; bf16 + fp16, plain + NT).  Entry point: ffpa_attn_varlen_mla_fwd (ffpa_capi.hip).
#define FFPA_MLA_STEM mla
#define FFPA_MLA_TREE 0
#define FFPA_MLA_GATHER 0
#define FFPA_MLA_POOL FFPA_MLA_POOL_16BIT
#define FFPA_MLA_EXIT_REFRESH 0
#include "ffpa_mla_variant.inc"

namespace ffpa {

#if FFPA_INST_D == 576  // (one copy of the append in the library: the first build's TU carries it)
// One new row's Hkv heads as raw bytes — 16-bit elements of either dtype —, every 16-byte chunk loaded and stored once.
__device__ __forceinline__ void mla_append_row(const MlaAppendArgs& a, const uint16_t* src, uint16_t* dst, int tid) {
  const int cpr = a.D / 8;  // 16-byte chunks per head row
  for (int e = tid; e < a.Hkv * cpr; e += 256) {
    const int h = e / cpr, c = e - h * cpr;
    *(u32x4*)(dst + h * a.s_head + c * 8) = *(const u32x4*)(src + h * a.s_new[2] + c * 8);
  }
}

// THE LATENT APPEND (ffpa_attn_varlen_mla_fwd with kv_new): one workgroup per new token row, placed by the rule of ffpa_mla.h and stored once — the append of
// ffpa_kvcache_append.hip writes a K and a V cache, and here there is one cache.  used[b] by the workgroup of the sequence's first row (one at Snew == 0 too).
__global__ __launch_bounds__(256) void ffpa_mla_append_kernel(const MlaAppendArgs a) {
  const int T = a.Snew > 0 ? a.Snew : 1;
  const int b = blockIdx.x / T, i = blockIdx.x - b * T;
  const int tid = threadIdx.x;
  const int len = a.seqlens[b];
  const MlaAppendPlace at = mla_append_place(a, b, i, len, i < a.Snew);
  if (i == 0 && tid == 0) a.used[b] = mla_append_used(a, len, a.Snew);
  if (!at.keep) return;
  mla_append_row(a, (const uint16_t*)a.kv_new + b * a.s_new[0] + i * a.s_new[1], (uint16_t*)a.cache + at.page * a.s_page + at.row * a.s_row, tid);
}

int launch_mla_append(const MlaAppendArgs& a, hipStream_t stream) {
  const int T = a.Snew > 0 ? a.Snew : 1;
  hipLaunchKernelGGL(ffpa_mla_append_kernel, dim3((unsigned)(a.B * T)), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

// THE LATENT APPEND OF A RAGGED STEP (ffpa_attn_mla_append_varlen): one workgroup per token row t of kv_new [T, Hkv, D] packed by cu_q.  The row finds its
// sequence b by the two-cache ragged append's search (cu_seqlens_find) and is placed as above, as token t - cu_q[b]; rows from cu_q[B] on are padding and write
// nothing.  Everything read through a wave-uniform index — the search, the sequence's length, its page id — stands in front of the kernel's first store (used[]).
//   used[b] for EVERY b < B, sequences without a token too, so not by the token rows: lane l of workgroup x writes used[256 x + l]; the grid has at least
//   ceil(B / 256) workgroups (T == 0 and T < B included).
__global__ __launch_bounds__(256) void ffpa_mla_append_varlen_kernel(const MlaAppendVarlenArgs va) {
  const MlaAppendArgs& a = va.a;
  const int t = blockIdx.x, tid = threadIdx.x;
  const int b = cu_seqlens_find(va.cu_q, a.B, va.T, t);  // (a.B: a padding row)
  const bool real = b < a.B;
  const int i = real ? t - va.cu_q[b] : -1;  // (negative under a cu_q that does not ascend: the row is dropped)
  const MlaAppendPlace at = mla_append_place(a, b, i, real ? a.seqlens[b] : 0, real && i >= 0);
  const int64_t s = (int64_t)t * 256 + tid;
  if (s < a.B) a.used[s] = mla_append_used(a, a.seqlens[s], va.cu_q[s + 1] - va.cu_q[s]);
  if (!at.keep) return;
  mla_append_row(a, (const uint16_t*)a.kv_new + t * a.s_new[1], (uint16_t*)a.cache + at.page * a.s_page + at.row * a.s_row, tid);
}

int launch_mla_append_varlen(const MlaAppendVarlenArgs& va, hipStream_t stream) {
  const unsigned used_wgs = (unsigned)((va.a.B + 255) / 256);
  hipLaunchKernelGGL(ffpa_mla_append_varlen_kernel, dim3((unsigned)va.T > used_wgs ? (unsigned)va.T : used_wgs), dim3(256), 0, stream, va);
  return (int)hipGetLastError();
}
#endif

}  // namespace ffpa
