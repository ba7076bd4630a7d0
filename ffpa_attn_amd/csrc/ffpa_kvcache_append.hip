// ffpa_kvcache_append.hip — the prepare launch of ffpa_attn_with_kvcache(k=, v=, rotary_cos=, rotary_sin=) (C-ABI: ffpa_attn_kvcache_append, ffpa_capi.hip).
// A TU of its own: the dense, packed and paged attention objects stay exactly what they were.
//
// ONE launch per call, memory-bound: every workgroup is one token row (sequence b, token i) x a slice of its heads.
//   * new key i of sequence b goes to cache row pos = max(cache_seqlens[b], 0) + i — row pos % page_size of page block_table[b, pos / page_size] (ids clamped to
//     the pool), or row pos of sequence b's slab — unless pos >= capacity: then it is dropped.  V is copied, K is rotated on the way.
//   * with rotary, q is rotated into q_rot (query token i at position max(cache_seqlens[b], 0) + i when causal, at max(cache_seqlens[b], 0) otherwise: FlashAttention's
//     rule); the attention launch that follows on the same stream reads q_rot.
//   * the lengths the attention launch reads as seqused: used[b] = min(max(cache_seqlens[b], 0) + Snew, capacity).
// Every row moves as 16-byte loads and stores.  A lane owns one "unit" of a head — an 8-dim chunk, or (NeoX form) the two chunks of dims d and d + rotary_dim / 2
// that form pairs — and walks kAppendHeadsPerLane heads with the cos / sin of its unit loaded once into registers (one 8- or 16-byte load per token row and
// position).  Every load of a lane — its K heads, its q heads, its V chunk — is issued before its first store.  The rotation is fp32 (x * cos - y * sin, no
// FMA contraction: the same bits as the same formula in torch's fp32 ops), rounded once to the cache's dtype.  A decode batch has few token rows, so the launch
// side spreads a row's heads over more workgroups (down to one head per lane) until the grid covers the CUs.
#include "ffpa_kvcache_append.h"
#include "ffpa_kvcache_append_rows.h"  // (Vec, HeadRows: shared with the packed-token append)

namespace ffpa {
namespace {

template <typename T, bool INTERLEAVED>
__global__ __launch_bounds__(256) void ffpa_kv_append_kernel(const KvAppendArgs a) {
  using v8 = typename Vec<T>::v8;
  const int b = blockIdx.x / a.T, i = blockIdx.x - b * a.T;
  const int tid = threadIdx.x;
  const int len = a.seqlens[b];
  const int64_t base = len > 0 ? len : 0;  // (negative lengths act as 0, as in the attention kernels)
  if (blockIdx.y == 0 && i == 0 && tid == 0) {
    const int64_t n = base + a.Snew;
    a.used[b] = (int)(n < a.cap ? n : a.cap);
  }
  const int64_t pos = base + i;
  const bool kv_row = i < a.Snew && pos < a.cap;
  const bool q_row = a.rd > 0 && i < a.Sq;
  if (!kv_row && !q_row) return;

  // the lane's unit of a head (K and q: hs < slots) and its heads h0, h0 + hstep, ...
  const int hs = tid / a.units, u = tid - hs * a.units;
  const bool lane = hs < a.slots;
  const int h0 = blockIdx.y * a.slots + hs, hstep = gridDim.y * a.slots;
  int lo;
  bool rot;
  if constexpr (INTERLEAVED) {
    lo = 8 * u;
    rot = lo < a.rd;
  } else {
    const int npair = a.rd / 16;
    rot = u < npair;
    lo = rot ? 8 * u : a.rd + 8 * (u - npair);
  }
  const int hi = lo + a.rd / 2;
  const int half = a.rd / 2;

  int64_t kc_off = 0, vc_off = 0;  // the cache row's element offsets in the pools
  if (kv_row) {
    int page = b, row = (int)pos;
    if (a.table != nullptr) {
      page = a.table[(int64_t)b * a.bt_stride + row / a.page_size];
      page = page > 0 ? page : 0;
      page = page < a.num_pages - 1 ? page : a.num_pages - 1;
      row = row % a.page_size;
    }
    kc_off = page * a.kc_page_stride + row * a.skc[0];
    vc_off = page * a.vc_page_stride + row * a.svc[0];
  }
  const T* ksrc = (const T*)a.k + b * a.sk[0] + i * a.sk[1];
  const T* qsrc = (const T*)a.q + b * a.sq[0] + i * a.sq[1];
  HeadRows<T, INTERLEAVED> kr, qr;
  if (kv_row && lane) {
    const int64_t kp = pos < a.seqlen_ro - 1 ? pos : a.seqlen_ro - 1;
    kr.load(ksrc, a.sk[2], a.Hkv, h0, hstep, lo, hi, rot, (const T*)a.cos + (rot ? kp * half : 0), (const T*)a.sin + (rot ? kp * half : 0));
  }
  if (q_row && lane) {
    int64_t qp = a.causal ? base + i : base;
    qp = qp < a.seqlen_ro - 1 ? qp : a.seqlen_ro - 1;
    qr.load(qsrc, a.sq[2], a.Hq, h0, hstep, lo, hi, rot, (const T*)a.cos + (rot ? qp * half : 0), (const T*)a.sin + (rot ? qp * half : 0));
  }
  if (kv_row) {
    // V: a plain copy, 16 bytes per lane, over every workgroup of the token row
    const int cpr = a.D / 8;
    const T* vs = (const T*)a.v + b * a.sv[0] + i * a.sv[1];
    T* vd = (T*)a.vc + vc_off;
    for (int e = blockIdx.y * 256 + tid; e < a.Hkv * cpr; e += gridDim.y * 256) {
      const int h = e / cpr, c = e - h * cpr;
      *(v8*)(vd + h * a.svc[1] + c * 8) = *(const v8*)(vs + h * a.sv[2] + c * 8);
    }
  }
  if (kv_row && lane) kr.store((T*)a.kc + kc_off, a.skc[1], a.Hkv, h0, hstep, lo, hi, rot);
  if (q_row && lane) qr.store((T*)a.q_rot + b * a.sqr[0] + i * a.sqr[1], a.sqr[2], a.Hq, h0, hstep, lo, hi, rot);
}

}  // namespace

int launch_kv_append(int dtype, bool interleaved, const KvAppendArgs& a, unsigned grid_y, hipStream_t stream) {
  const dim3 grid((unsigned)(a.B * a.T), grid_y);
  if (dtype == 0) {
    if (interleaved)
      hipLaunchKernelGGL((ffpa_kv_append_kernel<__bf16, true>), grid, dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((ffpa_kv_append_kernel<__bf16, false>), grid, dim3(256), 0, stream, a);
  } else {
    if (interleaved)
      hipLaunchKernelGGL((ffpa_kv_append_kernel<_Float16, true>), grid, dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((ffpa_kv_append_kernel<_Float16, false>), grid, dim3(256), 0, stream, a);
  }
  return (int)hipGetLastError();
}

}  // namespace ffpa
