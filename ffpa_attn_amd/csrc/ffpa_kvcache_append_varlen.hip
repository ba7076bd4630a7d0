// ffpa_kvcache_append_varlen.hip — the prepare launch of ffpa_attn_varlen_with_kvcache (C-ABI: ffpa_attn_kvcache_append_varlen, ffpa_capi.hip): the append of
// ffpa_kvcache_append.hip for a RAGGED step — q / k / v are token rows [total, H, D] packed by cu_seqlens_q (a prompt chunk, a few speculative verifications and
// dozens of one-token decodes in one batch).  A TU of its own: the [B, S] append's object and the attention objects stay exactly what they were.
//
// ONE launch per call: every workgroup is one token row t x a slice of its heads.
//   * the row finds its sequence b (cu_q[b] <= t < cu_q[b + 1]) by a binary search of cu_q — t is the workgroup's index, so the search is wave-uniform, and it
//     stands in front of the kernel's first store, so it runs on scalar loads, log2(B) + 1 of them (see the kernel); empty sequences (cu_q[b + 1] == cu_q[b]) are stepped over, rows from cu_q[B] on are padding and write nothing.
//   * its index in the sequence is i = t - cu_q[b]; key i goes to cache row pos = max(cache_seqlens[b], 0) + i exactly as in the [B, S] form (paged or contiguous,
//     ids clamped to the pool, pos >= capacity dropped; pos / page_size < pages_per_row, so the table is never read past the row).
//   * rotary position: positions == nullptr — the [B, S] form's rule (key at pos, query token at pos when causal, at max(cache_seqlens[b], 0) otherwise);
//     else key AND query token at positions[t], the key still WRITTEN at its slot pos (a tree draft: the position is the depth, not the slot).  Clamped to
//     [0, seqlen_ro - 1].
//   * used[b] = min(max(cache_seqlens[b], 0) + (cu_q[b + 1] - cu_q[b]), capacity) for every b < B — sequences without a token too, so not by the token rows:
//     lane l of workgroup row x (y == 0) writes used[256 x + l]; the grid has at least ceil(B / 256) rows.
// The lane layout, the loads-before-stores order and the rotation are HeadRows' (ffpa_kvcache_append_rows.h): on a uniform batch the bytes written to the cache
// and to q_rot are the [B, S] kernel's.
#include "ffpa_cu_seqlens_find.h"
#include "ffpa_kvcache_append.h"
#include "ffpa_kvcache_append_rows.h"

namespace ffpa {
namespace {

template <typename T, bool INTERLEAVED>
__global__ __launch_bounds__(256) void ffpa_kv_append_varlen_kernel(const KvAppendVarlenArgs va) {
  using v8 = typename Vec<T>::v8;
  const KvAppendArgs& a = va.a;
  const int t = blockIdx.x, tid = threadIdx.x;
  // Everything the row reads through a wave-uniform index — the search of cu_q, its sequence's length, its page id, its position — is read BEFORE the kernel's
  // first store (used[], below): up to there the compiler can prove the arrays unchanged and reads them with scalar loads; a load behind the store is a vector
  // load plus a readfirstlane, and the search is a chain of dependent ones.
  const int b = cu_seqlens_find(va.cu_q, a.B, a.T, t);  // (a.B: a padding row)
  const bool real = b < a.B;
  const int i = real ? t - va.cu_q[b] : -1;  // (negative under a cu_q that does not ascend: the row is dropped, never a negative cache row)
  const int len = real ? a.seqlens[b] : 0;
  const int64_t base = len > 0 ? len : 0;  // (negative lengths act as 0, as in the attention kernels)
  const int64_t pos = base + i;
  const bool kv_row = real && i >= 0 && pos < a.cap;
  const bool q_row = real && i >= 0 && a.rd > 0;
  int page = b, row = (int)pos;
  if (kv_row && a.table != nullptr) {
    page = a.table[(int64_t)b * a.bt_stride + row / a.page_size];
    page = page > 0 ? page : 0;
    page = page < a.num_pages - 1 ? page : a.num_pages - 1;
    row = row % a.page_size;
  }
  // rotary positions of the key and of the query token, clamped to the tables' rows
  int64_t kp = pos, qp = a.causal ? pos : base;
  if (va.positions != nullptr && (kv_row || q_row) && a.rd > 0) kp = qp = va.positions[t];
  const int64_t last = a.seqlen_ro - 1;
  kp = kp < last ? kp : last, qp = qp < last ? qp : last;
  kp = kp > 0 ? kp : 0, qp = qp > 0 ? qp : 0;

  if (blockIdx.y == 0) {
    const int s = t * 256 + tid;
    if (s < a.B) {
      const int slen = a.seqlens[s];
      const int64_t n = (int64_t)(slen > 0 ? slen : 0) + (va.cu_q[s + 1] - va.cu_q[s]);
      a.used[s] = (int)(n < a.cap ? n : a.cap);
    }
  }
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
  const int hi_d = lo + a.rd / 2;
  const int half = a.rd / 2;

  int64_t kc_off = 0, vc_off = 0;  // the cache row's element offsets in the pools
  if (kv_row) {
    kc_off = page * a.kc_page_stride + row * a.skc[0];
    vc_off = page * a.vc_page_stride + row * a.svc[0];
  }
  const T* ksrc = (const T*)a.k + t * a.sk[1];
  const T* qsrc = (const T*)a.q + t * a.sq[1];
  HeadRows<T, INTERLEAVED> kr, qr;
  if (kv_row && lane)
    kr.load(ksrc, a.sk[2], a.Hkv, h0, hstep, lo, hi_d, rot, (const T*)a.cos + (rot ? kp * half : 0), (const T*)a.sin + (rot ? kp * half : 0));
  if (q_row && lane)
    qr.load(qsrc, a.sq[2], a.Hq, h0, hstep, lo, hi_d, rot, (const T*)a.cos + (rot ? qp * half : 0), (const T*)a.sin + (rot ? qp * half : 0));
  if (kv_row) {
    // V: a plain copy, 16 bytes per lane, over every workgroup of the token row
    const int cpr = a.D / 8;
    const T* vs = (const T*)a.v + t * a.sv[1];
    T* vd = (T*)a.vc + vc_off;
    for (int e = blockIdx.y * 256 + tid; e < a.Hkv * cpr; e += gridDim.y * 256) {
      const int h = e / cpr, c = e - h * cpr;
      *(v8*)(vd + h * a.svc[1] + c * 8) = *(const v8*)(vs + h * a.sv[2] + c * 8);
    }
  }
  if (kv_row && lane) kr.store((T*)a.kc + kc_off, a.skc[1], a.Hkv, h0, hstep, lo, hi_d, rot);
  if (q_row && lane) qr.store((T*)a.q_rot + t * a.sqr[1], a.sqr[2], a.Hq, h0, hstep, lo, hi_d, rot);
}

}  // namespace

int launch_kv_append_varlen(int dtype, bool interleaved, const KvAppendVarlenArgs& va, unsigned grid_y, hipStream_t stream) {
  const unsigned used_rows = (unsigned)((va.a.B + 255) / 256);
  const dim3 grid((unsigned)va.a.T > used_rows ? (unsigned)va.a.T : used_rows, grid_y);
  if (dtype == 0) {
    if (interleaved)
      hipLaunchKernelGGL((ffpa_kv_append_varlen_kernel<__bf16, true>), grid, dim3(256), 0, stream, va);
    else
      hipLaunchKernelGGL((ffpa_kv_append_varlen_kernel<__bf16, false>), grid, dim3(256), 0, stream, va);
  } else {
    if (interleaved)
      hipLaunchKernelGGL((ffpa_kv_append_varlen_kernel<_Float16, true>), grid, dim3(256), 0, stream, va);
    else
      hipLaunchKernelGGL((ffpa_kv_append_varlen_kernel<_Float16, false>), grid, dim3(256), 0, stream, va);
  }
  return (int)hipGetLastError();
}

}  // namespace ffpa
