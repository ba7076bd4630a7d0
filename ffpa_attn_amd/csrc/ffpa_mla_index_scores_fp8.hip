// ffpa_mla_index_scores_fp8.hip — the indexer's score launch over FP8 index keys (ffpa_attn_mla_index_scores_fp8, ffpa_capi.hip) and the quantising append that
// fills their cache (ffpa_attn_mla_index_k_append_fp8): the form in which the engines that serve DeepSeek-V3.2 keep the index keys (DeepGEMM's
// fp8_paged_mqa_logits reads it, vLLM's indexer_k_quant_and_cache writes it).  A TU of its own; the MFMA is a compiler builtin (the hazard padding is the
// compiler's), every store is an ordinary vector store, there is no inline assembly.
//
// THE RESULT.  The token rules are ffpa_mla_index_scores.hip's to the letter: token t is token i of sequence b (cu_seqlens_q and its binary search, or t / Sq and
// t % Sq), sees the key positions [0, n), n = clamp(L - (S - 1 - i), 0, N) under causal, clamp(L, 0, N) otherwise, never more than the table (W * page_size) or
// the capacity can name; key p is row p % page_size of page table[b, min(p / page_size, W - 1)], the id clamped into [0, num_pages - 1].
//     scores[t, p] = kscale[b, p] * sum_h w[t, h] * max(0, sum_d q8[t, h, d] * k8[b, p, d])   for p < n,      -inf for n <= p < N  (a padding row: all -inf)
// q8 / k8 the e4m3 codes' values, kscale the key's float32 in its page's scale plane (ffpa_mla_index_scores_fp8.h: the page format) — any positive finite value.
//
// HOW.  The 16-bit kernel's work split — one workgroup of 4 waves per (token, chunk of key positions), the chunk the fastest grid index, a wave walking its
// quarter in steps of 64 keys — with an operand path of its own:
//   * v_mfma_f32_16x16x128_f8f6f4 (both formats e4m3, no block scales): ONE instruction contracts a (16 heads x 16 keys) block over all 128 columns, A = Q,
//     B = K, 8 VGPRs per lane each.  16 MFMAs per 64-key step at Hi = 64 where the 16-bit kernel issues 64.
//   * THE COLUMN ASSIGNMENT.  Lane l of row l % 16 holds the 32 contiguous bytes at column 32 (l / 16) of its row, as two 16-byte loads — for A and for B
//     alike.  The product is contracted over all 128 columns inside the one instruction, so any lane -> column assignment gives the right sum as long as A
//     and B use the SAME one; this one makes every load 16 bytes wide and four lanes cover a row's 128 bytes.
//   * Q — Hi / 16 blocks x 8 VGPRs, 32 at Hi = 64 — is loaded once and lives as long as the wave.  A 64-key step of K is 8 sixteen-byte loads per lane out of
//     8 KiB of contiguous code plane (page_size % 64 == 0: a step never leaves its page), plus ONE 4-byte load: lane l's key scale, 256 coalesced bytes per
//     wave out of the scale plane.  The NEXT step's nine loads are issued in front of this step's MFMAs: two register buffers, the loop unrolled by two, no
//     load behind a condition of its own (ffpa_mla_index_scores.hip says why).
//   * Rows at and past n are never turned into an address — not in the code plane, not in the scale plane: the key is clamped into [step's first key, n - 1],
//     the same 64-key block, the same page, and the result is masked.
//   * C comes out as the 16x16x32 instructions' does: lane l holds key l % 16 and heads 16 hb + 4 (l / 16) + i.  max(0, .) times the lane's four weights sums
//     in-lane, two cross-lane adds (xor 16, xor 32) finish the heads, lane l keeps block l / 16's total — key 64 step + l, whose scale it loaded — multiplies
//     once and stores: one coalesced 256-byte store per wave and step.  No LDS, no atomics, no barrier.
// The wave-uniform reads stand in front of the first store.  Addresses are 64-bit.  Every index that becomes an address is bounded first: a head by Hi, a key by
// n <= min(N, W * page_size), a table column by W - 1, a page id by num_pages - 1, an output column by N.
//
// THE APPEND.  One wave per new key row, lane l holding columns 2 l and 2 l + 1: amax by a wave max-reduce, the scale
//     s = max(amax, 1e-4) / 448 in fp32 (IEEE division), rounded UP to a power of two on its exponent bits (a non-zero mantissa: exponent + 1, mantissa cleared)
// and   code = rne_e4m3(clamp(float32(x) / scale, +-448)),   the division a multiplication by the exact reciprocal power of two,
// the clamp / NaN rule and the conversion instruction those of the FP8 latent appends (ffpa_mla_fp8_inst.hip: NaN stays NaN; finite inputs are the contract).  128
// codes into the page's code plane, the scale into its scale plane — byte for byte what quantize_index_rows + pack_index_key_pages (kvcache.py) give.  The
// placement is the latent appends' (ffpa_mla.h): a negative length acts as 0, a position at or past the capacity is dropped without a table read, a page id is
// clamped into the pool, lens_after is written for EVERY sequence (lane l of workgroup x writes lens_after[64 x + l]).
#include "ffpa_mla_index_scores_fp8.h"

#include "ffpa_cu_seqlens_find.h"

namespace ffpa {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStep = 64;  // keys per wave and step: four 16-key MFMA column blocks

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// 32 contiguous bytes (16-byte aligned) as one MFMA operand
__device__ __forceinline__ i32x8 load32(const uint8_t* src) {
  const i32x4 lo = *reinterpret_cast<const i32x4*>(src), hi = *reinterpret_cast<const i32x4*>(src + 16);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// where a wave stands in its sequence's keys: the step's first key, its page's index in the table row and its first row inside that page
struct Walk {
  int p0, pidx, row0;
};

// a 64-key step's operands: key block kb's fragment, and the scale of the key the lane stores
struct KStep {
  i32x8 k[4];
  float scale;
};

// the nine loads of the 64-key step at `at`.  Keys at and past n read key n - 1 (at.p0 < n: the same block, the same page), codes and scale alike.
__device__ __forceinline__ void load_step(KStep& s, const MlaIndexScoresFp8Args& a, const int* table, int b, int n, Walk at, int lane) {
  const int r = lane & 15, g = lane >> 4;
  int page = table != nullptr ? table[min(at.pidx, a.W - 1)] : b;  // wave-uniform
  page = clampi(page, 0, a.num_pages - 1);
  const uint8_t* base = a.k + (int64_t)page * a.s_k_page;
  const int last = n - 1 - at.p0;  // >= 0
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) s.k[kb] = load32(base + (int64_t)(at.row0 + min(16 * kb + r, last)) * kMlaIndexFp8Dim + 32 * g);
  s.scale = *reinterpret_cast<const float*>(base + (int64_t)a.page_size * kMlaIndexFp8Dim + 4 * (int64_t)(at.row0 + min(lane, last)));
}

// the 64 scores of a step, the key scale not yet applied: lane l returns the sum of key at.p0 + l
template <int HB>
__device__ __forceinline__ float score_step(const i32x8 (&qf)[HB], const float (&wf)[HB][4], const KStep& s, int g) {
  float mine = 0.f;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    float part = 0.f;
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      // (cbsz = blgp = 0: A and B are e4m3; the scale operands zero: the compiler emits the instruction without block scales)
      const f32x4 acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(qf[hb], s.k[kb], zero, 0, 0, 0, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) part = fmaf(wf[hb][i], fmaxf(acc[i], 0.f), part);
    }
    part += __shfl_xor(part, 16, 64);
    part += __shfl_xor(part, 32, 64);
    if (g == kb) mine = part;
  }
  return mine;
}

template <int HB>
__global__ __launch_bounds__(kThreads) void ffpa_mla_index_scores_fp8_kernel(const MlaIndexScoresFp8Args a) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int nchunks = (a.N + a.chunk - 1) / a.chunk;
  const int t = (int)(blockIdx.x / (unsigned)nchunks), chunk = (int)(blockIdx.x % (unsigned)nchunks);

  // ---- wave-uniform: the token's sequence, its visible length (ffpa_mla_index_scores.hip's rule)
  int b, n;
  {
    int i, S;
    if (a.cu_seqlens_q != nullptr) {
      b = cu_seqlens_find(a.cu_seqlens_q, a.B, a.cu_seqlens_q[a.B], t);
      const int lo = b < a.B ? a.cu_seqlens_q[b] : 0;
      i = t - lo, S = b < a.B ? a.cu_seqlens_q[b + 1] - lo : 0;
    } else {
      S = a.T / a.B, b = t / S, i = t % S;
    }
    const bool pad = b >= a.B;
    b = clampi(b, 0, a.B - 1);
    const int L = a.cache_seqlens[b];
    int64_t vis = a.causal ? (int64_t)L - (S - 1 - i) : (int64_t)L;
    const int64_t cap = (int64_t)a.W * a.page_size;  // what the table (the capacity) can name
    vis = vis > cap ? cap : vis;
    n = pad ? 0 : (int)(vis < 0 ? 0 : (vis > a.N ? a.N : vis));
  }
  const int per_wave = a.chunk / kWaves;
  const int begin = chunk * a.chunk + wave * per_wave, end = min(begin + per_wave, a.N);
  float* out = a.scores + (int64_t)t * a.s_out;
  const float ninf = -__builtin_inff();

  if (begin < n) {
    // ---- Q and the weights, once: lane l holds 32 bytes of head 16 hb + l % 16 of A, and the weights of the heads 16 hb + 4 (l / 16) + i its C values belong to
    i32x8 qf[HB];
    float wf[HB][4];
    {
      const uint8_t* qrow = a.q + (int64_t)t * a.s_q_tok + 32 * g;
      const float* wrow = a.w + (int64_t)t * a.s_w;
#pragma unroll
      for (int hb = 0; hb < HB; ++hb) {
        qf[hb] = load32(qrow + (int64_t)(16 * hb + r) * a.s_q_head);
#pragma unroll
        for (int i = 0; i < 4; ++i) wf[hb][i] = wrow[16 * hb + 4 * g + i];
      }
    }
    const int* table = a.block_table != nullptr ? a.block_table + (int64_t)b * a.s_table : nullptr;
    const int live = min((min(end, n) - begin + kStep - 1) / kStep, per_wave / kStep);  // steps with a visible key: >= 1
    Walk at = {begin, begin / a.page_size, begin % a.page_size};
    const auto next = [&](Walk w) {
      w.p0 += kStep, w.row0 += kStep;
      if (w.row0 >= a.page_size) w.row0 = 0, ++w.pidx;
      return w;
    };
    const auto store = [&](const Walk& w, float x) {
      if (w.p0 + lane < end) out[w.p0 + lane] = w.p0 + lane < n ? x : ninf;
    };
    // Two register buffers, the loop unrolled by two, no load behind a condition of its own: between the loads of a step and its MFMAs lie exactly the nine
    // loads of the next one, so the wait in front of the MFMAs is for the older nine alone.
    KStep k0, k1;
    load_step(k0, a, table, b, n, at, lane);
    int left = live;
    while (left > 2) {
      const Walk at1 = next(at), at2 = next(at1);
      load_step(k1, a, table, b, n, at1, lane);
      store(at, k0.scale * score_step<HB>(qf, wf, k0, g));
      load_step(k0, a, table, b, n, at2, lane);
      store(at1, k1.scale * score_step<HB>(qf, wf, k1, g));
      at = at2, left -= 2;
    }
    if (left == 2) {
      const Walk at1 = next(at);
      load_step(k1, a, table, b, n, at1, lane);
      store(at, k0.scale * score_step<HB>(qf, wf, k0, g));
      store(at1, k1.scale * score_step<HB>(qf, wf, k1, g));
    } else {
      store(at, k0.scale * score_step<HB>(qf, wf, k0, g));
    }
    for (int p = begin + live * kStep + lane; p < end; p += 64) out[p] = ninf;
  } else {
    for (int p = begin + lane; p < end; p += 64) out[p] = ninf;
  }
}

// ---- the quantising append: one wave per row of k_new
template <typename T>
__global__ __launch_bounds__(64) void ffpa_mla_index_k_append_fp8_kernel(const MlaIndexKAppendFp8Args a) {
  typedef T v2 __attribute__((ext_vector_type(2)));
  const int t = (int)blockIdx.x, lane = (int)threadIdx.x;

  // ---- wave-uniform, in front of the first store: the row's sequence, its cache position, its page
  int b = a.B, i = -1;
  if (a.cu_seqlens_q != nullptr) {
    b = cu_seqlens_find(a.cu_seqlens_q, a.B, a.T, t);  // (a.B: a padding row, or a workgroup of the grid that only writes lens_after)
    if (b < a.B) i = t - a.cu_seqlens_q[b];            // (negative under a cu_seqlens_q that does not ascend: the row is dropped)
  } else if (t < a.T) {
    const int S = a.T / a.B;
    b = t / S, i = t - b * S;
  }
  const int64_t cap = (int64_t)a.W * a.page_size;
  bool keep = b < a.B && i >= 0;
  int64_t pos = 0;
  if (keep) {
    const int len = a.cache_seqlens[b];
    pos = (int64_t)(len > 0 ? len : 0) + i;
    keep = pos < cap;
  }
  int page = 0;
  if (keep) {  // (pos < cap: pos / page_size < W, the table's row is not left)
    page = a.block_table != nullptr ? a.block_table[(int64_t)b * a.s_table + pos / a.page_size] : b;
    page = clampi(page, 0, a.num_pages - 1);
  }

  const int64_t s = (int64_t)t * 64 + lane;
  if (s < a.B) {
    const int len = a.cache_seqlens[s];
    const int nnew = a.cu_seqlens_q != nullptr ? a.cu_seqlens_q[s + 1] - a.cu_seqlens_q[s] : a.T / a.B;
    const int64_t u = (int64_t)(len > 0 ? len : 0) + nnew;
    a.lens_after[s] = (int)(u < cap ? u : cap);
  }
  if (!keep) return;

  const v2 x = *reinterpret_cast<const v2*>(static_cast<const T*>(a.k_new) + (int64_t)t * a.s_new + 2 * lane);
  const float x0 = (float)x[0], x1 = (float)x[1];
  float amax = fmaxf(fabsf(x0), fabsf(x1));
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));
  uint32_t bits = __float_as_uint(fmaxf(amax, 1e-4f) / 448.f);
  bits = (bits & 0x7F800000u) + ((bits & 0x007FFFFFu) != 0u ? 0x00800000u : 0u);  // up to a power of two
  const float inv = __uint_as_float(0x7F000000u - bits);                           // its exact reciprocal: exponent 254 - E
  float v[2] = {x0 * inv, x1 * inv};
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float c = fminf(fmaxf(v[e], -448.f), 448.f);
    v[e] = v[e] != v[e] ? v[e] : c;
  }
  const int codes = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
  const int row = (int)(pos % a.page_size);
  uint8_t* base = a.k + (int64_t)page * a.s_k_page;
  *reinterpret_cast<uint16_t*>(base + (int64_t)row * kMlaIndexFp8Dim + 2 * lane) = (uint16_t)codes;
  if (lane == 0) *reinterpret_cast<float*>(base + (int64_t)a.page_size * kMlaIndexFp8Dim + 4 * (int64_t)row) = __uint_as_float(bits);
}

}  // namespace

// a.Hi in {32, 64}, a.chunk in {256, 512, 1024} and T * ceil(N / chunk) <= 2^24 are the caller's checks
int launch_mla_index_scores_fp8(const MlaIndexScoresFp8Args& a, hipStream_t stream) {
  if (a.T == 0) return 0;
  const unsigned grid = (unsigned)a.T * (unsigned)((a.N + a.chunk - 1) / a.chunk);
  if (a.Hi == 32)
    hipLaunchKernelGGL(ffpa_mla_index_scores_fp8_kernel<2>, dim3(grid), dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(ffpa_mla_index_scores_fp8_kernel<4>, dim3(grid), dim3(kThreads), 0, stream, a);
  return (int)hipGetLastError();
}

// one workgroup (one wave) per row of k_new, and at least ceil(B / 64) of them: lens_after is written for every sequence, with T = 0 too
int launch_mla_index_k_append_fp8(const MlaIndexKAppendFp8Args& a, hipStream_t stream) {
  const unsigned lens_wgs = (unsigned)((a.B + 63) / 64);
  const unsigned grid = (unsigned)a.T > lens_wgs ? (unsigned)a.T : lens_wgs;
  if (a.fp16)
    hipLaunchKernelGGL(ffpa_mla_index_k_append_fp8_kernel<_Float16>, dim3(grid), dim3(64), 0, stream, a);
  else
    hipLaunchKernelGGL(ffpa_mla_index_k_append_fp8_kernel<__bf16>, dim3(grid), dim3(64), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace ffpa
