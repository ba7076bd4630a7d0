// ffpa_mla_index_scores.hip — the score launch of DeepSeek-V3.2's "lightning indexer" (ffpa_attn_mla_index_scores, ffpa_capi.hip): from the step's index queries,
// the paged pool of index keys and the per-head weights to the float32 scores [T, N] the selection (ffpa_mla_sparse_topk.hip) takes, -inf tail included, in one
// kernel.  A TU of its own; the MFMAs are compiler builtins (the hazard padding is the compiler's), every store is an ordinary vector store.
//
// THE RESULT.  Token t is token i of sequence b (cu_seqlens_q and its binary search, or t / Sq and t % Sq — the selection's rule, to the letter), which has S
// query tokens and length L = cache_seqlens[b]; it sees the key positions [0, n), n = clamp(L - (S - 1 - i), 0, N) under causal, clamp(L, 0, N) otherwise, and
// never more than the table (W * page_size) or the capacity can name.  Key p of sequence b is row p % page_size of page table[b, min(p / page_size, W - 1)], the
// page id clamped into [0, num_pages - 1].
//     scores[t, p] = sum_h w[t, h] * max(0, sum_d q[t, h, d] * k[b, p, d])   for p < n,        -inf for n <= p < N  (a padding row: all -inf)
// with fp32 products and sums.
//
// HOW.  A skinny GEMM — M = the token's Hi heads, N = keys, K = 128 — with a non-linear reduction over M, streaming the pool once.
//   * One workgroup of 4 waves per (token, chunk of `chunk` consecutive key positions), the chunk the fastest grid index: the tokens of one sequence are
//     neighbours in launch order and re-read their keys from L2.  A wave walks its quarter of the chunk in steps of 64 keys.
//   * v_mfma_f32_16x16x32 with A = Q (heads are the rows) and B = K (keys are the columns), both straight from global memory in the MFMA's own layout: lane l
//     holds 16 bytes of row l % 16, columns 32 ks + 8 (l / 16) ... of k-step ks.  A key row is consumed by exactly one wave, so nothing goes through LDS.  Q —
//     Hi / 16 head blocks x 4 k-steps, 64 VGPRs at Hi = 64 — is loaded once and lives as long as the wave; a 64-key step is 16 loads of K, and the NEXT step's
//     16 are issued in front of this step's MFMAs (two register buffers, the loop unrolled by two so that no buffer is copied).
//   * The page of a 64-key step is one wave-uniform table read (page_size % 64 == 0), taken with the loads, a step ahead; the page index and the row inside
//     the page are carried along, so the wave divides by page_size once.
//   * Rows at and past n are never turned into an address: the key is clamped into [step's first key, n - 1] — the same 64-key block, the same page — and the
//     result masked.
//   * C comes out with lane l holding key l % 16 and heads 16 hb + 4 (l / 16) + i: max(0, .) times the lane's four weights (fp32, held in that layout) sums
//     in-lane over i and hb, two cross-lane adds (xor 16, xor 32) finish the heads.  After the four key blocks lane l keeps block l / 16's total and stores key
//     64 step + l: one coalesced 256-byte store per wave and step.  No LDS, no atomics, no barrier.
//   * Positions in [n, N) are stored as -inf by the wave that owns them; a wave whose quarter starts at or past n loads nothing.
// The wave-uniform reads — the sequence search, the length — stand in front of the first store.  Addresses are 64-bit.  Every index that becomes an address is
// bounded first: a head by Hi, a key by n <= min(N, W * page_size), a table column by W - 1, a page id by num_pages - 1, an output column by N.
#include "ffpa_mla_index_scores.h"

#include "ffpa_cu_seqlens_find.h"

namespace ffpa {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStep = 64;                    // keys per wave and step: four 16-key MFMA column blocks
constexpr int kKSteps = kMlaIndexDim / 32;   // MFMA k-steps over the 128 columns

typedef __attribute__((ext_vector_type(4))) float f32x4;

template <typename T>
struct Frag {
  typedef __attribute__((ext_vector_type(8))) T v8;
};

__device__ __forceinline__ f32x4 mfma(Frag<__bf16>::v8 a, Frag<__bf16>::v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma(Frag<_Float16>::v8 a, Frag<_Float16>::v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// where a wave stands in its sequence's keys: the step's first key, its page's index in the table row and its first row inside that page
struct Walk {
  int p0, pidx, row0;
};

// the 16 fragments of the 64-key step at `at`: key block kb, k-step ks.  Keys at and past n read key n - 1 (at.p0 < n: the same block, the same page).
template <typename T>
__device__ __forceinline__ void load_step(typename Frag<T>::v8 (&kf)[4][kKSteps], const MlaIndexScoresArgs& a, const int* table, int b, int n, Walk at, int r, int g) {
  int page = table != nullptr ? table[min(at.pidx, a.W - 1)] : b;  // wave-uniform
  page = clampi(page, 0, a.num_pages - 1);
  const T* base = static_cast<const T*>(a.k) + (int64_t)page * a.s_k_page + 8 * g;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    const int row = at.row0 + min(16 * kb + r, n - 1 - at.p0);
    const T* src = base + (int64_t)row * a.s_k_row;
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) kf[kb][ks] = *reinterpret_cast<const typename Frag<T>::v8*>(src + 32 * ks);
  }
}

// the 64 scores of a step: lane l returns the score of key at.p0 + l
template <typename T, int HB>
__device__ __forceinline__ float score_step(const typename Frag<T>::v8 (&qf)[HB][kKSteps], const float (&wf)[HB][4], const typename Frag<T>::v8 (&kf)[4][kKSteps],
                                            int g) {
  float mine = 0.f;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    float part = 0.f;
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < kKSteps; ++ks) acc = mfma(qf[hb][ks], kf[kb][ks], acc);
#pragma unroll
      for (int i = 0; i < 4; ++i) part = fmaf(wf[hb][i], fmaxf(acc[i], 0.f), part);
    }
    part += __shfl_xor(part, 16, 64);
    part += __shfl_xor(part, 32, 64);
    if (g == kb) mine = part;
  }
  return mine;
}

template <typename T, int HB>
__global__ __launch_bounds__(kThreads) void ffpa_mla_index_scores_kernel(const MlaIndexScoresArgs a) {
  typedef typename Frag<T>::v8 v8;
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int nchunks = (a.N + a.chunk - 1) / a.chunk;
  const int t = (int)(blockIdx.x / (unsigned)nchunks), chunk = (int)(blockIdx.x % (unsigned)nchunks);

  // ---- wave-uniform: the token's sequence, its visible length
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
    // ---- Q and the weights, once: lane l holds head 16 hb + l % 16 of A, and the weights of the heads 16 hb + 4 (l / 16) + i its C values belong to
    v8 qf[HB][kKSteps];
    float wf[HB][4];
    {
      const T* qrow = static_cast<const T*>(a.q) + (int64_t)t * a.s_q_tok + 8 * g;
      const float* wrow = a.w + (int64_t)t * a.s_w;
#pragma unroll
      for (int hb = 0; hb < HB; ++hb) {
#pragma unroll
        for (int ks = 0; ks < kKSteps; ++ks) qf[hb][ks] = *reinterpret_cast<const v8*>(qrow + (int64_t)(16 * hb + r) * a.s_q_head + 32 * ks);
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
    // Two register buffers, the loop unrolled by two.  No load stands behind a condition of its own: between the loads of a step and its MFMAs lie exactly the
    // 16 loads of the next one, so the wait in front of the MFMAs is for the older 16 alone (a conditional prefetch would make it a wait for all of them).
    v8 k0[4][kKSteps], k1[4][kKSteps];
    load_step<T>(k0, a, table, b, n, at, r, g);
    int left = live;
    while (left > 2) {
      const Walk at1 = next(at), at2 = next(at1);
      load_step<T>(k1, a, table, b, n, at1, r, g);
      store(at, score_step<T, HB>(qf, wf, k0, g));
      load_step<T>(k0, a, table, b, n, at2, r, g);
      store(at1, score_step<T, HB>(qf, wf, k1, g));
      at = at2, left -= 2;
    }
    if (left == 2) {
      const Walk at1 = next(at);
      load_step<T>(k1, a, table, b, n, at1, r, g);
      store(at, score_step<T, HB>(qf, wf, k0, g));
      store(at1, score_step<T, HB>(qf, wf, k1, g));
    } else {
      store(at, score_step<T, HB>(qf, wf, k0, g));
    }
    for (int p = begin + live * kStep + lane; p < end; p += 64) out[p] = ninf;
  } else {
    for (int p = begin + lane; p < end; p += 64) out[p] = ninf;
  }
}

template <typename T>
int launch_for(const MlaIndexScoresArgs& a, unsigned grid, hipStream_t stream) {
  if (a.Hi == 32)
    hipLaunchKernelGGL((ffpa_mla_index_scores_kernel<T, 2>), dim3(grid), dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((ffpa_mla_index_scores_kernel<T, 4>), dim3(grid), dim3(kThreads), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace

// a.Hi in {32, 64}, a.chunk in {256, 512, 1024} and T * ceil(N / chunk) <= 2^24 are the caller's checks
int launch_mla_index_scores(const MlaIndexScoresArgs& a, hipStream_t stream) {
  if (a.T == 0) return 0;
  const unsigned grid = (unsigned)a.T * (unsigned)((a.N + a.chunk - 1) / a.chunk);
  return a.fp16 ? launch_for<_Float16>(a, grid, stream) : launch_for<__bf16>(a, grid, stream);
}

}  // namespace ffpa
