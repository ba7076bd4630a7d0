// ffpa_fwd_fp8_inst.hip — the FP8 attention forward of one head dim (-DFFPA_INST_D in {256, 320, 384, 448, 512}): both products on
// v_mfma_f32_16x16x128_f8f6f4 (OCP e4m3 x e4m3, fp32 accumulators, no block scales), over the scratch ffpa_fwd_fp8_quant.hip writes (ffpa_fwd_fp8.h: the layout).
// The MFMA is a compiler builtin (the hazard padding is the compiler's), every store is an ordinary vector store, there is no inline assembly.
//
// THE WORK SPLIT.  One workgroup of 4 waves per (batch, query head, tile of 64 query rows); a wave owns kRB = 1 row block of 16 rows and the whole head dim
// (kRB = 2 — an A fragment read from LDS feeding two row blocks — needs 355 spilled registers at D = 512 as the loops stand, and is not built).  Both
// products are computed TRANSPOSED, the 16 query rows as the B operand:
//     S^T (16 keys x 16 rows) = K8 fragment (A) . Q8 fragment (B), summed over the NC = ceil(D / 128) column chunks,
//     O^T (16 channels x 16 rows) += V8T fragment (A) . P^T (B), ONE instruction per 16 channels: the contraction is the tile's 128 keys.
// Lane l = 16 g + r then holds, of its row block, row r: in accumulator kb of S^T
// the keys 16 kb + 4 g + i, in accumulator db of O^T the channels 16 db + 4 g + i (i = 0 .. 3).
//   * THE ROW STATISTICS are per lane: the row maximum is an in-lane max over 32 scores and two cross-lane steps (xor 16, xor 32); the row sum stays a per-lane
//     partial until the epilogue.
//   * P NEVER MOVES.  The B operand of the PV MFMA wants, in register j byte i of lane group g, contraction position 32 g + 4 j + i.  Accumulator j of S^T holds
//     key 16 j + 4 g + i in element i: four probabilities become one register with two v_cvt_pk_fp8_f32, and the pre-pass has stored V8T with key
//     16 j + 4 g + i AT position 32 g + 4 j + i.  No lane exchange, no LDS round trip.
//   * THE P SCALE AND THE RESCALE.  The running maximum is exact (O and l are rescaled whenever it grows; a step that leaves every row's maximum where it was — a
//     wave-uniform test — skips the multiplications): p <= 1, and p * 2^8 <= 256 < 448 converts without saturation.  2^-8 is undone in the epilogue with v_scale / l.
//   * Registers at D = 512: O^T 32 x 4 = 128, Q8 4 x 8 = 32, S^T 8 x 4 = 32 (dead once P is packed: 8), 32 staging; the compiler allocates 396, no scratch.
//   * LDS: the K8 tile (128 x DP bytes) and the V8T tile (128 x D bytes) of the current step, 128 KiB at D = 512, single-buffered per product and filled ACROSS
//     the other product: V8T(t) travels global -> registers -> LDS in two halves under the QK^T MFMAs of step t, K8(t + 1) under its PV MFMAs.  Two barriers per
//     step: behind the softmax (V8T(t) complete, K8(t) no longer read) and behind the PV MFMAs (K8(t + 1) complete, V8T(t) no longer read).
//   * Causal launches (key j visible to row i iff j <= i + Nkv - Nq) walk only the key tiles below the tile's last row; elements are tested only in tiles that
//     reach past the first row's limit or past Nkv.  A row without a visible key keeps m = -inf, l = 0 and stores 0.
// Every address is 64-bit; a tile index is < the tiles the scratch was sized for, an output row < Nq.
#include "ffpa_fwd_fp8.h"
#include "ffpa_launch_kernel.h"

#ifndef FFPA_INST_D
#error "ffpa_fwd_fp8_inst.hip is compiled once per head dim: -DFFPA_INST_D=<256 | 320 | 384 | 448 | 512>"
#endif

namespace ffpa {
namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int kRB = kFp8BlockRows / 64;  // row blocks of 16 per wave
constexpr int kKB = kFp8BlockKeys / 16;  // key blocks of 16 per tile: the registers of a P^T operand
static_assert(kKB == 8, "a P^T operand is 8 registers: 128 keys per tile");

// a lane's operand out of a 2 KiB fragment: 16 bytes from each plane
__device__ __forceinline__ i32x8 fragment(const uint8_t* f, int lane) {
  const i32x4 lo = *reinterpret_cast<const i32x4*>(f + 16 * lane), hi = *reinterpret_cast<const i32x4*>(f + 1024 + 16 * lane);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// half `half` of a tile of 2 * N * 4 KiB, global -> registers and registers -> LDS: 16 bytes per thread and step, contiguous over the workgroup
template <int N>
__device__ __forceinline__ void fetch(i32x4 (&st)[8], const uint8_t* src, int half, int tid) {
#pragma unroll
  for (int i = 0; i < N; ++i) st[i] = *reinterpret_cast<const i32x4*>(src + 16 * ((half * N + i) * 256 + tid));
}
template <int N>
__device__ __forceinline__ void put(const i32x4 (&st)[8], uint8_t* dst, int half, int tid) {
#pragma unroll
  for (int i = 0; i < N; ++i) *reinterpret_cast<i32x4*>(dst + 16 * ((half * N + i) * 256 + tid)) = st[i];
}

template <int D, typename T>
__global__ __launch_bounds__(256) void ffpa_fwd_fp8_kernel(const Fp8FwdArgs a) {
  typedef T out4 __attribute__((ext_vector_type(4)));
  constexpr int NC = fp8_padded_dim(D) / 128, NDB = D / 16;
  constexpr int KBYTES = kFp8BlockKeys * NC * 128, VBYTES = kFp8BlockKeys * D;
  constexpr int KCH = KBYTES / 8192, VCH = VBYTES / 8192;  // 16-byte pieces per thread in HALF a tile
  static_assert(KCH <= 8 && VCH <= 8 && KCH * 8192 == KBYTES && VCH * 8192 == VBYTES && NDB % 2 == 0, "the staging registers hold half a tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint8_t* const kbuf = reinterpret_cast<uint8_t*>(smem);
  uint8_t* const vbuf = kbuf + KBYTES;

  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int RT = (a.Nq + kFp8BlockRows - 1) / kFp8BlockRows, NT = (a.Nkv + kFp8BlockKeys - 1) / kFp8BlockKeys;
  const int rt = (int)(blockIdx.x % (unsigned)RT), hq = (int)((blockIdx.x / (unsigned)RT) % (unsigned)a.Hq), b = (int)(blockIdx.x / ((unsigned)RT * (unsigned)a.Hq));
  const int hkv = hq / (a.Hq / a.Hkv);
  const int row0 = rt * kFp8BlockRows, off = a.Nkv - a.Nq;
  int nt = NT;  // key tiles with a key some row of the workgroup sees
  if (a.causal) {
    const int64_t last = (int64_t)min(row0 + kFp8BlockRows - 1, a.Nq - 1) + off;  // the last row's limit
    nt = last < 0 ? 0 : (int)min((int64_t)NT, last / kFp8BlockKeys + 1);
  }
  const int64_t qtile = ((int64_t)b * a.Hq + hq) * RT + rt, kvhead = (int64_t)b * a.Hkv + hkv;
  const uint8_t* const ktiles = a.k8 + kvhead * NT * KBYTES;
  const uint8_t* const vtiles = a.v8t + kvhead * NT * VBYTES;
  const float qs = a.q_scale[qtile];
  const float ninf = -__builtin_inff();

  i32x8 qf[kRB][NC];
  f32x4 o[kRB][NDB];
  float m[kRB], l[kRB];
#pragma unroll
  for (int rb = 0; rb < kRB; ++rb) {
    m[rb] = ninf, l[rb] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) qf[rb][c] = fragment(a.q8 + qtile * (kFp8BlockRows * NC * 128) + (int64_t)((wave * kRB + rb) * NC + c) * 2048, lane);
#pragma unroll
    for (int db = 0; db < NDB; ++db) o[rb][db] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  i32x4 st[8];
  if (nt > 0) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      fetch<KCH>(st, ktiles, half, tid);
      put<KCH>(st, kbuf, half, tid);
    }
  }
  __syncthreads();

  for (int t = 0; t < nt; ++t) {
    // ---- S^T = K8 . Q8^T, V8T(t) on its way into LDS
    const uint8_t* const vt = vtiles + (int64_t)t * VBYTES;
    f32x4 s[kRB][kKB];
    fetch<VCH>(st, vt, 0, tid);
#pragma unroll
    for (int kb = 0; kb < kKB; ++kb) {
      if (kb == kKB / 2) {
        put<VCH>(st, vbuf, 0, tid);
        fetch<VCH>(st, vt, 1, tid);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const i32x8 kf = fragment(kbuf + (kb * NC + c) * 2048, lane);
#pragma unroll
        for (int rb = 0; rb < kRB; ++rb) {
          const f32x4 acc = c == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : s[rb][kb];
          // (cbsz = blgp = 0: A and B are e4m3; the scale operands zero: the instruction without block scales)
          s[rb][kb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf[rb][c], acc, 0, 0, 0, 0, 0, 0);
        }
      }
    }
    put<VCH>(st, vbuf, 1, tid);

    // ---- the softmax step, in the exp2 domain, per lane: row r of each row block, keys 16 kb + 4 g + i
    const float sc = qs * a.k_scale[kvhead * NT + t];
    const int key0 = t * kFp8BlockKeys + 4 * g;
    const bool edge = key0 - 4 * g + kFp8BlockKeys > a.Nkv || (a.causal && key0 - 4 * g + kFp8BlockKeys - 1 > row0 + off);  // workgroup-uniform
    i32x8 pf[kRB];
    float alpha[kRB];
#pragma unroll
    for (int rb = 0; rb < kRB; ++rb) {
      const int row = row0 + 16 * (wave * kRB + rb) + r;
      const int lim = a.causal ? min(row + off, a.Nkv - 1) : a.Nkv - 1;  // the row's last visible key
      float mx = ninf;
#pragma unroll
      for (int kb = 0; kb < kKB; ++kb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float x = s[rb][kb][i] * sc;
          if (edge && key0 + 16 * kb + i > lim) x = ninf;
          s[rb][kb][i] = x;
          mx = fmaxf(mx, x);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m[rb], mx);
      const float m_use = m_new == ninf ? 0.f : m_new;  // (a row that has seen no key yet: p = exp2(-inf) = 0)
      alpha[rb] = __builtin_amdgcn_exp2f(m[rb] - m_use);
      float psum = 0.f;
#pragma unroll
      for (int kb = 0; kb < kKB; ++kb) {
        float p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          p[i] = __builtin_amdgcn_exp2f(s[rb][kb][i] - m_use);
          psum += p[i];
        }
        constexpr float up = (float)(1 << kFp8PShift);
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(p[0] * up, p[1] * up, 0, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(p[2] * up, p[3] * up, pk, true);
        pf[rb][kb] = pk;
      }
      l[rb] = l[rb] * alpha[rb] + psum;
      m[rb] = m_new;
    }
    bool same = true;
#pragma unroll
    for (int rb = 0; rb < kRB; ++rb) same = same && alpha[rb] == 1.f;
    if (!__all(same)) {
#pragma unroll
      for (int rb = 0; rb < kRB; ++rb)
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[rb][db] *= alpha[rb];
    }
    __syncthreads();  // V8T(t) is in LDS; nobody reads K8(t) any more

    // ---- O^T += V8T . P^T, K8(t + 1) on its way into LDS
    const bool more = t + 1 < nt;
    const uint8_t* const kt = ktiles + (int64_t)(t + 1) * KBYTES;
    if (more) fetch<KCH>(st, kt, 0, tid);
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      if (db == NDB / 2 && more) {
        put<KCH>(st, kbuf, 0, tid);
        fetch<KCH>(st, kt, 1, tid);
      }
      const i32x8 vf = fragment(vbuf + db * 2048, lane);
#pragma unroll
      for (int rb = 0; rb < kRB; ++rb) o[rb][db] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf[rb], o[rb][db], 0, 0, 0, 0, 0, 0);
    }
    if (more) put<KCH>(st, kbuf, 1, tid);
    __syncthreads();  // K8(t + 1) is in LDS; nobody reads V8T(t) any more
  }

  // ---- O = O^T / (l 2^8) . v_scale: the division is the one rounding in front of the output's, the scale product behind it exact (a power of two).  The
  // division comes FIRST: O^T reaches 2^8 . 448 . l and O^T . v_scale leaves fp32 once v_scale passes about 2^110 (|v| ~ 2^118, bf16 only), where the quotient (<= 448 v_scale) is still finite
  const float* const vscale = a.v_scale + kvhead * D;
#pragma unroll
  for (int rb = 0; rb < kRB; ++rb) {
    float lt = l[rb];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    const float den = lt * (float)(1 << kFp8PShift);
    const int row = row0 + 16 * (wave * kRB + rb) + r;
    if (row < a.Nq) {
      T* const orow = static_cast<T*>(a.o) + (int64_t)b * a.s_o[0] + (int64_t)hq * a.s_o[1] + (int64_t)row * a.s_o[2];
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const f32x4 vs = *reinterpret_cast<const f32x4*>(vscale + 16 * db + 4 * g);
        out4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = (T)(lt > 0.f ? o[rb][db][i] / den * vs[i] : 0.f);
        *reinterpret_cast<out4*>(orow + 16 * db + 4 * g) = y;
      }
    }
  }
}

}  // namespace

#define FFPA_FP8_CAT_(a, b) a##b
#define FFPA_FP8_CAT(a, b) FFPA_FP8_CAT_(a, b)
int FFPA_FP8_CAT(launch_fwd_fp8_d, FFPA_INST_D)(const Fp8FwdArgs& a, hipStream_t stream) {
  constexpr int D = FFPA_INST_D;
  const int wgs = a.B * a.Hq * ((a.Nq + kFp8BlockRows - 1) / kFp8BlockRows);
  const int lds = kFp8BlockKeys * (fp8_padded_dim(D) + D);
  if (a.fp16) return launch_kernel<ffpa_fwd_fp8_kernel<D, _Float16>>(wgs, lds, stream, a);
  return launch_kernel<ffpa_fwd_fp8_kernel<D, __bf16>>(wgs, lds, stream, a);
}

}  // namespace ffpa
