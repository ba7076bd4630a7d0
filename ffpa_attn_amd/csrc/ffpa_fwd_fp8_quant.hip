// ffpa_fwd_fp8_quant.hip — the pre-pass of the FP8 attention forward (ffpa_attn_fp8_quantize, ffpa_capi.hip): three launches that turn bf16 / fp16 q, k, v into
// the e4m3 scratch the attention kernel reads (ffpa_fwd_fp8.h: the layout).  quantize_attn_fp8 (ffpa_attn_amd/interface.py) is the definition; these kernels
// write its bytes.  Plain C++, no inline assembly.
//
//   1. fp8_stats_kernel      per (key tile, batch, KV head): channel d's K sum over the tile's keys, added in key order in fp32, and its largest |v|.
//   2. fp8_finalize_kernel   per (batch, KV head): kmean[d] = (the tiles' sums added in tile order) / float32(Nkv) (0 without smooth_k), and
//                            v_scale[d] = pow2_up(max(amax, 1e-4) / 448).
//   3. fp8_codes_kernel      one workgroup per Q8 tile, then one per (K8, V8T) tile: the tile's largest |x| (x = float32(q) * q_premul, or float32(k) - kmean),
//                            scale = pow2_up(max(amax, 1e-4) / 448), code = rne_e4m3(clamp(x / scale, +-448)); V's codes with its channel's scale.
// Every float32 operation is one the helper states in the same order: the sums are sequential, the division by 448 and by Nkv IEEE, the division by a scale a
// multiplication by its exact reciprocal.  pow2_up works on the exponent bits (a non-zero mantissa: exponent + 1, mantissa cleared), as the index keys' append does.
// Finite inputs are the contract.  A row at or past Nq / Nkv and a column at or past D become no address; they are zero codes.
#include "ffpa_fwd_fp8.h"

namespace ffpa {
namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;

__device__ __forceinline__ uint32_t pow2_up_bits(float amax) {
  const uint32_t bits = __float_as_uint(fmaxf(amax, 1e-4f) / 448.f);
  return (bits & 0x7F800000u) + ((bits & 0x007FFFFFu) != 0u ? 0x00800000u : 0u);
}
__device__ __forceinline__ float recip_pow2(uint32_t bits) { return __uint_as_float(0x7F000000u - bits); }  // exponent 254 - E

__device__ __forceinline__ float clamp448(float x) { return fminf(fmaxf(x, -448.f), 448.f); }

// 16 float32 -> 16 codes
__device__ __forceinline__ i32x4 codes16(const float (&x)[16]) {
  i32x4 out;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    int pk = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w], x[4 * w + 1], 0, false);
    out[w] = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w + 2], x[4 * w + 3], pk, true);
  }
  return out;
}

// the workgroup's maximum of a non-negative value, known to every thread (red: 4 floats of LDS)
__device__ __forceinline__ float block_max(float x, float* red) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x = fmaxf(x, __shfl_xor(x, s, 64));
  __syncthreads();  // (red may still be read from the call before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

template <typename T>
__global__ __launch_bounds__(256) void fp8_stats_kernel(const Fp8QuantArgs a) {
  const int t = (int)blockIdx.x, bh = (int)blockIdx.y, b = bh / a.Hkv, h = bh % a.Hkv;
  const int NT = (int)gridDim.x;
  const T* const k = static_cast<const T*>(a.k) + (int64_t)b * a.s_k[0] + (int64_t)h * a.s_k[1];
  const T* const v = static_cast<const T*>(a.v) + (int64_t)b * a.s_v[0] + (int64_t)h * a.s_v[1];
  const int keys = min(kFp8BlockKeys, a.Nkv - t * kFp8BlockKeys);
  for (int d = (int)threadIdx.x; d < a.D; d += 256) {
    float sum = 0.f, amax = 0.f;
    for (int j = 0; j < keys; ++j) {
      const int64_t key = (int64_t)t * kFp8BlockKeys + j;
      sum += (float)k[key * a.s_k[2] + d];
      amax = fmaxf(amax, fabsf((float)v[key * a.s_v[2] + d]));
    }
    const int64_t at = ((int64_t)bh * NT + t) * a.D + d;
    a.ksum_part[at] = sum, a.vamax_part[at] = amax;
  }
}

__global__ __launch_bounds__(256) void fp8_finalize_kernel(const Fp8QuantArgs a) {
  const int bh = (int)blockIdx.x;
  const int NT = (a.Nkv + kFp8BlockKeys - 1) / kFp8BlockKeys;
  for (int d = (int)threadIdx.x; d < a.D; d += 256) {
    float sum = 0.f, amax = 0.f;
    for (int t = 0; t < NT; ++t) {
      const int64_t at = ((int64_t)bh * NT + t) * a.D + d;
      sum += a.ksum_part[at];
      amax = fmaxf(amax, a.vamax_part[at]);
    }
    a.kmean[(int64_t)bh * a.D + d] = a.smooth_k ? sum / (float)a.Nkv : 0.f;
    a.v_scale[(int64_t)bh * a.D + d] = __uint_as_float(pow2_up_bits(amax));
  }
}

// 16 contiguous elements of a row as float32 (the row 16-byte aligned, d0 a multiple of 16), or zeros
template <typename T>
__device__ __forceinline__ void load16(float (&x)[16], const T* row, int d0, bool valid) {
  typedef T v8 __attribute__((ext_vector_type(8)));
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = 0.f;
  if (valid) {
    const v8 lo = *reinterpret_cast<const v8*>(row + d0), hi = *reinterpret_cast<const v8*>(row + d0 + 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (float)lo[e], x[8 + e] = (float)hi[e];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fp8_codes_kernel(const Fp8QuantArgs a) {
  __shared__ float red[4];
  const int tid = (int)threadIdx.x;
  const int NC = fp8_padded_dim(a.D) / 128;
  const int RT = (a.Nq + kFp8BlockRows - 1) / kFp8BlockRows, NT = (a.Nkv + kFp8BlockKeys - 1) / kFp8BlockKeys;
  const int64_t qjobs = (int64_t)a.B * a.Hq * RT;
  const int64_t job = (int64_t)blockIdx.x;

  if (job < qjobs) {
    // ---- a Q8 tile: piece ch of 16 bytes is fragment ch / 128 = (row block, chunk), plane (ch % 128) / 64, lane ch % 64
    const int rt = (int)(job % RT), hq = (int)((job / RT) % a.Hq), b = (int)(job / ((int64_t)RT * a.Hq));
    const T* const q = static_cast<const T*>(a.q) + (int64_t)b * a.s_q[0] + (int64_t)hq * a.s_q[1];
    const int pieces = kFp8BlockRows / 16 * NC * 128;
    float amax = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
      float inv = 0.f;
      if (pass == 1) {
        const uint32_t bits = pow2_up_bits(block_max(amax, red));
        if (tid == 0) a.q_scale[job] = __uint_as_float(bits);
        inv = recip_pow2(bits);
      }
      for (int ch = tid; ch < pieces; ch += 256) {
        const int f = ch >> 7, hpl = (ch >> 6) & 1, lane = ch & 63, g = lane >> 4, r = lane & 15;
        const int row = rt * kFp8BlockRows + 16 * (f / NC) + r, d0 = 128 * (f % NC) + 32 * g + 16 * hpl;
        float x[16];
        load16(x, q + (int64_t)row * a.s_q[2], d0, row < a.Nq && d0 < a.D);
#pragma unroll
        for (int e = 0; e < 16; ++e) x[e] *= a.q_premul;
        if (pass == 0) {
#pragma unroll
          for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(x[e]));
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e) x[e] = clamp448(x[e] * inv);
          *reinterpret_cast<i32x4*>(a.q8 + job * ((int64_t)kFp8BlockRows * NC * 128) + 16 * (int64_t)ch) = codes16(x);
        }
      }
    }
    return;
  }

  // ---- a (K8, V8T) tile
  const int64_t kvjob = job - qjobs;
  const int t = (int)(kvjob % NT);
  const int64_t bh = kvjob / NT;
  const int h = (int)(bh % a.Hkv), b = (int)(bh / a.Hkv);
  const T* const k = static_cast<const T*>(a.k) + (int64_t)b * a.s_k[0] + (int64_t)h * a.s_k[1];
  const T* const v = static_cast<const T*>(a.v) + (int64_t)b * a.s_v[0] + (int64_t)h * a.s_v[1];
  const float* const mean = a.kmean + bh * a.D;
  {
    const int pieces = kFp8BlockKeys / 16 * NC * 128;
    float amax = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
      float inv = 0.f;
      if (pass == 1) {
        const uint32_t bits = pow2_up_bits(block_max(amax, red));
        if (tid == 0) a.k_scale[kvjob] = __uint_as_float(bits);
        inv = recip_pow2(bits);
      }
      for (int ch = tid; ch < pieces; ch += 256) {
        const int f = ch >> 7, hpl = (ch >> 6) & 1, lane = ch & 63, g = lane >> 4, r = lane & 15;
        const int key = t * kFp8BlockKeys + 16 * (f / NC) + r, d0 = 128 * (f % NC) + 32 * g + 16 * hpl;
        const bool valid = key < a.Nkv && d0 < a.D;
        float x[16];
        load16(x, k + (int64_t)key * a.s_k[2], d0, valid);
        if (valid) {
#pragma unroll
          for (int e = 0; e < 16; ++e) x[e] -= mean[d0 + e];
        }
        if (pass == 0) {
#pragma unroll
          for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(x[e]));
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e) x[e] = clamp448(x[e] * inv);
          *reinterpret_cast<i32x4*>(a.k8 + kvjob * ((int64_t)kFp8BlockKeys * NC * 128) + 16 * (int64_t)ch) = codes16(x);
        }
      }
    }
  }
  {
    // V8T: piece ch is fragment db = ch / 128, plane, lane: channel 16 db + r, positions p = 32 g + 16 plane + e, key 16 ((p % 32) / 4) + 4 (p / 32) + p % 4
    const int pieces = a.D / 16 * 128;
    for (int ch = tid; ch < pieces; ch += 256) {
      const int db = ch >> 7, hpl = (ch >> 6) & 1, lane = ch & 63, g = lane >> 4, r = lane & 15;
      const int d = 16 * db + r;
      const float inv = recip_pow2(__float_as_uint(a.v_scale[bh * a.D + d]));
      float x[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = t * kFp8BlockKeys + 16 * (4 * hpl + e / 4) + 4 * g + e % 4;
        x[e] = key < a.Nkv ? clamp448((float)v[(int64_t)key * a.s_v[2] + d] * inv) : 0.f;
      }
      *reinterpret_cast<i32x4*>(a.v8t + kvjob * ((int64_t)kFp8BlockKeys * a.D) + 16 * (int64_t)ch) = codes16(x);
    }
  }
}

template <typename T>
int launch_all(const Fp8QuantArgs& a, hipStream_t stream) {
  const int NT = (a.Nkv + kFp8BlockKeys - 1) / kFp8BlockKeys, RT = (a.Nq + kFp8BlockRows - 1) / kFp8BlockRows;
  hipLaunchKernelGGL(fp8_stats_kernel<T>, dim3((unsigned)NT, (unsigned)(a.B * a.Hkv)), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(fp8_finalize_kernel, dim3((unsigned)(a.B * a.Hkv)), dim3(256), 0, stream, a);
  const int64_t jobs = (int64_t)a.B * a.Hq * RT + (int64_t)a.B * a.Hkv * NT;
  hipLaunchKernelGGL(fp8_codes_kernel<T>, dim3((unsigned)jobs), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace

// B * Hkv <= 65535 (the stats grid's y) and B * (Hq * row tiles + Hkv * key tiles) < 2^31 are the caller's checks
int launch_fwd_fp8_quantize(const Fp8QuantArgs& a, hipStream_t stream) { return a.fp16 ? launch_all<_Float16>(a, stream) : launch_all<__bf16>(a, stream); }

}  // namespace ffpa
