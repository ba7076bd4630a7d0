// ffpa_bwd_kernel.h — the attention backward for head dims 513 ... 1024 (ffpa_attn_bwd, ffpa_capi.hip): the arguments, the launchers of the four builds
// (ffpa_bwd_inst.hip, -DFFPA_INST_D in {640, 768, 896, 1024}) and, for that unit alone (FFPA_BWD_KERNELS), the three kernels.  A header of its own: no other
// kernel object sees it.  The MFMAs and the transpose reads are compiler builtins (the hazard padding is the compiler's), every store is an ordinary vector
// store, there are no atomics and no inline assembly: two runs give the same bits.
//
// THE THREE LAUNCHES (one stream, in this order)
//   1. ffpa_bwd_delta_kernel      one wave per row of the PADDED row axis (NqP = Nq rounded up to 32): delta = sum_d dO . O - dlse and lse2 = LSE log2(e) into the
//                                 caller's scratch.  A row whose LSE is -inf (it saw no key) and a padding row get lse2 = +inf and delta = 0: P = exp2(s - inf) = 0.
//   2. ffpa_bwd_dkdv_kernel<T, D> one workgroup of 4 waves per (batch, KV head, tile of 16 keys); it walks the query heads of the group and their tiles of 32
//                                 rows (under the causal flag from the first tile that sees the key tile), so GQA needs neither expanded K / V nor a reduction.
//   3. ffpa_bwd_dq_kernel<T, D>   one workgroup per (batch, query head, tile of 32 rows); it walks the tiles of 32 keys (under the causal flag up to the diagonal).
//
// THE WORK SPLIT OF 2 AND 3: the head dim in quarters.  Wave w owns columns [w D / 4, (w + 1) D / 4) of the accumulators — dK^T and dV^T in 2, dQ^T in 3, fp32 —
// and reads only that quarter of Q, dO, K and V.  Per step it forms a PARTIAL S = Q_q K_q^T and dP = dO_q V_q^T on v_mfma_f32_16x16x32 (contraction: its columns),
// the four partials meet in LDS (every wave writes its own, a barrier, every wave adds all four in wave order: the same bits in each), and every wave then holds
//     P = exp2(S scale log2(e) - lse2)   and   dS = P o (dP - delta),
// rounded once to T.  The accumulators are indexed [column 4 g + i][key or row r] in lane 16 g + r, so that
//   * P and dS NEVER MOVE: the score accumulators hold, for lane (r, g), rows (2) / keys (3) 4 g + i of both 16-blocks of the step's 32 — the B operand of the
//     second product wants contraction positions 8 g + j, and position 8 g + j stands for element 4 g + j of block 0 (j < 4) or of block 1 (j >= 4);
//   * the A operand — dO^T, Q^T (2) or K^T (3), [16 columns][32 rows or keys] — is two ds_read_b64_tr_b16 from the wave's row-major image of its quarter of the tile
//     (lane n of group g addresses row 4 g + n / 4, columns 4 (n % 4) ..., and receives column n of rows 4 g ... 4 g + 3; the second read is 16 rows on);
//   * a lane stores 4 consecutive columns of one key / row: 8 bytes.
//     dV^T += dO^T P      dK^T += Q^T dS      dQ^T += K^T dS^T      (scale is applied to dK and dQ once, in fp32, at the store)
// LDS: per wave the image(s) of its quarter — 32 rows of D / 4 columns, the row stride padded by 32 bytes so that the 8 rows a 32-lane half reads fall into
// different banks — then the exchange area.  2: Q and dO images, 4 x 4 KiB exchange: 152 KiB at D = 1024.  3: the K image, 4 x 8 KiB exchange: 100 KiB.
// The fragments of a step that feed the FIRST products are loaded global -> registers one step ahead (they are the image's source too).
// Two barriers per step: behind the partials' writes and behind the second products (the exchange area is written again, the images are wave-private).
// Rows at and past Nq, keys at and past Nkv and columns at and past d_valid are never read: their fragments are zeros, P is forced to 0 for them, nothing of
// them is stored.  Every address is 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ffpa {

constexpr int kBwdRows = 32;      // rows of a row tile (kernels 2 and 3) — the contraction of dK^T / dV^T
constexpr int kBwdKeysDkdv = 16;  // keys of a workgroup of kernel 2
constexpr int kBwdKeysDq = 32;    // keys of a step of kernel 3 — the contraction of dQ^T

constexpr int bwd_padded_dim(int d) { return d <= 640 ? 640 : (d + 127) / 128 * 128; }
constexpr int bwd_image_bytes(int D) { return kBwdRows * (D / 4 * 2 + 32); }
constexpr int bwd_dkdv_lds_bytes(int D) { return 8 * bwd_image_bytes(D) + 4 * 4096; }
constexpr int bwd_dq_lds_bytes(int D) { return 4 * bwd_image_bytes(D) + 4 * 8192; }

struct BwdArgs {
  const void *q, *k, *v, *o, *dout;  // 16-bit, last dim contiguous
  const float *lse, *dlse;           // [B, Hq, Nq] contiguous; dlse may be NULL
  void *dq, *dk, *dv;
  float *lse2, *delta;               // scratch, [B, Hq, NqP] each
  int64_t sq[3], sk[3], sv[3], so[3], sdo[3], sdq[3], sdk[3], sdv[3];  // elements: {batch, head, row}
  int B, Hq, Hkv, Nq, Nkv, NqP, d_valid, causal, fp16;
  float scale, scale_log2;
};

// one per padded head dim (ffpa_bwd_inst.hip): the three launches; 0, or launch_kernel's error
#define FFPA_BWD_DECLARE(d) int launch_bwd_d##d(const BwdArgs& a, hipStream_t stream);
FFPA_BWD_DECLARE(640)
FFPA_BWD_DECLARE(768)
FFPA_BWD_DECLARE(896)
FFPA_BWD_DECLARE(1024)
#undef FFPA_BWD_DECLARE

#ifdef FFPA_BWD_KERNELS
namespace bwd {

typedef __attribute__((ext_vector_type(4))) float f32x4;
#define FFPA_BWD_LDS __attribute__((address_space(3)))

template <typename T>
struct Elem;
template <>
struct Elem<__bf16> {
  typedef __attribute__((ext_vector_type(8))) __bf16 v8;
  typedef __attribute__((ext_vector_type(4))) __bf16 v4;
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ v4 tr_read(const char* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((FFPA_BWD_LDS v4*)p); }
};
template <>
struct Elem<_Float16> {
  typedef __attribute__((ext_vector_type(8))) _Float16 v8;
  typedef __attribute__((ext_vector_type(4))) _Float16 v4;
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ v4 tr_read(const char* p) {
    typedef __attribute__((ext_vector_type(4))) short s4;
    return __builtin_bit_cast(v4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((FFPA_BWD_LDS s4*)p));
  }
};

constexpr float kLog2e = 1.4426950408889634f;

template <typename T>
__device__ __forceinline__ const T* row_ptr(const void* base, const int64_t (&s)[3], int b, int h, int row) {
  return static_cast<const T*>(base) + (int64_t)b * s[0] + (int64_t)h * s[1] + (int64_t)row * s[2];
}

// the fragments of 16 rows of one quarter: lane (r, g) holds row r, columns c0 + 32 kk + 8 g ... + 7 — zeros where the row or the columns do not exist.  Without a
// branch: such a lane reads the tensor's first 16 bytes (`safe`: always there, 16-byte aligned) and drops them
template <typename T, int NKK>
__device__ __forceinline__ void load_fragments(typename Elem<T>::v8 (&f)[NKK], const T* row, const void* safe, bool row_ok, int col, int d_valid) {
  typedef typename Elem<T>::v8 v8;
  v8 zero;
#pragma unroll
  for (int j = 0; j < 8; ++j) zero[j] = (T)0.f;
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    const bool ok = row_ok && col + 32 * kk < d_valid;
    const v8 x = *reinterpret_cast<const v8*>(ok ? row + col + 32 * kk : static_cast<const T*>(safe));
    f[kk] = ok ? x : zero;
  }
}

// ... and into the wave's image: row `row` of the image, byte column 2 * (32 kk + 8 g)
template <typename T, int NKK>
__device__ __forceinline__ void put_fragments(const typename Elem<T>::v8 (&f)[NKK], char* image_row_col) {
  typedef typename Elem<T>::v8 v8;
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) *reinterpret_cast<v8*>(image_row_col + 64 * kk) = f[kk];
}

// the A operand [16 columns cb][32 rows] out of an image: tr = the lane's transpose-read address of column block 0
template <typename T>
__device__ __forceinline__ typename Elem<T>::v8 transposed(const char* tr, int cb, int row_stride) {
  const typename Elem<T>::v4 lo = Elem<T>::tr_read(tr + 32 * cb), hi = Elem<T>::tr_read(tr + 32 * cb + 16 * row_stride);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <typename T>
__device__ __forceinline__ typename Elem<T>::v8 pack(const f32x4& lo, const f32x4& hi) {
  typename Elem<T>::v8 x;
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = (T)lo[i], x[4 + i] = (T)hi[i];
  return x;
}

// the partials of the four waves, added in wave order: N f32x4 per lane and wave, slot-major (a slot of a wave is 1 KiB, read and written 16 bytes per lane)
template <int N>
__device__ __forceinline__ void exchange(f32x4 (&x)[N], char* area, int wave, int lane) {
#pragma unroll
  for (int n = 0; n < N; ++n) *reinterpret_cast<f32x4*>(area + ((wave * N + n) * 64 + lane) * 16) = x[n];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) {
    f32x4 s = *reinterpret_cast<const f32x4*>(area + (n * 64 + lane) * 16);
#pragma unroll
    for (int w = 1; w < 4; ++w) s += *reinterpret_cast<const f32x4*>(area + ((w * N + n) * 64 + lane) * 16);
    x[n] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ffpa_bwd_delta_kernel(const BwdArgs a) {
  typedef typename Elem<T>::v8 v8;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int64_t prow = (int64_t)blockIdx.x * 4 + wave, total = (int64_t)a.B * a.Hq * a.NqP;
  if (prow >= total) return;
  const int i = (int)(prow % a.NqP);
  const int64_t bh = prow / a.NqP;
  const int h = (int)(bh % a.Hq), b = (int)(bh / a.Hq);
  float l2 = __builtin_inff(), dl = 0.f;
  if (i < a.Nq) {  // (wave-uniform)
    const T* const orow = row_ptr<T>(a.o, a.so, b, h, i);
    const T* const drow = row_ptr<T>(a.dout, a.sdo, b, h, i);
    float s = 0.f;
    for (int c = 8 * lane; c < a.d_valid; c += 512) {
      const v8 x = *reinterpret_cast<const v8*>(orow + c), y = *reinterpret_cast<const v8*>(drow + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) s = __builtin_fmaf((float)x[j], (float)y[j], s);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    const float lse = a.lse[bh * a.Nq + i];
    if (lse > -__builtin_inff()) {
      l2 = lse * kLog2e;
      dl = s - (a.dlse != nullptr ? a.dlse[bh * a.Nq + i] : 0.f);
    }
  }
  if (lane == 0) a.lse2[prow] = l2, a.delta[prow] = dl;
}

template <typename T, int D>
__global__ __launch_bounds__(256) void ffpa_bwd_dkdv_kernel(const BwdArgs a) {
  typedef Elem<T> E;
  typedef typename E::v8 v8;
  typedef T t4 __attribute__((ext_vector_type(4)));
  constexpr int DQ = D / 4, NKK = DQ / 32, NCB = DQ / 16, RS = DQ * 2 + 32, IMG = bwd_image_bytes(D);
  static_assert(DQ % 32 == 0 && IMG == kBwdRows * RS, "a quarter is whole 32-column contraction steps");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  char* const qimg = smem + wave * 2 * IMG;
  char* const oimg = qimg + IMG;
  char* const area = smem + 8 * IMG;

  const int KT = (a.Nkv + kBwdKeysDkdv - 1) / kBwdKeysDkdv, G = a.Hq / a.Hkv, off = a.Nkv - a.Nq;
  const int kt = (int)(blockIdx.x % (unsigned)KT), hkv = (int)((blockIdx.x / (unsigned)KT) % (unsigned)a.Hkv), b = (int)(blockIdx.x / ((unsigned)KT * (unsigned)a.Hkv));
  const int k0 = kt * kBwdKeysDkdv, c0 = wave * DQ, col = c0 + 8 * g;
  const int key = k0 + r;  // the key of this lane's score elements and of its B fragments
  const bool key_ok = key < a.Nkv;

  v8 kf[NKK], vf[NKK];
  load_fragments<T, NKK>(kf, row_ptr<T>(a.k, a.sk, b, hkv, key), a.k, key_ok, col, a.d_valid);
  load_fragments<T, NKK>(vf, row_ptr<T>(a.v, a.sv, b, hkv, key), a.v, key_ok, col, a.d_valid);
  f32x4 dk[NCB], dv[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) dk[cb] = dv[cb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int RT = a.NqP / kBwdRows;
  const int rt0 = a.causal ? max(0, k0 - off) / kBwdRows : 0;  // the first row tile with a row that sees key k0 (rows i >= k0 - off)
  const int nrt = RT - rt0, steps = nrt > 0 ? G * nrt : 0;
  const int put_at = r * RS + 16 * g, tr_at = (4 * g + (r >> 2)) * RS + 8 * (r & 3);  // offsets into an image: the fragment's, the transpose read's

  v8 qf[2][NKK], of[2][NKK];
  auto fetch = [&](int h, int row0) {
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int row = row0 + 16 * blk + r;
      load_fragments<T, NKK>(qf[blk], row_ptr<T>(a.q, a.sq, b, h, row), a.q, row < a.Nq, col, a.d_valid);
      load_fragments<T, NKK>(of[blk], row_ptr<T>(a.dout, a.sdo, b, h, row), a.dout, row < a.Nq, col, a.d_valid);
    }
  };
  if (steps > 0) fetch(hkv * G, rt0 * kBwdRows);
  int h = hkv * G, row0 = rt0 * kBwdRows;  // the step's query head and first row; the walk is head-major
  for (int t = 0; t < steps; ++t) {
    const bool wrap = row0 + kBwdRows >= a.NqP;
    const int h_next = wrap ? h + 1 : h, row0_next = wrap ? rt0 * kBwdRows : row0 + kBwdRows;
    // ---- the partial S and dP of this wave's columns; the fragments go into the images on the way
    f32x4 x[4];  // S block 0, S block 1, dP block 0, dP block 1: [row 4 g + i of the block][key r]
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      put_fragments<T, NKK>(qf[blk], qimg + put_at + 16 * blk * RS);
      put_fragments<T, NKK>(of[blk], oimg + put_at + 16 * blk * RS);
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        s = E::mfma(qf[blk][kk], kf[kk], s);
        dp = E::mfma(of[blk][kk], vf[kk], dp);
      }
      x[blk] = s, x[2 + blk] = dp;
    }
    if (t + 1 < steps) fetch(h_next, row0_next);
    exchange<4>(x, area, wave, lane);

    // ---- P and dS, rounded once
    const int64_t srow = ((int64_t)b * a.Hq + h) * a.NqP + row0 + 4 * g;
    f32x4 p[2], ds[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const f32x4 l2 = *reinterpret_cast<const f32x4*>(a.lse2 + srow + 16 * blk), dl = *reinterpret_cast<const f32x4*>(a.delta + srow + 16 * blk);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + 16 * blk + 4 * g + i;
        const bool seen = key_ok & (key <= (a.causal ? row + off : a.Nkv));
        const float pe = __builtin_amdgcn_exp2f(seen ? __builtin_fmaf(x[blk][i], a.scale_log2, -l2[i]) : -__builtin_inff());  // (exp2(-inf) = 0: a select, no branch)
        p[blk][i] = pe;
        ds[blk][i] = pe * (x[2 + blk][i] - dl[i]);
      }
    }
    const v8 pb = pack<T>(p[0], p[1]), dsb = pack<T>(ds[0], ds[1]);

    // ---- dV^T += dO^T P,  dK^T += Q^T dS: this wave's columns
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      dv[cb] = E::mfma(transposed<T>(oimg + tr_at, cb, RS), pb, dv[cb]);
      dk[cb] = E::mfma(transposed<T>(qimg + tr_at, cb, RS), dsb, dk[cb]);
    }
    __syncthreads();  // the exchange area is written again
    h = h_next, row0 = row0_next;
  }

  if (key_ok) {
    T* const dkrow = const_cast<T*>(row_ptr<T>(a.dk, a.sdk, b, hkv, key));
    T* const dvrow = const_cast<T*>(row_ptr<T>(a.dv, a.sdv, b, hkv, key));
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int c = c0 + 16 * cb + 4 * g;
      if (c < a.d_valid) {
        t4 yk, yv;
#pragma unroll
        for (int i = 0; i < 4; ++i) yk[i] = (T)(dk[cb][i] * a.scale), yv[i] = (T)dv[cb][i];
        *reinterpret_cast<t4*>(dkrow + c) = yk;
        *reinterpret_cast<t4*>(dvrow + c) = yv;
      }
    }
  }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void ffpa_bwd_dq_kernel(const BwdArgs a) {
  typedef Elem<T> E;
  typedef typename E::v8 v8;
  typedef T t4 __attribute__((ext_vector_type(4)));
  constexpr int DQ = D / 4, NKK = DQ / 32, NCB = DQ / 16, RS = DQ * 2 + 32, IMG = bwd_image_bytes(D);
  static_assert(kBwdKeysDq == kBwdRows, "the K image is an image of 32 rows");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  char* const kimg = smem + wave * IMG;
  char* const area = smem + 4 * IMG;

  const int RT = a.NqP / kBwdRows, G = a.Hq / a.Hkv, off = a.Nkv - a.Nq;
  const int rt = (int)(blockIdx.x % (unsigned)RT), h = (int)((blockIdx.x / (unsigned)RT) % (unsigned)a.Hq), b = (int)(blockIdx.x / ((unsigned)RT * (unsigned)a.Hq));
  const int hkv = h / G, row0 = rt * kBwdRows, c0 = wave * DQ, col = c0 + 8 * g;

  // the row tile's Q and dO fragments (B operands: row r of each block) and row statistics stay in registers
  v8 qf[2][NKK], of[2][NKK];
  float l2[2], dl[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int row = row0 + 16 * rb + r;
    load_fragments<T, NKK>(qf[rb], row_ptr<T>(a.q, a.sq, b, h, row), a.q, row < a.Nq, col, a.d_valid);
    load_fragments<T, NKK>(of[rb], row_ptr<T>(a.dout, a.sdo, b, h, row), a.dout, row < a.Nq, col, a.d_valid);
    const int64_t srow = ((int64_t)b * a.Hq + h) * a.NqP + row;
    l2[rb] = a.lse2[srow], dl[rb] = a.delta[srow];
  }
  f32x4 dq[2][NCB];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) dq[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int NT = (a.Nkv + kBwdKeysDq - 1) / kBwdKeysDq;
  int nt = NT;  // key tiles with a key some row of the tile sees
  if (a.causal) {
    const int64_t last = (int64_t)min(row0 + kBwdRows - 1, a.Nq - 1) + off;
    nt = last < 0 ? 0 : (int)min((int64_t)NT, last / kBwdKeysDq + 1);
  }
  const int put_at = r * RS + 16 * g, tr_at = (4 * g + (r >> 2)) * RS + 8 * (r & 3);

  v8 kf[2][NKK];
  auto fetch_k = [&](int t) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int key = t * kBwdKeysDq + 16 * kb + r;
      load_fragments<T, NKK>(kf[kb], row_ptr<T>(a.k, a.sk, b, hkv, key), a.k, key < a.Nkv, col, a.d_valid);
    }
  };
  if (nt > 0) fetch_k(0);
  for (int t = 0; t < nt; ++t) {
    const int k0 = t * kBwdKeysDq;
    // ---- the partial S^T and dP^T of this wave's columns: [key 4 g + i of the block][row r]; K goes into the image on the way
    f32x4 x[8];  // S^T (kb, rb) at 2 kb + rb, dP^T at 4 + 2 kb + rb
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      put_fragments<T, NKK>(kf[kb], kimg + put_at + 16 * kb * RS);
      v8 vf[NKK];
      const int key = k0 + 16 * kb + r;
      load_fragments<T, NKK>(vf, row_ptr<T>(a.v, a.sv, b, hkv, key), a.v, key < a.Nkv, col, a.d_valid);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
          s = E::mfma(kf[kb][kk], qf[rb][kk], s);
          dp = E::mfma(vf[kk], of[rb][kk], dp);
        }
        x[2 * kb + rb] = s, x[4 + 2 * kb + rb] = dp;
      }
    }
    if (t + 1 < nt) fetch_k(t + 1);
    exchange<8>(x, area, wave, lane);

    // ---- dS^T, rounded once: the B operand of row block rb holds keys 4 g + i of both key blocks
    v8 dsb[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const int row = row0 + 16 * rb + r;
      f32x4 ds[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = k0 + 16 * kb + 4 * g + i;
          const bool seen = (key < a.Nkv) & (key <= (a.causal ? row + off : a.Nkv));
          const float pe = __builtin_amdgcn_exp2f(seen ? __builtin_fmaf(x[2 * kb + rb][i], a.scale_log2, -l2[rb]) : -__builtin_inff());
          ds[kb][i] = pe * (x[4 + 2 * kb + rb][i] - dl[rb]);
        }
      dsb[rb] = pack<T>(ds[0], ds[1]);
    }

    // ---- dQ^T += K^T dS^T: this wave's columns
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const v8 kt = transposed<T>(kimg + tr_at, cb, RS);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) dq[rb][cb] = E::mfma(kt, dsb[rb], dq[rb][cb]);
    }
    __syncthreads();  // the exchange area is written again
  }

#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int row = row0 + 16 * rb + r;
    if (row < a.Nq) {
      T* const dqrow = const_cast<T*>(row_ptr<T>(a.dq, a.sdq, b, h, row));
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const int c = c0 + 16 * cb + 4 * g;
        if (c < a.d_valid) {
          t4 y;
#pragma unroll
          for (int i = 0; i < 4; ++i) y[i] = (T)(dq[rb][cb][i] * a.scale);
          *reinterpret_cast<t4*>(dqrow + c) = y;
        }
      }
    }
  }
}

}  // namespace bwd
#endif  // FFPA_BWD_KERNELS

}  // namespace ffpa
