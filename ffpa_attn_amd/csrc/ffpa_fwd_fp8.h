// ffpa_fwd_fp8.h — the FP8 (OCP e4m3) attention forward for head dims 256 ... 512 (ffpa_attn_fp8_quantize and ffpa_attn_fp8_fwd, ffpa_capi.hip): the scratch
// layout both sides of it agree on, the arguments of the pre-pass and of the attention kernel, and their launchers (ffpa_fwd_fp8_quant.hip, ffpa_fwd_fp8_inst.hip).
// A header of its own: no other kernel object sees it.
//
// THE SCRATCH LAYOUT.  Every operand of v_mfma_f32_16x16x128_f8f6f4 is a FRAGMENT of 2 KiB: 16 rows x 128 contraction positions, stored as two planes of 1 KiB —
// plane h in {0, 1} holds, for lane l = 16 g + r (r = row, g = lane group), the 16 bytes of positions 32 g + 16 h + [0, 16) at byte 16 l.  A lane's operand is
// one 16-byte read from each plane at 16 * lane: every read and every copy of a fragment is contiguous over the wave.  (The instruction contracts over all 128
// positions at once: which position a lane's byte stands for is free as long as A and B agree, and here both are written by the same rule.)
//   Q8   [B, Hq, row tiles]   a tile = kFp8BlockRows / 16 row blocks x NC column chunks of 128 (NC = ceil(D / 128); columns at and past D are zero codes):
//        fragment (row block rb, chunk c), row 16 rb + r, position p = column 128 c + p.  Rows at and past Nq are zero codes.
//   K8   [B, Hkv, key tiles]  a tile = 8 key blocks x NC chunks: fragment (kb, c), row = key 16 kb + r of the tile, position p = column 128 c + p.  Keys at and
//        past Nkv are zero codes.
//   V8T  [B, Hkv, key tiles]  a tile = D / 16 fragments: fragment db, row = channel 16 db + r, position p = the tile's key  16 ((p % 32) / 4) + 4 (p / 32) + p % 4
//        — the key whose probability the score MFMAs leave in byte p % 4 of accumulator (p % 32) / 4 of lane group p / 32 (see ffpa_fwd_fp8_inst.hip).
//   q_scale [B, Hq, row tiles], k_scale [B, Hkv, key tiles], v_scale [B, Hkv, D]: float32 powers of two.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ffpa {

constexpr int kFp8BlockKeys = 128;   // keys of a K8 / V8T tile: the PV MFMA's whole contraction
constexpr int kFp8BlockRows = 64;    // query rows of a Q8 tile = of a workgroup: 4 waves x 1 row block of 16
constexpr int kFp8PShift = 8;        // P is multiplied by 2^8 in front of its conversion to e4m3 (p <= 1: 256 < 448)

constexpr int fp8_padded_dim(int d) { return (d + 127) / 128 * 128; }

// the pre-pass: three launches on one stream (partial statistics per key tile; the K mean and the V scale; the codes)
struct Fp8QuantArgs {
  const void *q, *k, *v;                 // 16-bit, last dim contiguous
  uint8_t *q8, *k8, *v8t;                // the scratch above
  float *q_scale, *k_scale, *v_scale;
  float *ksum_part, *vamax_part;         // [B, Hkv, key tiles, D] each
  float *kmean;                          // [B, Hkv, D]
  int64_t s_q[3], s_k[3], s_v[3];        // elements: {batch, head, row}
  int B, Hq, Hkv, Nq, Nkv, D, fp16, smooth_k;
  float q_premul;                        // float32(scale * log2(e))
};

int launch_fwd_fp8_quantize(const Fp8QuantArgs& a, hipStream_t stream);

struct Fp8FwdArgs {
  const uint8_t *q8, *k8, *v8t;
  const float *q_scale, *k_scale, *v_scale;
  void* o;                               // [B, Hq, Nq, D] 16-bit by s_o = {batch, head, row}; last dim contiguous, rows 8-byte aligned
  int64_t s_o[3];
  int B, Hq, Hkv, Nq, Nkv, fp16, causal;
};

// one per head dim (ffpa_fwd_fp8_inst.hip, -DFFPA_INST_D): 0, or launch_kernel's error
#define FFPA_FP8_DECLARE(d) int launch_fwd_fp8_d##d(const Fp8FwdArgs& a, hipStream_t stream);
FFPA_FP8_DECLARE(256)
FFPA_FP8_DECLARE(320)
FFPA_FP8_DECLARE(384)
FFPA_FP8_DECLARE(448)
FFPA_FP8_DECLARE(512)
#undef FFPA_FP8_DECLARE

}  // namespace ffpa
