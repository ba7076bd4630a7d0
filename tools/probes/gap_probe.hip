// gap_probe.hip — how many single-issue instructions does ONE wave per SIMD hide in the gap of its own v_mfma_f32_16x16x32_bf16 (16 cycles)?
//
// The prefill kernels run one wave per SIMD (the wave owns the SIMD's whole 512-entry register file), so nothing but the wave's own MFMAs can cover its
// softmax VALU work.  Round 4 measured "VALU between a wave's own 16-cycle MFMAs is paid in full" on a whole restructured kernel (profiles/
// r04_pipe1_nd1_negative.txt) — with packed FMAs, LDS scratch reads and DMA pieces in the same gaps.  This probe isolates the question: a loop of
// independent-accumulator MFMAs (the QK^T / PV pattern: a chain is revisited every 8th / 16th MFMA) with NF fillers of one kind behind every MFMA, one
// workgroup of four waves per CU on every CU (160 KiB of LDS requested: one workgroup per CU), random bf16 operands; s_memtime around the loop.
// Output: cycles per MFMA for every (kind, NF); the bare loop is the reference (16 cycles + issue).
//
//   hipcc --offload-arch=gfx950 -O2 tools/probes/gap_probe.hip -o tools/probes/bin/gap_probe && tools/probes/bin/gap_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
#include <vector>

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) float f32x2;

enum Kind { K_NONE = 0, K_FMA, K_EXP, K_PKFMA, K_ADD, K_CVT, K_MAX, K_DSREAD, K_MIX_SOFTMAX, K_SALU, K_EXP_FMA, K_DSTR, K_COUNT };
static const char* kNames[] = {"none", "v_fma_f32", "v_exp_f32", "v_pk_fma_f32", "v_add_f32", "v_cvt_pk_bf16_f32", "v_max_f32", "ds_read_b128", "softmax mix (fma,exp,add,cvt/2)",
                               "s_add_u32", "exp + fma alternating", "ds_read_b64_tr_b16"};

template <int KIND>
__device__ __forceinline__ void filler(int i, float (&f)[16], f32x2 (&g)[4], uint32_t (&u)[4], f32x4 (&lr)[4], const __attribute__((address_space(3))) char* lp, uint32_t& sreg) {
  if constexpr (KIND == K_FMA) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[i & 15]) : "v"(f[(i + 5) & 15]), "v"(f[(i + 9) & 15]));
  else if constexpr (KIND == K_EXP) asm volatile("v_exp_f32 %0, %1" : "=v"(f[i & 15]) : "v"(f[(i + 7) & 15]));
  else if constexpr (KIND == K_PKFMA) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(g[i & 3]) : "v"(g[(i + 1) & 3]), "v"(g[(i + 2) & 3]));
  else if constexpr (KIND == K_ADD) asm volatile("v_add_f32 %0, %0, %1" : "+v"(f[i & 15]) : "v"(f[(i + 5) & 15]));
  else if constexpr (KIND == K_CVT) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u[i & 3]) : "v"(f[(i + 3) & 15]), "v"(f[(i + 11) & 15]));
  else if constexpr (KIND == K_MAX) asm volatile("v_max_f32 %0, %0, %1" : "+v"(f[i & 15]) : "v"(f[(i + 5) & 15]));
  else if constexpr (KIND == K_DSREAD) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(lr[i & 3]) : "v"(lp), "n"(0));
  else if constexpr (KIND == K_DSTR) asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(g[i & 3]) : "v"(lp));
  else if constexpr (KIND == K_SALU) asm volatile("s_add_u32 %0, %0, 1" : "+s"(sreg) : : "scc");
  else if constexpr (KIND == K_MIX_SOFTMAX) {
    // per score: half an FMA (exponent argument), one exp, one add (row sum), half a cvt — issued round-robin
    switch (i % 6) {
      case 0: asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[i & 15]) : "v"(f[(i + 5) & 15]), "v"(f[(i + 9) & 15])); break;
      case 1: asm volatile("v_exp_f32 %0, %1" : "=v"(f[i & 15]) : "v"(f[(i + 7) & 15])); break;
      case 2: asm volatile("v_add_f32 %0, %0, %1" : "+v"(f[i & 15]) : "v"(f[(i + 5) & 15])); break;
      case 3: asm volatile("v_exp_f32 %0, %1" : "=v"(f[i & 15]) : "v"(f[(i + 7) & 15])); break;
      case 4: asm volatile("v_add_f32 %0, %0, %1" : "+v"(f[i & 15]) : "v"(f[(i + 5) & 15])); break;
      default: asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u[i & 3]) : "v"(f[(i + 3) & 15]), "v"(f[(i + 11) & 15])); break;
    }
  } else if constexpr (KIND == K_EXP_FMA) {
    if (i & 1) asm volatile("v_exp_f32 %0, %1" : "=v"(f[i & 15]) : "v"(f[(i + 7) & 15]));
    else asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[i & 15]) : "v"(f[(i + 5) & 15]), "v"(f[(i + 9) & 15]));
  }
}

// NACC independent accumulator chains, visited round-robin (QK^T at D = 512: 8 chains; PV: 64)
template <int KIND, int NF, int NACC, int SHARE>
__global__ __launch_bounds__(256) void probe(const uint32_t* __restrict__ src, float* __restrict__ sink, unsigned long long* __restrict__ cycles, int iters) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const uint32_t* p = src + (size_t)(blockIdx.x * 256 + tid) * 64;
  bf16x8 a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = *(const bf16x8*)(p + 4 * i);
    b[i] = *(const bf16x8*)(p + 16 + 4 * i);
  }
  float f[16];
  f32x2 g[4];
  uint32_t u[4] = {0, 0, 0, 0};
  f32x4 lr[4];
#pragma unroll
  for (int i = 0; i < 16; ++i) f[i] = __uint_as_float((p[32 + i] & 0x007fffffu) | 0x3f000000u);  // [0.5, 1)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    g[i] = f32x2{f[2 * i], f[2 * i + 1]};
    lr[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int i = tid; i < 4096; i += 256) ((__attribute__((address_space(3))) uint32_t*)smem)[i] = p[i & 63];
  __syncthreads();
  const __attribute__((address_space(3))) char* lp = (const __attribute__((address_space(3))) char*)smem + (tid & 63) * (KIND == K_DSTR ? 8 : 16);  // (conflict free either way)
  f32x4 acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint32_t sreg = 0;
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int m = 0; m < 2 * NACC; ++m) {
      // SHARE = 2: one A fragment feeds two MFMAs (the kernels' two 16-row halves)
      asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[m % NACC]) : "v"(a[(m / SHARE) & 3]), "v"(b[m & 3]));
#pragma unroll
      for (int k = 0; k < NF; ++k) filler<KIND>(m * NF + k, f, g, u, lr, lp, sreg);
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  asm volatile("s_nop 15\n\ts_nop 3");
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
#pragma unroll
  for (int i = 0; i < 16; ++i) s += f[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) s += g[i][0] + g[i][1] + __uint_as_float(u[i]) + lr[i][0] + lr[i][3];
  if (s == 1.2345f || sreg == 0xdeadbeefu) sink[blockIdx.x * 256 + tid] = s;
  if ((tid & 63) == 0) cycles[blockIdx.x * 4 + (tid >> 6)] = t1 - t0;
}

// ---- round 30: how the loops' OWN fragment reads are dealt between the two gaps of an MFMA PAIR (one fragment feeds the MFMAs of both row halves).
// The prefill loops request a fragment PF fragments ahead and wait for the oldest one in front of the pair's first MFMA; the probe issues the same
// instructions in the same places (the counted wait never blocks in steady state: the reads are far ahead), on a conflict-free LDS image.
//   PV forms  (two ds_read_b64_tr_b16 per pair):  P30 = {tr, tr, wait} | {}      P21 = {tr, wait} | {tr}
//   QK^T forms (one ds_read_b128 per pair):       Q10 = {b128, wait} | {}        Q01 = {wait} | {b128}
// PIECE > 0: every PIECE-th pair carries a 1 KiB LDS-DMA piece the way Mfma16::with_dma issues it — s_add_u32 m0 in front of the first MFMA, the
// buffer_load ... lds behind it.  PFORM says how THAT pair deals its reads: 0 = as the parent (every read in front), 1 = as the other pairs of the form
// (P21 / Q01: the read follows the piece in the second gap).  Every wave stages the first KiB of `src` into a KiB of its own behind the read image.
enum Form { F_BARE = 0, F_P30, F_P21, F_Q10, F_Q01, F_COUNT };
static const char* kFormNames[] = {"bare pairs", "{tr, tr, wait} | {}", "{tr, wait} | {tr}", "{b128, wait} | {}", "{wait} | {b128}"};

template <int N, typename F>
__device__ __forceinline__ void unrolled(F&& f) {
  if constexpr (N > 0) {
    unrolled<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}

// One `it` iteration is one KV step's loop: NP = 32 fragment pairs, the first PF fragments requested in front of it, the last PF pairs request nothing.  The reads are
// the compiler's own (builtins, fenced into their gap by sched_barrier, their counted waits placed by hipcc) exactly as in the kernels; their data are the MFMAs' A operands.
template <int FORM, int NACC, int PIECE, int PFORM>
__global__ __launch_bounds__(256) void pair_probe(const uint32_t* __restrict__ src, float* __restrict__ sink, unsigned long long* __restrict__ cycles, int iters) {
  typedef const __attribute__((address_space(3))) char* lds_ptr;
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  constexpr int NP = 32;
  constexpr bool kPv = FORM == F_P30 || FORM == F_P21, kQk = FORM == F_Q10 || FORM == F_Q01;
  constexpr int PF = kPv ? 4 : 6;  // (FFPA_M16_PF2 / FFPA_M16_PF1)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const uint32_t* p = src + (size_t)(blockIdx.x * 256 + tid) * 64;
  bf16x8 a0 = *(const bf16x8*)p, b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = *(const bf16x8*)(p + 16 + 4 * i);
  for (int i = tid; i < 4096; i += 256) ((__attribute__((address_space(3))) uint32_t*)smem)[i] = p[i & 63];  // the read image: the first 16 KiB
  __syncthreads();
  // fragment n of a step: PV = two transpose reads (8 B per lane, one contiguous 512 B row per wave each), QK^T = one 16 B read per lane (1 KiB per wave); n * 1 KiB < 16 KiB
  lds_ptr lp = (lds_ptr)smem + (tid & 63) * (kPv ? 8 : 16);
  asm volatile("" : "+v"(lp));
  // the DMA piece: 1 KiB per wave at LDS bytes [32 KiB + wave KiB, + 1 KiB) — inside the 160 KiB the launch requests, clear of the read image; source = the first
  // KiB of `src` (descriptor range 1 KiB, per-lane offset lane * 16 < 1 KiB)
  const uint32_t lds_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(uintptr_t)(lds_ptr)smem + 32768 + (tid >> 6) * 1024));
  const uint64_t sa = (uint64_t)src;
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  u32x4 rsrc = {(uint32_t)sa, (uint32_t)(sa >> 32) & 0xffffu, 1024u, 0x00020000u};
#pragma unroll
  for (int i = 0; i < 4; ++i) rsrc[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)rsrc[i]);
  const uint32_t voff = (tid & 63) * 16, soff = 0;
  f32x4 acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto half = [&](int n, int h) -> bf16x4 { return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(lp + (n % 16) * 1024 + h * 512)); };
  auto whole = [&](int n) -> bf16x8 { return *(const __attribute__((address_space(3))) bf16x8*)(lp + (n % 16) * 1024); };
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
    bf16x4 lo[NP], hi[NP];
    bf16x8 kf[NP];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < PF; ++n) {
      if constexpr (kPv) {
        lo[n] = half(n, 0);
        hi[n] = half(n, 1);
      } else if constexpr (kQk) {
        kf[n] = whole(n);
      }
    }
    unrolled<NP>([&](auto ic) {
      constexpr int m = decltype(ic)::value;
      constexpr bool piece = PIECE > 0 && m % (PIECE > 0 ? PIECE : 1) == 0;
      constexpr bool split = (FORM == F_P21 || FORM == F_Q01) && (!piece || PFORM == 1);
      constexpr bool req = m + PF < NP;
      __builtin_amdgcn_sched_barrier(0);
      // ---- gap 1
      if constexpr (kPv && req) {
        lo[m + PF] = half(m + PF, 0);
        if constexpr (!split) hi[m + PF] = half(m + PF, 1);
      }
      if constexpr (kQk && req && !split) kf[m + PF] = whole(m + PF);
      bf16x8 av = a0;
      if constexpr (kPv) av = __builtin_shufflevector(lo[m], hi[m], 0, 1, 2, 3, 4, 5, 6, 7);
      if constexpr (kQk) av = kf[m];
      if constexpr (piece)
        asm volatile("s_add_u32 m0, %3, 0\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0\n\tbuffer_load_dwordx4 %4, %5, %6 offen lds"
                     : "+v"(acc[(2 * m) % NACC]) : "v"(av), "v"(b[(2 * m) & 3]), "s"(lds_base), "v"(voff), "s"(rsrc), "s"(soff) : "memory", "scc", "m0");
      else
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[(2 * m) % NACC]) : "v"(av), "v"(b[(2 * m) & 3]));
      // ---- gap 2
      if constexpr (req && split) {
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (kPv) hi[m + PF] = half(m + PF, 1);
        else kf[m + PF] = whole(m + PF);
        __builtin_amdgcn_sched_barrier(0);
      }
      asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[(2 * m + 1) % NACC]) : "v"(av), "v"(b[(2 * m + 1) & 3]));
    });
    __builtin_amdgcn_sched_barrier(0);
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15\n\ts_nop 3" ::: "memory");
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  if (s == 1.2345f) sink[blockIdx.x * 256 + tid] = s;
  if ((tid & 63) == 0) cycles[blockIdx.x * 4 + (tid >> 6)] = t1 - t0;
}

template <int FORM, int NACC, int PIECE, int PFORM>
static double run_pairs(const uint32_t* src, float* sink, unsigned long long* cyc, int cus, double bare) {
  const int iters = 200;
  auto kern = pair_probe<FORM, NACC, PIECE, PFORM>;
  hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(kern, dim3(cus), dim3(256), 160 * 1024, 0, src, sink, cyc, iters);
  if (hipDeviceSynchronize() != hipSuccess) {
    printf("PAIR probe launch failed\n");
    exit(1);
  }
  std::vector<unsigned long long> h(cus * 4);
  hipMemcpy(h.data(), cyc, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost);
  double sum = 0;
  for (auto x : h) sum += (double)x;
  const double per = sum / h.size() / (iters * 32.0);
  printf("PAIR chains %2d  %-22s", NACC, kFormNames[FORM]);
  if (PIECE > 0) printf(" + a DMA piece on every %d-th pair, its reads %s", PIECE, (FORM == F_P21 || FORM == F_Q01) ? (PFORM ? "dealt alike (read behind the piece)" : "all in front (parent form)") : "all in front");
  printf(": %6.2f cycles per MFMA pair", per);
  if (bare > 0) printf("  (+ %5.2f over bare pairs)", per - bare);
  printf("\n");
  return per;
}

template <int KIND, int NF, int NACC>
static void run(const uint32_t* src, float* sink, unsigned long long* cyc, int cus, double bare) {
  const int iters = 200;
  auto kern = probe<KIND, NF, NACC, 2>;
  hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(kern, dim3(cus), dim3(256), 160 * 1024, 0, src, sink, cyc, iters);
  hipDeviceSynchronize();
  std::vector<unsigned long long> h(cus * 4);
  hipMemcpy(h.data(), cyc, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost);
  double sum = 0;
  for (auto x : h) sum += (double)x;
  const double per = sum / h.size() / (iters * 2.0 * NACC);
  printf("GAP  chains %2d  %-34s x %d per MFMA: %6.2f cycles per MFMA", NACC, kNames[KIND], NF, per);
  if (bare > 0) printf("  (+ %5.2f over the bare loop = %5.2f per filler)", per - bare, NF ? (per - bare) / NF : 0.0);
  printf("\n");
}

template <int KIND, int NACC>
static void sweep(const uint32_t* src, float* sink, unsigned long long* cyc, int cus, double bare) {
  run<KIND, 1, NACC>(src, sink, cyc, cus, bare);
  run<KIND, 2, NACC>(src, sink, cyc, cus, bare);
  run<KIND, 3, NACC>(src, sink, cyc, cus, bare);
  run<KIND, 4, NACC>(src, sink, cyc, cus, bare);
}

static double bare_of(const uint32_t* src, float* sink, unsigned long long* cyc, int cus, int nacc) {
  const int iters = 200;
  auto launch = [&](auto kern, int NACC) {
    hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(kern, dim3(cus), dim3(256), 160 * 1024, 0, src, sink, cyc, iters);
    hipDeviceSynchronize();
    std::vector<unsigned long long> h(cus * 4);
    hipMemcpy(h.data(), cyc, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost);
    double sum = 0;
    for (auto x : h) sum += (double)x;
    return sum / h.size() / (iters * 2.0 * NACC);
  };
  return nacc == 8 ? launch(probe<K_NONE, 0, 8, 2>, 8) : launch(probe<K_NONE, 0, 32, 2>, 32);
}

int main() {
  int cus = 256;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) == hipSuccess) cus = prop.multiProcessorCount;
  const size_t n = (size_t)cus * 256 * 64;
  std::vector<uint32_t> h(n);
  srand(1);
  for (auto& x : h) {
    // two random bf16 in [-2, 2): sign, exponent 126 .. 128, random mantissa
    auto one = []() { return (uint32_t)(((rand() & 1) << 15) | ((126 + rand() % 3) << 7) | (rand() & 0x7f)); };
    x = one() | (one() << 16);
  }
  uint32_t* src;
  float* sink;
  unsigned long long* cyc;
  hipMalloc(&src, n * 4);
  hipMalloc(&sink, (size_t)cus * 256 * 4);
  hipMalloc(&cyc, (size_t)cus * 4 * 8);
  hipMemcpy(src, h.data(), n * 4, hipMemcpyHostToDevice);
  printf("# gap_probe on %s (%d CUs): one workgroup of four waves per CU, v_mfma_f32_16x16x32_bf16 on random operands, NF fillers behind every MFMA\n", prop.gcnArchName, cus);
  const double bare8 = bare_of(src, sink, cyc, cus, 8);
  printf("GAP  chains  8  bare loop: %6.2f cycles per MFMA\n", bare8);
  sweep<K_FMA, 8>(src, sink, cyc, cus, bare8);
  sweep<K_ADD, 8>(src, sink, cyc, cus, bare8);
  sweep<K_MAX, 8>(src, sink, cyc, cus, bare8);
  sweep<K_EXP, 8>(src, sink, cyc, cus, bare8);
  sweep<K_PKFMA, 8>(src, sink, cyc, cus, bare8);
  sweep<K_CVT, 8>(src, sink, cyc, cus, bare8);
  sweep<K_MIX_SOFTMAX, 8>(src, sink, cyc, cus, bare8);
  sweep<K_EXP_FMA, 8>(src, sink, cyc, cus, bare8);
  sweep<K_SALU, 8>(src, sink, cyc, cus, bare8);
  run<K_DSREAD, 1, 8>(src, sink, cyc, cus, bare8);
  const double bare32 = bare_of(src, sink, cyc, cus, 32);
  printf("GAP  chains 32  bare loop: %6.2f cycles per MFMA\n", bare32);
  sweep<K_FMA, 32>(src, sink, cyc, cus, bare32);
  sweep<K_EXP, 32>(src, sink, cyc, cus, bare32);
  sweep<K_MIX_SOFTMAX, 32>(src, sink, cyc, cus, bare32);
  // round 30: the loops' own fragment reads, per MFMA and dealt over the two gaps of an MFMA pair (pair_probe)
  run<K_DSTR, 1, 8>(src, sink, cyc, cus, bare8);
  run<K_DSTR, 2, 8>(src, sink, cyc, cus, bare8);
  run<K_DSTR, 1, 32>(src, sink, cyc, cus, bare32);
  run<K_DSTR, 2, 32>(src, sink, cyc, cus, bare32);
  const double pair32 = run_pairs<F_BARE, 32, 0, 0>(src, sink, cyc, cus, 0);
  run_pairs<F_P30, 32, 0, 0>(src, sink, cyc, cus, pair32);
  run_pairs<F_P21, 32, 0, 0>(src, sink, cyc, cus, pair32);
  run_pairs<F_P30, 32, 8, 0>(src, sink, cyc, cus, pair32);  // (the PV loop at D = 512: a K piece on every 8th pair)
  run_pairs<F_P21, 32, 8, 0>(src, sink, cyc, cus, pair32);
  run_pairs<F_P21, 32, 8, 1>(src, sink, cyc, cus, pair32);
  const double pair16 = run_pairs<F_BARE, 16, 0, 0>(src, sink, cyc, cus, 0);
  run_pairs<F_Q10, 16, 0, 0>(src, sink, cyc, cus, pair16);
  run_pairs<F_Q01, 16, 0, 0>(src, sink, cyc, cus, pair16);
  run_pairs<F_Q10, 16, 4, 0>(src, sink, cyc, cus, pair16);  // (the QK^T loop at D = 512: a V piece on every 4th pair)
  run_pairs<F_Q01, 16, 4, 0>(src, sink, cyc, cus, pair16);
  run_pairs<F_Q01, 16, 4, 1>(src, sink, cyc, cus, pair16);
  return 0;
}
