// ffpa_mla_gather64.h — what the WIDE-POOL builds of the sparse latent kernels (ffpa_mla_sparse*_wide_inst.hip; FFPA_M16_KV_GATHER64 of ffpa_fwd_m16_paged_body.inc)
// issue where the narrow builds issue a buffer load: the same pieces from a 64-bit GLOBAL address per lane, through no descriptor.  There is no range check and so
// no zero fill: a lane without a row is handed the address of the unit's zero row (ffpa_mla_variant.inc) by the gather.  A header of its own, seen by the three
// wide units alone.
#pragma once
#include "ffpa_fwd_m16_kernel.h"

namespace ffpa {

// A 1 KiB LDS-DMA piece from per-lane global addresses: global_load_lds_dwordx4 (gfx950 has the 16-byte form), destination M0 + lane * 16 as the buffer form's —
// M0 is written in the same statement, and the statement is as invisible to the compiler's vmcnt scoreboard as lds_dma_16_at (ffpa_common.h says why).  `rsrc` and
// `soff` are the buffer form's arguments, kept so that the tile text calls both forms with one line; they are not read.
template <bool NT>
struct LdsDma16G64 {
  template <int LCONST>
  static __device__ __forceinline__ void at(u32x4, uint32_t lds_base, uint64_t addr, uint32_t) {
    if constexpr (NT)
      asm volatile("s_add_u32 m0, %0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt" : : "s"(lds_base), "v"(addr), "n"(LCONST) : "memory", "scc" FFPA_M0_CLOBBER);
    else
      asm volatile("s_add_u32 m0, %0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(lds_base), "v"(addr), "n"(LCONST) : "memory", "scc" FFPA_M0_CLOBBER);
  }
};

// Mfma16 / Mfma16Nt with that piece riding on the MFMA (the MFMA is the wait state between the M0 write and the piece: Mfma16::with_dma).
template <typename T, bool NT>
struct Mfma16G64;
#define FFPA_MFMA16_G64(TYPE, SUFFIX, NT_, HINT)                                                                                                    \
  template <>                                                                                                                                       \
  struct Mfma16G64<TYPE, NT_> : Mfma16<TYPE> {                                                                                                      \
    typedef Elem<TYPE>::v8 v8;                                                                                                                      \
    template <int KIND, int LCONST>                                                                                                                 \
    static __device__ __forceinline__ void with_dma(f32x4& d, v8 a, v8 b, u32x4, uint32_t lds_base, uint64_t addr, uint32_t) {                     \
      if constexpr (KIND == 0)                                                                                                                      \
        asm volatile("s_add_u32 m0, %3, %5\n\tv_mfma_f32_16x16x32_" SUFFIX " %0, %1, %2, 0\n\tglobal_load_lds_dwordx4 %4, off" HINT                 \
                     : "=&v"(d) : "v"(a), "v"(b), "s"(lds_base), "v"(addr), "n"(LCONST) : "memory", "scc" FFPA_M0_CLOBBER);                          \
      else if constexpr (KIND == 1)                                                                                                                 \
        asm volatile("s_add_u32 m0, %3, %5\n\tv_mfma_f32_16x16x32_" SUFFIX " %0, %1, %2, %0\n\tglobal_load_lds_dwordx4 %4, off" HINT                \
                     : "+v"(d) : "v"(a), "v"(b), "s"(lds_base), "v"(addr), "n"(LCONST) : "memory", "scc" FFPA_M0_CLOBBER);                           \
      else                                                                                                                                          \
        asm volatile("s_add_u32 m0, %3, %5\n\tv_mfma_f32_16x16x32_" SUFFIX " %0, %1, %2, %0\n\tglobal_load_lds_dwordx4 %4, off" HINT                \
                     : "+a"(d) : "v"(a), "v"(b), "s"(lds_base), "v"(addr), "n"(LCONST) : "memory", "scc" FFPA_M0_CLOBBER);                           \
    }                                                                                                                                               \
  };
FFPA_MFMA16_G64(__bf16, "bf16", false, "")
FFPA_MFMA16_G64(__bf16, "bf16", true, " nt")
FFPA_MFMA16_G64(_Float16, "f16", false, "")
FFPA_MFMA16_G64(_Float16, "f16", true, " nt")
#undef FFPA_MFMA16_G64

// The register loads of the pools the kernel stages in VGPRs (e4m3 codes: 8 bytes; a 656-byte row: 16 bytes at the slot and the dword of its scale), from a global
// address.  The compiler's own loads, as the buffer forms they replace: it counts vmcnt for them and waits in front of the first use.  A NoPE slot of a 656-byte
// row lies at a multiple of 8, so the 16-byte load promises no more than that.  NT: the non-temporal hint.
template <typename V, bool NT>
__device__ __forceinline__ V global_load_at(uint64_t addr) {
  typedef V __attribute__((aligned(sizeof(V) < 8 ? sizeof(V) : 8))) LooseV;
  const auto* p = (const __attribute__((address_space(1))) LooseV*)addr;
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

}  // namespace ffpa
