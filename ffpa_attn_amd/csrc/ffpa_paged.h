// ffpa_paged.h — the paged-KV twin of the packed-sequence kernel: its arguments and the per-head-dim launchers (ffpa_paged_inst.hip, one object per D) the
// C-ABI dispatches through (ffpa_attn_varlen_paged_fwd, ffpa_capi.hip).  A header of its own so that the dense and packed objects see nothing of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ffpa_common.h"
#include "ffpa_launch.h"

namespace ffpa {
struct FwdArgs;
struct VarlenArgs;

// Where a sequence's keys live (include/ffpa_attn.h: ffpa_paged_kv): key j of sequence i is row j % page_size of page table[i * bt_stride + j / page_size];
// page p of K starts p * k_page_stride elements past FwdArgs::k (V likewise), rows and heads inside a page have FwdArgs' row / head strides.
struct PagedArgs {
  const int* table;        // [batch][bt_stride] page ids
  int64_t bt_stride;       // entries between two sequences' rows
  int64_t k_page_stride;   // elements between two pages of K
  int64_t v_page_stride;   // ... of V
  int cap;                 // keys a sequence can hold: pages_per_row * page_size (Nkv_i = min(seqused_k[i], cap))
  int page_size;           // keys per page: a multiple of the kernel's tile (64)
  int tiles_per_page;      // page_size / block keys
  int num_pages;           // pages in the pool: ids are clamped to [0, num_pages)
};

// tile_src (ffpa_common.h) for a tile whose first row is `tile_base` (its page's row): the same row count and span — rows past the sequence's last key read as
// zeros, a tile at or past the end moves no bytes.  What FFPA_M16_KV_SRC of ffpa_fwd_m16_paged_body.inc calls: the paged kernel and the latent kernels built on it.
template <int BC>
__device__ __forceinline__ TileSrc tile_src_at(const char* tile_base, uint32_t row_bytes, int key0, int nkv, uint32_t RB) {
  const int kc = key0 < nkv ? key0 : nkv;
  int rows = nkv - kc;
  rows = rows < BC ? rows : BC;
  const uint32_t span = (uint32_t)(rows < 1 ? rows : 1) * ((uint32_t)(rows - 1) * row_bytes + (uint32_t)RB);
  TileSrc t;
  t.base = tile_base;
  t.rows = rows;
  t.rsrc = make_rsrc(t.base, span);
  return t;
}

#define FFPA_DECL(D) int launch_paged_d##D(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, hipStream_t stream);
FFPA_FOR_EACH_VARLEN_HEAD_DIM(FFPA_DECL)
#undef FFPA_DECL

}  // namespace ffpa
