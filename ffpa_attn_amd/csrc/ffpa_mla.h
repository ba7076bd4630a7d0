// ffpa_mla.h — MLA latent-cache attention (the ffpa_attn_varlen_mla*_fwd calls, ffpa_capi.hip): THE LIST OF ITS KERNEL VARIANTS, what the kernels take beyond
// FwdArgs / VarlenArgs / PagedArgs, the launchers of the seven ffpa_mla*_inst.hip units (one shell: ffpa_mla_variant.inc) and the 16-bit appends.  A header of its
// own so that the dense, packed and paged objects see nothing of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ffpa {
struct FwdArgs;
struct VarlenArgs;
struct PagedArgs;

// The (head dim, value width) pairs every variant is built for: one line per pair here, one entry of MLA_BUILDS in build.py.
#define FFPA_FOR_EACH_MLA_BUILD(X) X(576, 512)

// THE VARIANTS.  A latent kernel is three independent choices — is there a tree mask, how are the keys found, what does the pool hold — and one switch that was
// found by measurement.  One row per variant, in link order (build.py's MLA_VARIANTS names the same stems in the same order); the row's stem names the unit
// (ffpa_<stem>_inst.hip), the kernel (ffpa_fwd_m16_<stem>_kernel) and the launchers (launch_<stem>_d<D>).  X(stem, tree, gather, pool, exit refresh, ...):
//   tree          the element test of the tiles that hold a draft key reads the row's 64-bit mask word (and the wait in front of the KV loop: ffpa_mla_variant.inc)
//   gather        0: the keys of a sequence are found through its page table; 1: through a list of pool rows per query token (the sparse calls)
//   pool          what a latent row is made of (FFPA_MLA_POOL_*)
//   exit refresh  the epilogue's arguments are read again from the argument block behind the KV loop (ffpa_mla_variant.inc says why): on where the loop has no
//                 scalar register to spare — measured per variant, not derived from the other three
#define FFPA_MLA_POOL_16BIT 0  // bf16 / fp16 elements, q's dtype
#define FFPA_MLA_POOL_E4M3 1   // OCP e4m3 codes under ONE per-tensor scale (MlaFp8Args::kv_scale)
#define FFPA_MLA_POOL_DS 2     // the 656-byte rows of DeepSeek-V3.2 (ffpa_mla_sparse_ds.h): e4m3 codes, a scale per 128 columns in the row, bf16 rotary columns; q is bf16
#define FFPA_FOR_EACH_MLA_VARIANT(X, ...)                      \
  X(mla, 0, 0, FFPA_MLA_POOL_16BIT, 0, __VA_ARGS__)            \
  X(mla_sparse, 0, 1, FFPA_MLA_POOL_16BIT, 0, __VA_ARGS__)     \
  X(mla_tree, 1, 0, FFPA_MLA_POOL_16BIT, 1, __VA_ARGS__)       \
  X(mla_fp8, 0, 0, FFPA_MLA_POOL_E4M3, 0, __VA_ARGS__)         \
  X(mla_sparse_fp8, 0, 1, FFPA_MLA_POOL_E4M3, 1, __VA_ARGS__)  \
  X(mla_tree_fp8, 1, 0, FFPA_MLA_POOL_E4M3, 1, __VA_ARGS__)    \
  X(mla_sparse_ds, 0, 1, FFPA_MLA_POOL_DS, 1, __VA_ARGS__)

struct MlaVariant {
  const char* stem;
  bool tree, gather;
  int pool;
  bool exit_refresh;
};
#define FFPA_ROW(stem, tree, gather, pool, refresh, ...) {#stem, tree != 0, gather != 0, pool, refresh != 0},
constexpr MlaVariant kMlaVariants[] = {FFPA_FOR_EACH_MLA_VARIANT(FFPA_ROW, )};
#undef FFPA_ROW
#define FFPA_ROW(stem, ...) kMlaVariant_##stem,
enum MlaVariantId { FFPA_FOR_EACH_MLA_VARIANT(FFPA_ROW, ) kMlaVariantCount };
#undef FFPA_ROW

// What the latent kernels need beyond the three shared structs (they keep their layout): the keys of a KV head are the latent rows' D columns, its values the
// first `dv` of the same rows — only O columns < dv are stored.
struct MlaArgs {
  int dv;
};

// The latent append: row i of sequence b of kv_new goes to cache position max(seqlens[b], 0) + i (dropped at or past cap), ONE store per element, and
// used[b] = min(max(seqlens[b], 0) + Snew, cap) is what the attention launch behind it reads as the sequence's length.
struct MlaAppendArgs {
  const void* kv_new;   // [B, Snew, Hkv, D] by s_new = {batch, row, head}
  void* cache;          // the pool
  const int* seqlens;   // [B] lengths before the step
  int* used;            // [B] lengths after it
  const int* table;     // [B][bt_stride] page ids (clamped to the pool)
  int64_t s_new[3];
  int64_t s_row, s_head, s_page;  // elements between two rows / heads / pages of the pool
  int64_t bt_stride;
  int B, Snew, Hkv, D, cap, page_size, num_pages;
};

// The latent append of a RAGGED step (ffpa_attn_mla_append_varlen): kv_new is token rows [T, Hkv, D] packed by cu_q (a.s_new = {unused, row, head}; a.Snew is not
// read), row t is token i = t - cu_q[b] of its sequence b and goes to cache position max(seqlens[b], 0) + i; used[b] = min(max(seqlens[b], 0) + (cu_q[b + 1] -
// cu_q[b]), cap) for every b < B.
struct MlaAppendVarlenArgs {
  MlaAppendArgs a;
  const int* cu_q;  // [B + 1]
  int T;            // token rows of kv_new (>= cu_q[B]: the rest is padding)
};

// THE PLACEMENT RULE of the latent appends — the four kernels of ffpa_mla_inst.hip and ffpa_mla_fp8_inst.hip, which differ in how a workgroup finds its (b, i) and in
// how it writes the row.  Everything here is read through wave-uniform indices: a scalar load as long as it stands in front of the kernel's first store, so every
// kernel calls mla_append_place BEFORE it stores used[].
//   The id of the page that holds cache position `pos` of sequence b, clamped to the pool.
__device__ __forceinline__ int mla_append_page(const MlaAppendArgs& a, int b, int64_t pos) {
  int page = a.table[(int64_t)b * a.bt_stride + pos / a.page_size];
  page = page > 0 ? page : 0;
  return page < a.num_pages - 1 ? page : a.num_pages - 1;
}

//   Where new row i of sequence b goes: cache position max(len, 0) + i (a negative length acts as 0, as in the attention kernels); `keep` is false — and the table
//   is not read — for a position at or past the capacity and for a row the step does not have (`valid` false; i may be negative then, never a negative cache row).
//   pos < cap means pos / page_size < pages_per_row: the table's row is not left.
struct MlaAppendPlace {
  bool keep;
  int page, row;
};
__device__ __forceinline__ MlaAppendPlace mla_append_place(const MlaAppendArgs& a, int b, int i, int len, bool valid) {
  const int64_t pos = (int64_t)(len > 0 ? len : 0) + i;
  MlaAppendPlace at = {valid && pos < a.cap, 0, 0};
  if (at.keep) {
    at.page = mla_append_page(a, b, pos);
    at.row = (int)(pos % a.page_size);
  }
  return at;
}

//   used[b] of a sequence of length `len` that brings n new rows (n = 0 included: every sequence gets one).
__device__ __forceinline__ int mla_append_used(const MlaAppendArgs& a, int len, int n) {
  const int64_t u = (int64_t)(len > 0 ? len : 0) + n;
  return (int)(u < a.cap ? u : a.cap);
}

// ONE host signature for every variant's launcher: the fourth struct is the e4m3 builds' (ffpa_mla_fp8.h: the value width and the scale); the kernels over the
// other pools still take MlaArgs by value — their launcher passes on the value width alone.  -4: a dtype the variant is not built for.
struct MlaFp8Args;
typedef int (*mla_launch_fn)(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaFp8Args& ma, hipStream_t stream);
#define FFPA_DECL_ONE(stem, tree, gather, pool, refresh, D) \
  int launch_##stem##_d##D(int dtype, int nt, const FwdArgs& a, const VarlenArgs& va, const PagedArgs& pa, const MlaFp8Args& ma, hipStream_t stream);
#define FFPA_DECL(D, DV) FFPA_FOR_EACH_MLA_VARIANT(FFPA_DECL_ONE, D)
FFPA_FOR_EACH_MLA_BUILD(FFPA_DECL)
#undef FFPA_DECL
#undef FFPA_DECL_ONE
int launch_mla_append(const MlaAppendArgs& a, hipStream_t stream);
int launch_mla_append_varlen(const MlaAppendVarlenArgs& va, hipStream_t stream);

}  // namespace ffpa
