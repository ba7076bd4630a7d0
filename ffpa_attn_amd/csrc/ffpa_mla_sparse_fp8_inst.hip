// ffpa_mla_sparse_fp8_inst.hip — SPARSE (top-k indexed) attention over an FP8 MLA latent pool (e4m3 codes, one per-tensor scale): DeepSeek-V3.2's top-k attention
// as an engine with kv_cache_dtype = "fp8" issues it.  The gather variant of the latent kernel (ffpa_mla_variant.inc) over an e4m3 pool.  Entry point:
// ffpa_attn_varlen_mla_sparse_fp8_fwd (ffpa_capi.hip).
#define FFPA_MLA_STEM mla_sparse_fp8
#define FFPA_MLA_TREE 0
#define FFPA_MLA_GATHER 1
#define FFPA_MLA_POOL FFPA_MLA_POOL_E4M3
#define FFPA_MLA_EXIT_REFRESH 1
#include "ffpa_mla_variant.inc"
