// ffpa_mla_sparse_ds_inst.hip — SPARSE (top-k indexed) attention over the 656-byte FP8 latent rows of DeepSeek-V3.2 (ffpa_mla_sparse_ds.h: 512 e4m3 codes, four
// float32 scales — one per 128 columns —, 64 bf16 rotary columns), the row format in which the engines that serve that model keep its cache.  The gather variant
// of the latent kernel (ffpa_mla_variant.inc) over such rows: bf16 ONLY, (576, 512) only.  Entry point: ffpa_attn_varlen_mla_sparse_ds_fwd (ffpa_capi.hip).
#define FFPA_MLA_STEM mla_sparse_ds
#define FFPA_MLA_TREE 0
#define FFPA_MLA_GATHER 1
#define FFPA_MLA_POOL FFPA_MLA_POOL_DS
#define FFPA_MLA_EXIT_REFRESH 1
#include "ffpa_mla_variant.inc"
