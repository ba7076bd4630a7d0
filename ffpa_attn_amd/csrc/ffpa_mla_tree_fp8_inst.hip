// ffpa_mla_tree_fp8_inst.hip — TREE-MASK attention over an FP8 MLA latent cache: the verification step of tree speculative decoding over a pool of e4m3 codes
// under one per-tensor scale.  The tree variant of the latent kernel (ffpa_mla_variant.inc) over an e4m3 pool; the step's new rows are written by the FP8 latent
// call's quantising append in front of it.  Entry point: ffpa_attn_varlen_mla_tree_fp8_fwd (ffpa_capi.hip).
#define FFPA_MLA_STEM mla_tree_fp8
#define FFPA_MLA_TREE 1
#define FFPA_MLA_GATHER 0
#define FFPA_MLA_POOL FFPA_MLA_POOL_E4M3
#define FFPA_MLA_EXIT_REFRESH 1
#include "ffpa_mla_variant.inc"
