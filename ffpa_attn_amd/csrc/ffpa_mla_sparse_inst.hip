// ffpa_mla_sparse_inst.hip — SPARSE (top-k indexed) attention over the MLA latent cache (DeepSeek-V3.2's "DeepSeek Sparse Attention" in its absorbed decode form,
// FlashMLA's sparse decode call): every query token brings its own list of latent rows — slots of the pool, shared by all heads of the token — and attends to
// those rows only.  The gather variant of the latent kernel (ffpa_mla_variant.inc) over a 16-bit pool.  Entry point: ffpa_attn_varlen_mla_sparse_fwd (ffpa_capi.hip).
#define FFPA_MLA_STEM mla_sparse
#define FFPA_MLA_TREE 0
#define FFPA_MLA_GATHER 1
#define FFPA_MLA_POOL FFPA_MLA_POOL_16BIT
#define FFPA_MLA_EXIT_REFRESH 0
#include "ffpa_mla_variant.inc"
