// ffpa_mla_sparse_wide_inst.hip — ffpa_mla_sparse_inst.hip for a WIDE pool: sparse (top-k indexed) attention over a 16-bit pool whose rows span more
// than 2^31 bytes per latent head.  The gather variant of the latent kernel (ffpa_mla_variant.inc) with 64-bit lane addresses, no descriptor and a zero row for
// the keys past a token's count (FFPA_MLA_GATHER 2).  Entry point: ffpa_attn_varlen_mla_sparse_wide_fwd (ffpa_capi.hip).
#define FFPA_MLA_STEM mla_sparse_wide
#define FFPA_MLA_TREE 0
#define FFPA_MLA_GATHER 2
#define FFPA_MLA_POOL FFPA_MLA_POOL_16BIT
#define FFPA_MLA_EXIT_REFRESH 0
#include "ffpa_mla_variant.inc"
