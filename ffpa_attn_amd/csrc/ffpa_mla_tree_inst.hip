// ffpa_mla_tree_inst.hip — TREE-MASK attention over the MLA latent cache: the verification step of tree speculative decoding (an MTP head driven as an EAGLE draft
// model) for the models whose cache is one latent pool.  The Sq draft nodes of a sequence are the last rows of its latent cache; node i sees the whole prefix and,
// among the draft rows, what its 64-bit mask word says.  The tree variant of the latent kernel (ffpa_mla_variant.inc) over a 16-bit pool.  Entry point:
// ffpa_attn_varlen_mla_tree_fwd (ffpa_capi.hip).
#define FFPA_MLA_STEM mla_tree
#define FFPA_MLA_TREE 1
#define FFPA_MLA_GATHER 0
#define FFPA_MLA_POOL FFPA_MLA_POOL_16BIT
#define FFPA_MLA_EXIT_REFRESH 1
#include "ffpa_mla_variant.inc"
