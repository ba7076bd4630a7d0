/*
 * ffpa_attn.h — C-ABI of the MI355X (gfx950) fused attention forward.
 *
 * This is the drop-in boundary for the ONE hot path this repo accelerates:
 * the large-headdim Split-D attention forward that the reference reaches via
 *
 *   torch.ops.ffpa_attn._fwd_cuda            (src/ffpa_attn/cuda/__init__.py:57-139)
 *     -> ffpa_attn._C.ffpa_attn_forward      (csrc/cuffpa/ffpa_api.cc:86-239, pybind :265-306)
 *       -> launch_ffpa_attn_fwd_template     (csrc/cuffpa/launch.cuh:61-606)
 *         -> split_d_fwd_sm80 & friends      (csrc/cuffpa/native/sm_80/split_d.cuh:96-777)
 *
 * Every entry point is extern "C", takes plain pointers / sizes / strides and
 * a hipStream_t passed as void*.  No torch types, no allocation, no device
 * synchronisation, no global mutable state beyond write-once per-device caches (CU count, arch check,
 * kernel attributes; std::atomic): the caller owns every buffer and
 * picks the stream.  Each function cites the reference interface it replaces.
 */
#ifndef FFPA_ATTN_H_
#define FFPA_ATTN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFPA_ATTN_ABI_VERSION 7 /* 5: + the packed-sequence entry points (ffpa_attn_varlen_fwd ...); 6: + KV splits inside the packed call (its workspace fields, ffpa_attn_varlen_fwd_workspace_bytes, plan out[4]); 7: + the paged-KV call (ffpa_paged_kv, ffpa_attn_varlen_paged_fwd ...), + the KV-cache append (ffpa_kv_append_params, ffpa_attn_kvcache_append: its own size-checked struct, no existing layout changed), + the merge of two attention states (ffpa_merge_states_params, ffpa_attn_merge_states: likewise) */

/* status codes (0 == success).  The Python host maps them onto the exception
 * classes the reference raises (TORCH_CHECK -> RuntimeError,
 * std::invalid_argument -> ValueError; ffpa_api.cc:193-197, env.py:750-752). */
enum ffpa_status {
  FFPA_OK = 0,
  FFPA_ERR_NULL_POINTER = 1,      /* q/k/v/o missing                                   */
  FFPA_ERR_BAD_DTYPE = 2,         /* dtype not bf16/fp16, or bias dtype unknown         */
  FFPA_ERR_BAD_HEADDIM = 3,       /* "headdim not support!" (env.py:750-752)            */
  FFPA_ERR_BAD_SHAPE = 4,         /* non-positive dims, Hq % Hkv != 0                   */
  FFPA_ERR_BAD_STRIDE = 5,        /* stride not a multiple of 8 elements / too large    */
  FFPA_ERR_MISALIGNED = 6,        /* base pointer not 16-byte aligned                   */
  FFPA_ERR_UNSUPPORTED = 7,       /* feature not built (e.g. dropout)                   */
  FFPA_ERR_LAUNCH = 8,            /* hipGetLastError() after the launch                 */
  FFPA_ERR_NO_DEVICE = 9,         /* no current device, or it is not a gfx950           */
  FFPA_ERR_BAD_ABI = 10           /* struct_size / abi_version mismatch                 */
};

enum ffpa_dtype { FFPA_DTYPE_BF16 = 0, FFPA_DTYPE_FP16 = 1 };

/* attn_bias element type.  Same codes as the reference's native launcher
 * (csrc/cuffpa/native/launch.cuh:279-281): 0 none, 1 fp16, 2 bf16, 3 fp32 — plus 4: a boolean mask, one byte per
 * score, non-zero = the key is visible, zero = score -inf.  The reference's host materialises that as a 0 / -inf
 * tensor in q's dtype before every launch (src/ffpa_attn/functional.py:891-898); here the kernel reads the caller's
 * bytes (torch.bool storage) directly: same scores, no mask-sized temporary, 1 byte per element of mask traffic. */
enum ffpa_bias_dtype {
  FFPA_BIAS_NONE = 0,
  FFPA_BIAS_FP16 = 1,
  FFPA_BIAS_BF16 = 2,
  FFPA_BIAS_FP32 = 3,
  FFPA_BIAS_BOOL8 = 4
};

/* ffpa_fwd_params.flags */
#define FFPA_FLAG_DEBUG_SAFE_PATH 0x1u /* test-only: register-staged K/V + scalar V gather  */
#define FFPA_FLAG_NO_XCD_REMAP    0x2u /* bench-only: dispatch-order block mapping          */
/* (0x4u: retired — it belonged to the persistent-workgroup experiment, tools/experiments/r05_pruned_switches.diff) */
#define FFPA_FLAG_NO_BIAS_LDS     0x8u /* bench-only: read a key bias from global memory in every tile   */
#define FFPA_FLAG_L2_PREFETCH     0x10u /* bench-only: touch the K/V tile two steps ahead in every prefill launch (default: the launch side decides) */
#define FFPA_FLAG_NO_L2_PREFETCH  0x20u /* bench-only: never                                           */
#define FFPA_FLAG_FORCE_SPLITS    0x40u /* bench-only: honour num_splits > 1 for a prefill launch that fills the chip too (default: only under-filled launches split) */
#define FFPA_FLAG_KV_STREAM       0x80u /* bench-only: short-query launches fetch K / V with the non-temporal hint (default: the launch side decides — one reader per byte and K + V larger than the Infinity Cache) */
#define FFPA_FLAG_NO_KV_STREAM    0x800u /* bench-only: never                                          */
#define FFPA_FLAG_WIDE_TILE       0x1000u /* bench / test: prefill launches take the wide-row tile (ffpa_fwd_m16w_kernel) wherever the head dim and the mask kind have one (default: the launch side decides) */
#define FFPA_FLAG_NO_WIDE_TILE    0x2000u /* bench / test: never                                       */
#define FFPA_FLAG_PAIR_TILES      0x8000u /* bench / test: causal prefill launches pair row tiles i and n - 1 - i in one workgroup wherever the build can (default: the launch side decides) */
#define FFPA_FLAG_NO_PAIR_TILES   0x20000u /* bench / test: never                                      */
#define FFPA_FLAG_DETERMINISTIC   0x4000u /* batch-invariant bits: the plan of a (batch, head) slice does not depend on how many slices share the launch — prefill
                                             launches never split the KV axis and never take the wide-row tile (128-row tiles, one pass per row), short-query launches
                                             split by the KV length alone (a fixed number of KV tiles per range).  Costs what the launch-size rules would have gained
                                             (under-filled / ragged-round prefill launches: up to ~ 20 %).  Python: FFPA_HIP_DETERMINISTIC=1 sets it on every call. */
#define FFPA_FLAG_NO_HEAD_CHUNKS   0x80000u /* bench / test, ffpa_attn_fwd: causal GQA prefill launches keep the (batch, head, row tile) workgroup order (default: the launch side takes the head-chunk order — the same row tile of a KV group's heads at the same time — where its rule applies; same bits either way) */
#define FFPA_FLAG_TILE_RANGES      0x100000u /* bench / test, ffpa_attn_fwd: with FFPA_FLAG_FORCE_SPLITS and num_splits = n, a causal prefill launch splits every row tile's OWN visible KV tiles into n ranges (the packed-sequence kernel's dense mode) instead of n uniform ranges (default: the launch side takes two such ranges for causal launches of one round of workgroups) */
#define FFPA_FLAG_NO_TILE_RANGES   0x200000u /* bench / test, ffpa_attn_fwd: never */
#define FFPA_FLAG_NO_COMPACT_GRID   0x400000u /* bench / test, ffpa_attn_varlen_fwd: a ragged prefill batch keeps the grid of batch x ceil(max_seqlen_q / block rows) row tiles per head (default: callers that say total_q get ceil(total_q / block rows) + batch slots per head when three quarters of the full grid would be idle; same order, same bits) */
#define FFPA_FLAG_NO_PACK_GQA      0x40000u /* bench / test, ffpa_attn_varlen_fwd: short query sequences under GQA (group x max_seqlen_q rows fit one tile: decode, speculative decoding) keep one workgroup per QUERY head (default: the heads of a KV group x the tokens are packed into the rows of one tile) */
#define FFPA_FLAG_XCD_GROUP(log2p1) ((unsigned)(log2p1) << 8) /* bench-only: bits 8..10 = 1 + log2 of the XCDs that share a head's row tiles (1 -> 1, 2 -> 2, 3 -> 4, 4 -> 8); 0 = the launch side decides */

/*
 * One forward call.  Layout contract (replaces the dense-[B,H,N,D] assumption of
 * split_d.cuh:137-142): element strides for the batch / head / sequence dims,
 * headdim stride 1, every row 16-byte aligned (D % 8 == 0, strides % 8 == 0).
 *
 *   q  [B, Hq,  Nq,  D]     k, v [B, Hkv, Nkv, D]     o [B, Hq, Nq, D]
 *   lse  [B, Hq, Nq] fp32 contiguous, natural log, may be NULL (cuda/__init__.py:102-112)
 *   bias [B|1, Hq|1, Nq|1, Nkv|1] additive (fp16 / bf16 / fp32) or boolean (FFPA_BIAS_BOOL8), stride 0 on
 *        broadcast dims (native/launch.cuh:277-290); NULL <=> bias_dtype == FFPA_BIAS_NONE.
 *
 * Score = scale * q.k + bias ; masked iff (causal && key > row + causal_offset)
 * or key >= Nkv or (boolean mask && mask byte == 0).  causal_offset = Nkv - Nq reproduces the reference's
 * tail-aligned causal mask (split_d.cuh:222-228); 0 reproduces PyTorch SDPA's
 * top-left alignment (SURVEY.md §8 "config-4 semantic trap").
 */
typedef struct ffpa_fwd_params {
  uint32_t struct_size; /* sizeof(ffpa_fwd_params), checked */
  uint32_t abi_version; /* FFPA_ATTN_ABI_VERSION            */

  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse;       /* optional */
  const void* bias; /* optional */

  int32_t batch;       /* B   */
  int32_t heads_q;     /* Hq  */
  int32_t heads_kv;    /* Hkv */
  int32_t seqlen_q;    /* Nq  */
  int32_t seqlen_kv;   /* Nkv */
  int32_t head_dim;    /* D: any multiple of 8 in [8, 1024] */

  int64_t q_stride[3];    /* elements: batch, head, row */
  int64_t k_stride[3];
  int64_t v_stride[3];
  int64_t o_stride[3];
  int64_t bias_stride[4]; /* elements: batch, head, row, key (0 = broadcast) */

  int32_t dtype;         /* enum ffpa_dtype      */
  int32_t bias_dtype;    /* enum ffpa_bias_dtype */
  int32_t causal;        /* 0 / 1                */
  int32_t causal_offset; /* visible iff key <= row + causal_offset */

  float softmax_scale;     /* applied to q.k before softmax                       */
  float rescale_threshold; /* lazy-rescale threshold in log2 units; <0 => default
                              8.0 (FFPA_RESCALE_THRESHOLD, csrc/cuffpa/common.cuh:14);
                              0 => exact recurrence                                */
  float dropout_p;         /* [0, 1): P <- keep ? P/(1-p) : 0 after the row sum (prefill.cuh:508-546) */
  uint32_t flags;

  /* Philox4x32-10 key and base counter: element (b,hq,q,k) uses word e&3 of block e>>2 with
   * e = philox_offset + ((b*Hq + hq)*Nq + q)*Nkv + k; keep iff (word+1)*2^-32 > dropout_p — the
   * SDPA-efficient-attention-compatible convention of prefill.cuh:398-452.  The caller reserves the
   * ceil4(B*Hq*Nq*Nkv) offsets from its generator (functional.py:518-540). */
  uint64_t philox_seed;
  uint64_t philox_offset;

  /* Short-query (decode) launches, seqlen_q <= 32 — and prefill launches that would fill less than half of
   * the CUs: the KV axis is split over workgroups and merged by
   * LSE, the role of the reference's split_kv_decode_s1/s2 kernels (native/sm_80/split_kv.cuh:22-455,
   * heuristic native/launch.cuh:17-67).  The caller owns the scratch (the reference allocates it inside
   * the launcher, native/launch.cuh:314-318): size from ffpa_attn_fwd_workspace_bytes(). */
  void* workspace;          /* device scratch, 16-byte aligned; NULL => no split        */
  uint64_t workspace_bytes;
  int32_t num_splits;       /* 0 = library heuristic, 1 = never split, n = at most n     */
  /* Rows of several query heads of one KV group packed into the row axis by the caller (q viewed as
   * [B, Hkv, group*Nq, D]): the causal limit of packed row r is (r % causal_row_mod) + causal_offset.
   * 0 = rows are plain query rows. */
  int32_t causal_row_mod;

  /* Optional key ranges derived from the mask by the caller (NULL = none), four int32 per block of 32 query rows:
   *   {first, end}            EVERY key outside [first, end) is masked (bias == -inf / mask == False) for EVERY row of the
   *                           block; an empty block is {Nkv, 0};
   *   {free_first, free_end}  for EVERY key inside [free_first, free_end) the mask is neutral (bias == 0 / mask == True) for
   *                           EVERY row of the block; {0, 0} = no such claim.
   * Shape [Bb, Hb, ceil(Nq / 32), 4] with element strides kv_bounds_stride = {batch, head} (0 = broadcast);
   * ffpa_attn_mask_kv_bounds() computes it.  The kernel clips its KV-tile loop to the union of its blocks' [first, end) and
   * does not read the mask for tiles inside a block's free range: results are unchanged (the skipped tiles contribute
   * exp(-inf) = 0, the skipped mask reads would have added 0); an explicit causal / sliding-window / padding mask stops
   * costing the tiles it hides AND the tiles it leaves fully visible — only the tiles its edge crosses pay for it.  The
   * reference has no counterpart (it walks every tile and adds the bias everywhere: native/sm_80/split_d.cuh:222-228 clips
   * for is_causal only). */
  const int32_t* kv_bounds;
  int64_t kv_bounds_stride[2];

  /* Optional, short-query (seqlen_q <= 32) KV-split launches only (NULL = none; ignored by other launches):
   * ffpa_attn_fwd_split_tickets(params) int32 counters, ZERO on entry.  With them the
   * split partials are merged inside the same launch — the last split of a row tile to arrive (agent-scope release of its partial, one
   * relaxed atomic ticket, agent-scope acquire by the merger) combines all of them by LSE, writes O / LSE and puts its counter back to
   * zero: one launch per call instead of two, the role of the reference's split_kv_decode stage 2 (native/sm_80/split_kv.cuh:329-455)
   * without its second kernel.  The counters must not be shared by launches that may run concurrently (other streams); after a launch
   * completes they are zero again, so one buffer zeroed once serves every later call on that stream, HIP-graph replays included.
   * Without them a second kernel (ffpa_fwd_merge_kernel) follows the first on the same stream: the same numbers.  Which of the two is
   * faster is a measurement (profiles/r03_split_merge.txt), the Python host's default follows it. */
  int32_t* split_tickets;
} ffpa_fwd_params;

/*
 * Launch the fused forward on `stream` (a hipStream_t; NULL = default stream) of
 * the CURRENT device.  Asynchronous; returns an ffpa_status.
 * Replaces: ffpa_attn._C.ffpa_attn_forward (csrc/cuffpa/ffpa_api.cc:86-239).
 */
int ffpa_attn_fwd(const ffpa_fwd_params* params, void* stream);

/*
 * Scratch bytes the call would use with the split count it would choose (0 when it does not split).
 * Replaces the in-launcher allocations of native/launch.cuh:314-318,503-509.
 */
size_t ffpa_attn_fwd_workspace_bytes(const ffpa_fwd_params* params);

/*
 * Number of int32 counters ffpa_fwd_params.split_tickets must hold for this call (one per (batch, query head, row
 * tile): batch * heads_q * ceil(seqlen_q / block rows) — a short-query launch has one row tile per head today, the count does not
 * rely on it; 0 when the call is not a KV-split short-query launch).  The kernel leaves every counter at zero when the launch
 * completes; after a launch that failed or faulted the caller must zero the buffer again before reusing it.
 */
size_t ffpa_attn_fwd_split_tickets(const ffpa_fwd_params* params);

/*
 * The launch plan for `params` (for benches / roofline maths / tests): out[0] = kernel variant
 * (0 = prefill tiles, 1 = short-query tiles), out[1] = query rows per workgroup, out[2] = keys per
 * tile, out[3] = number of KV splits given params->workspace_bytes.  Returns an ffpa_status.
 */
int ffpa_attn_fwd_plan(const ffpa_fwd_params* params, int out[4]);

/*
 * The kernel the launch described by `params` runs, as text ("ffpa_fwd_m16_kernel<bf16, 512, MK=0, DROP=0>", with
 * " + ffpa_fwd_merge_kernel" appended for KV-split launches): what benches put next to their numbers and what a profile's
 * kernel column must show.  Written to buf (n bytes, NUL-terminated).  Returns an ffpa_status.
 */
int ffpa_attn_fwd_kernel(const ffpa_fwd_params* params, char* buf, size_t n);

/*
 * Visible-key bounds of an additive (-inf = hidden) or boolean (0 = hidden) mask, in the layout
 * ffpa_fwd_params.kv_bounds expects: one fused pass over
 * `bias` ([bb, hb, nq|1, nkv|1] with element strides bias_stride, 0 = broadcast; enum ffpa_bias_dtype) writes
 * out[bb][hb][ceil(nq / 32)][4] = {first, end, free_first, free_end} (int32, contiguous) on `stream`.  Returns an
 * ffpa_status.
 */
int ffpa_attn_mask_kv_bounds(const void* bias, int bias_dtype, const int64_t bias_stride[4], int bb, int hb,
                             int nq, int nkv, int32_t* out, void* stream);

/*
 * PACKED SEQUENCES ("varlen", FlashAttention's THD layout) — the reference's ffpa_attn_varlen_func
 * (src/ffpa_attn/ffpa_attn_interface.py:192-279), which it serves through its CuTe-DSL backend only
 * (torch.ops.ffpa_attn._varlen_fwd_cute, src/ffpa_attn/cute/__init__.py:466-575,792-829: NVIDIA SM8x / SM90 / SM100).
 *
 *   q  [total_q, Hq,  D]     k, v [total_k, Hkv, D]     o [total_q, Hq, D]     (element strides: row, head; head-dim stride 1)
 *   lse [Hq, total_q] fp32, natural log, element stride lse_stride_head between heads; may be NULL
 *   cu_seqlens_q / cu_seqlens_kv: int32 [batch + 1] ON THE DEVICE, non-decreasing, [0] == 0: sequence i owns rows
 *        cu_seqlens_q[i] .. cu_seqlens_q[i + 1] of q / o and cu_seqlens_kv[i] .. cu_seqlens_kv[i + 1] of k / v.
 *
 * ONE launch for the whole batch; the boundaries are read by the kernel (nothing is copied to the host, the call never
 * synchronises and captures into a HIP graph): the grid holds ceil(max_seqlen_q / block rows) row tiles per (sequence,
 * head), workgroups whose tile lies past their sequence's last row leave at once.  max_seqlen_q must be >= every
 * sequence's query length (rows past it would not be computed); max_seqlen_kv is only a hint for the launch side.
 * Short query sequences under GQA — decode (max_seqlen_q == 1), speculative decoding, small prefill chunks: (Hq / Hkv) x max_seqlen_q rows
 * fit one tile — run with the query heads of a KV group x the sequence's tokens packed into the rows of one tile per (sequence, KV head):
 * the group's K / V are read once (the reference's pack_gqa, cute/__init__.py:792-829).
 * Per sequence the arithmetic is the dense call's (same tile, same recurrence: bit-identical to ffpa_attn_fwd on that
 * sequence alone under FFPA_FLAG_DETERMINISTIC).  causal = the reference's tail-aligned mask PER SEQUENCE: row r of
 * sequence i sees key j iff j <= r + (Nkv_i - Nq_i).  Rows without a visible key (an empty key range; the first
 * Nq_i - Nkv_i rows of a causal sequence with more queries than keys) get O = 0 and LSE = -inf — the contract the
 * reference's tests pin for this entry point (tests/test_ffpa_cute_sm100.py:1117-1183) — where ffpa_attn_fwd keeps
 * SDPA's NaN.  No attn_bias, no dropout (the reference rejects both here: cute/__init__.py:76-139).
 */
typedef struct ffpa_varlen_fwd_params {
  uint32_t struct_size; /* sizeof(ffpa_varlen_fwd_params), checked */
  uint32_t abi_version; /* FFPA_ATTN_ABI_VERSION                    */

  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse; /* optional */
  const int32_t* cu_seqlens_q;  /* device, [batch + 1] */
  const int32_t* cu_seqlens_kv; /* device, [batch + 1] */
  const int32_t* seqused_kv;    /* optional, device, [batch]: sequence i uses only its first seqused_kv[i] key rows (clamped to its range) — a KV cache of
                                   fixed capacity per sequence (cu_seqlens_kv = multiples of the capacity) whose valid lengths live on the device and change
                                   between HIP-graph replays; FlashAttention's seqused_k / cache_seqlens.  NULL = every key row of the range */

  int32_t batch;          /* sequences */
  int32_t heads_q;        /* Hq  */
  int32_t heads_kv;       /* Hkv */
  int32_t head_dim;       /* D: any multiple of 8 in [8, 1024] */
  int32_t max_seqlen_q;   /* >= the longest query sequence */
  int32_t max_seqlen_kv;  /* >= the longest key sequence (launch-side hint) */

  int64_t q_stride[2]; /* elements: row, head */
  int64_t k_stride[2];
  int64_t v_stride[2];
  int64_t o_stride[2];
  int64_t lse_stride_head; /* elements between two heads of lse (>= total_q); ignored when lse == NULL */

  int32_t dtype;  /* enum ffpa_dtype */
  int32_t causal; /* 0 / 1: tail-aligned per sequence */

  float softmax_scale;     /* > 0 or < 0 or 0: as ffpa_fwd_params */
  float rescale_threshold; /* as ffpa_fwd_params: < 0 => 8.0 */
  uint32_t flags;          /* FFPA_FLAG_NO_XCD_REMAP, FFPA_FLAG_L2_PREFETCH / _NO_L2_PREFETCH, FFPA_FLAG_XCD_GROUP(), FFPA_FLAG_NO_PACK_GQA, FFPA_FLAG_KV_STREAM / _NO_KV_STREAM, FFPA_FLAG_DETERMINISTIC, FFPA_FLAG_FORCE_SPLITS; others ignored */
  uint32_t reserved;       /* 0 */

  /* KV SPLITS (ABI 6): batches whose (sequence, head) pairs leave most of the chip idle — a decode batch of a few long sequences: 8 sequences x 8 KV heads
   * are 64 workgroups for 256 CUs — split every sequence's KV range over num_splits workgroups (each sequence by ITS OWN length, read on the device:
   * ceil(tiles_i / splits) KV tiles per range), which write normalised fp32 partials + LSE to the workspace; a second kernel of the same call merges them
   * (the reference's decode stage 2, csrc/cuffpa/native/sm_80/split_kv.cuh:329-455).  Still nothing read on the host, still graph-capturable (two nodes).
   * Only launches with ONE row tile per (sequence, head) split (max_seqlen_q <= block rows: decode, speculative decoding, chunked prefill), and only with a
   * workspace: size from ffpa_attn_varlen_fwd_workspace_bytes().  A split launch's bits equal the unsplit launch's to fp32-merge rounding, not to the bit:
   * FFPA_FLAG_DETERMINISTIC or num_splits = 1 keeps one range per sequence. */
  void* workspace;          /* device scratch, 16-byte aligned; NULL => no split */
  uint64_t workspace_bytes;
  int32_t num_splits;       /* 0 = library heuristic, 1 = never split, n = at most n (with FFPA_FLAG_FORCE_SPLITS: exactly n where the key length allows) */
  int32_t total_q;          /* rows of q / o (>= cu_seqlens_q[batch]); 0 => no split (the partials are laid out [split, Hq, total_q, D]; a sequence whose rows
                               lie past total_q is skipped by a split launch — never stored outside the scratch) */
} ffpa_varlen_fwd_params;

/* Launch the packed-sequence forward on `stream` of the CURRENT device.  Asynchronous; returns an ffpa_status. */
int ffpa_attn_varlen_fwd(const ffpa_varlen_fwd_params* params, void* stream);

/* Scratch bytes the packed call wants for the KV split count its heuristic would pick with unlimited scratch (0 = it would not split). */
size_t ffpa_attn_varlen_fwd_workspace_bytes(const ffpa_varlen_fwd_params* params);

/* Its launch plan: out[0] = row tiles per (sequence, head) in the grid, out[1] = query rows per workgroup, out[2] = keys per tile,
 * out[3] = workgroups of the launch (all KV ranges), out[4] = KV ranges per sequence given params->workspace_bytes (ABI 6).  Returns an ffpa_status. */
int ffpa_attn_varlen_fwd_plan(const ffpa_varlen_fwd_params* params, int out[5]);

/* The kernel it runs, as text ("ffpa_fwd_m16_varlen_kernel<bf16, 512>").  Returns an ffpa_status. */
int ffpa_attn_varlen_fwd_kernel(const ffpa_varlen_fwd_params* params, char* buf, size_t n);

/*
 * PAGED KV CACHE (ABI 7) — vLLM / SGLang / FlashAttention's flash_attn_with_kvcache(..., block_table=...): K and V live in a pool of fixed-size pages, and
 * every sequence has a row of page ids.  The packed call above with these changes:
 *   p->k / p->v are the page pools: page p of K starts at k + p * k_page_stride elements (V likewise); inside a page, rows and heads have p->k_stride /
 *        p->v_stride = {row, head}.  Key j of sequence i is row j % page_size of page block_table[i * bt_stride + j / page_size].
 *   p->seqused_kv is REQUIRED: sequence i has Nkv_i = min(seqused_kv[i], pages_per_row * page_size) keys.
 *   p->cu_seqlens_kv may be NULL and is ignored; p->max_seqlen_kv stays a launch-side hint (>= the longest Nkv_i).
 * page_size must be a multiple of 64: the paged kernel's tiles hold 64 keys (32 at D > 512), so a tile never straddles two pages.  Page ids are clamped to
 * [0, num_pages) on the device (a bad table gives a wrong answer, not a fault); entries past a sequence's last used page are never read.  Same bits as the
 * packed call on the gathered keys wherever the tile is the same (every head dim but 256 / 320, where the packed call takes 128-key tiles).
 */
typedef struct ffpa_paged_kv {
  uint32_t struct_size;        /* sizeof(ffpa_paged_kv), checked */
  uint32_t reserved;           /* 0 */
  const int32_t* block_table;  /* device, [batch][bt_stride]: sequence i's page ids in key order */
  int64_t bt_stride;           /* elements between two sequences' rows (>= pages_per_row) */
  int32_t pages_per_row;       /* usable entries per row: Nkv_i is clamped to pages_per_row * page_size */
  int32_t page_size;           /* keys per page: a multiple of 64 */
  int32_t num_pages;           /* pages in the pool (ids are clamped to it) */
  int32_t reserved2;
  int64_t k_page_stride, v_page_stride; /* elements between two pages; multiples of 8 */
} ffpa_paged_kv;

/* Launch the paged forward on `stream` of the CURRENT device.  Asynchronous; returns an ffpa_status. */
int ffpa_attn_varlen_paged_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, void* stream);

/* As ffpa_attn_varlen_fwd_workspace_bytes / _plan / _kernel, for the paged call ("ffpa_fwd_m16_paged_kernel<bf16, 512>"). */
size_t ffpa_attn_varlen_paged_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv);
int ffpa_attn_varlen_paged_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, int out[5]);
int ffpa_attn_varlen_paged_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, char* buf, size_t n);

/*
 * TREE MASK over the last keys of every sequence — the verification step of tree speculative decoding (EAGLE, Medusa, SpecInfer; FlashInfer's custom_mask for
 * that case): the engine has appended the ntok_i draft nodes of sequence i to its keys and calls attention ONCE; node t must see the whole prefix and, among the
 * draft keys, its own ancestors only.  The packed call (kv == NULL) or its paged twin (kv != NULL) with these changes:
 *   the last ntok_i = cu_seqlens_q[i + 1] - cu_seqlens_q[i] keys of sequence i are its DRAFT keys.  Query token t of sequence i sees
 *        key p                        for every p < Nkv_i - ntok_i (the prefix), and
 *        key Nkv_i - ntok_i + j       iff bit j of bits[i * batch_stride + t] is set (0 <= j < ntok_i);
 *        draft positions below key 0 (Nkv_i < ntok_i) do not exist.  The mask is arbitrary: a clear diagonal and "sees a later node" are legal.
 *   p->causal is ignored (all ones below the diagonal IS the causal launch, all ones the non-causal one: the same bits as those launches).  A token whose
 *        word hides every key it could see gives O = 0, LSE = -inf, the packed call's empty-row contract; one token per sequence keeps its mask (bit 0 clear =
 *        "the prefix only").
 *   (ffpa_varlen_fwd_params has no dropout: like the packed call, the tree call cannot be asked for it, so there is nothing to refuse.)
 *   `tokens` words per sequence: max_seqlen_q <= tokens <= 64.  batch_stride = words between two sequences' rows (>= tokens), or 0 = one tree for the batch.
 * Which tiles are walked — the tile range, the KV ranges of a split launch and their share-out, the workgroup order — is the causal launch's, whose last token
 * sees the last key; only the element test of the KV tiles that hold a draft key reads the words.  The words are read on the device at launch time: a captured
 * graph follows words written in place.
 */
typedef struct ffpa_tree_mask {
  uint32_t struct_size;  /* sizeof(ffpa_tree_mask), checked */
  uint32_t reserved;     /* 0 */
  const uint64_t* bits;  /* device, 8-byte aligned: [batch or 1][tokens] words */
  int64_t batch_stride;  /* words between two sequences (>= tokens); 0 = every sequence reads row 0 */
  int32_t tokens;        /* words per sequence: 1 ... 64, >= max_seqlen_q */
  int32_t reserved2;
} ffpa_tree_mask;

/* Launch the forward under a tree mask on `stream` of the CURRENT device (kv: the paged pool, NULL = the packed call's contiguous keys).  Asynchronous; every bad
 * argument returns a status before any device work.  Returns an ffpa_status. */
int ffpa_attn_varlen_tree_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_tree_mask* tree, void* stream);

/* As ffpa_attn_varlen_fwd_workspace_bytes / _plan / _kernel, for the tree call ("ffpa_fwd_m16_paged_tree_kernel<bf16, 512>": the packed / paged kernel's build that tests mask words; the plan is that call's own). */
size_t ffpa_attn_varlen_tree_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_tree_mask* tree);
int ffpa_attn_varlen_tree_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_tree_mask* tree, int out[5]);
int ffpa_attn_varlen_tree_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_tree_mask* tree, char* buf, size_t n);

/*
 * SLIDING WINDOW (local attention: Mistral, Gemma 2 / 3, Phi-3; FlashAttention's window_size = (left, right)) over the packed call (kv == NULL) or its paged
 * twin (kv != NULL).  With L_i the keys of sequence i, ntok_i its query tokens and pos_t = t + L_i - ntok_i the position of token t (bottom-right aligned),
 * token t sees key j iff
 *        0 <= j < L_i,   left < 0 or j >= pos_t - left,   right < 0 or j <= pos_t + right          (-1 = unbounded on that side).
 *   p->causal means right = 0, whatever `right` says (FlashAttention's rule).  (-1, -1) without the causal flag is the plain launch and (-1, 0) the causal one: the
 *   same bits as those launches.  A token that sees no key gives O = 0, LSE = -inf, the packed call's empty-row contract.  One token per sequence — decode —
 *   keeps its left bound.
 * A row tile walks only the KV tiles between the left bound of its first token and the right bound of its last one — the tiles (and, paged, the pages) in front
 * of the window are never read —, a split launch's KV ranges share out those tiles, and the launch plan (the split count, the non-temporal fetch) prices the
 * widest key span a row tile can see, left + min(max_seqlen_q, tile rows + right) keys rounded up to a KV tile, instead of max_seqlen_kv: a 4k window over a
 * 32k cache plans like a 4k cache.
 */
typedef struct ffpa_window {
  uint32_t struct_size;  /* sizeof(ffpa_window), checked */
  uint32_t reserved;     /* 0, checked */
  int32_t left;          /* keys visible in front of a token's position; -1 = all of them */
  int32_t right;         /* keys visible behind it; -1 = all of them (p->causal: taken as 0) */
} ffpa_window;

/* Launch the forward under a sliding window on `stream` of the CURRENT device (kv: the paged pool, NULL = the packed call's contiguous keys).  Asynchronous; every
 * bad argument — a NULL w, a wrong struct_size, a non-zero reserved, left or right below -1 — returns a status before any device work.  Returns an ffpa_status. */
int ffpa_attn_varlen_window_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, void* stream);

/* As ffpa_attn_varlen_fwd_workspace_bytes / _plan / _kernel, for the window call ("ffpa_fwd_m16_paged_window_kernel<bf16, 512>"; the plan is the window's own). */
size_t ffpa_attn_varlen_window_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w);
int ffpa_attn_varlen_window_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, int out[5]);
int ffpa_attn_varlen_window_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, char* buf, size_t n);

/*
 * LOGIT SOFT-CAPPING (FlashAttention's softcap; Gemma 2 caps at 50, Grok-1 at 30) over the window call: with c = softcap,
 *        score(t, j) = c * tanh(softmax_scale * q_t.k_j / c),
 *   the mask — the key length, the causal edge, the window's edges — is applied to the CAPPED score (a hidden key has weight 0), and the softmax, O and the LSE
 *   (natural log) are taken over the capped scores.  A token that sees no key gives O = 0, LSE = -inf.  w == NULL means no window, (-1, -1): one kernel family
 *   (the *_softcap_kernel builds: the window builds with the cap on) serves capped layers with and without a window.  softcap must be finite and > 0: anything
 *   else returns a status before any device work ("off" is the window call).  Every other check, the plan (row tiles, rows, keys per tile, workgroups, splits) and
 *   the workspace are the window call's for the same (p, kv, w): the cap changes no tile count, and a split launch's partials are ordinary (O, LSE) states.
 *   The tanh is one exp2 and one rcp per score, 1 - 2 / (1 + exp2(2 log2(e) y)): absolute error <= 2^-21, so a capped score is off by at most c * 2^-21.
 */
int ffpa_attn_varlen_softcap_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, float softcap, void* stream);

/* As ffpa_attn_varlen_window_fwd_workspace_bytes / _plan / _kernel, for the soft-capping call ("ffpa_fwd_m16_paged_softcap_kernel<bf16, 512>"; a bad softcap:
 * 0 bytes / a status). */
size_t ffpa_attn_varlen_softcap_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, float softcap);
int ffpa_attn_varlen_softcap_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, float softcap, int out[5]);
int ffpa_attn_varlen_softcap_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_window* w, float softcap, char* buf, size_t n);

/*
 * MLA LATENT CACHE (multi-head latent attention in its "absorbed" decode form: DeepSeek-V2 / V3 / R1, Kimi K2) over the paged call: ONE pool holds the latent
 * rows, the keys of KV head h are a row's p->head_dim columns and its values the FIRST head_dim_v columns of the same row.  The paged call with these changes:
 *   kv is REQUIRED (a contiguous cache is a pool of one page per sequence: page_size = its capacity, a multiple of 64, and an identity block table).
 *   p->k is the latent pool (p->k_stride = {row, head} inside a page, kv->k_page_stride between pages); p->v, p->v_stride and kv->v_page_stride are NOT READ.
 *   p->o is [total_q, heads_q, head_dim_v] by p->o_stride: only columns < head_dim_v are stored.  p->lse as in the paged call.
 *   (p->head_dim, head_dim_v) must be a pair the library is built for — (576, 512) — and in general multiples of 64 with head_dim_v <= head_dim.
 *   p->softmax_scale is the caller's: these models scale by 1 / sqrt(qk_nope + qk_rope) (x their YaRN factor), which is not 1 / sqrt(head_dim).
 * A latent row is fetched once per workgroup (the kernel reads the K and the V^T fragments of a tile from one LDS image).  The heads_q / heads_kv query heads of
 * a KV head x the sequence's tokens are the rows of its tiles, head-major, however many they are: ceil(group * max_seqlen_q / block rows) row tiles per
 * (sequence, KV head), neighbours in the launch order — 128 heads on one latent head are two 64-row tiles per sequence (FFPA_FLAG_NO_PACK_GQA: one workgroup
 * per query head).  The non-temporal fetch is taken only where a latent byte has one reader: one row tile.
 * APPEND (seqlen_new > 0): row i of sequence b of kv_new ([batch, seqlen_new, heads_kv, head_dim] by kv_new_stride = {batch, row, head}) is first written — once —
 * at cache position max(cache_seqlens[b], 0) + i (dropped at or past pages_per_row * page_size), by one more launch on `stream` in front of the attention
 * launch, which also writes p->seqused_kv[b] = min(max(cache_seqlens[b], 0) + seqlen_new, capacity): p->seqused_kv is then an OUTPUT (and the lengths attention
 * runs over) and must not be cache_seqlens.  No rotary: these models rotate k_pe / q_pe before the concatenation.
 * RAGGED STEPS (sequences with different numbers of query tokens: MTP / speculative verification, an extend chunk among decodes): p->cu_seqlens_q says them, as
 * in the packed call, and a sequence of len_b tokens has ceil(group * len_b / block rows) row tiles.  The step's append is ffpa_attn_mla_append_varlen (below) in
 * front of this call with seqlen_new = 0 and p->seqused_kv = that call's `seqused`, on one stream.  When at least three quarters of the full grid of
 * batch * ceil(group * max_seqlen_q / block rows) row tiles per KV head would find no row, the grid is sized by the rows there are:
 * ceil(group * total_q / block rows) + batch slots per KV head (an upper bound of the sum of the sequences' tiles), each finding its (sequence, row tile) on the
 * device; FFPA_FLAG_NO_COMPACT_GRID keeps the full grid (same order, same bits).  Packing and the non-temporal fetch stay launch-wide decisions.
 * Not served (use the other calls on a (kv, kv) pair): windows, soft-capping; tree masks are ffpa_attn_varlen_mla_tree_fwd's and FP8 latents (a pool of e4m3
 * codes under one scale) ffpa_attn_varlen_mla_fp8_fwd's (both below): this call reads 16-bit pools only.
 */
typedef struct ffpa_mla {
  uint32_t struct_size;          /* sizeof(ffpa_mla), checked */
  uint32_t reserved;             /* 0, checked */
  int32_t head_dim_v;            /* value width: the first head_dim_v columns of a latent row */
  int32_t seqlen_new;            /* rows per sequence of kv_new; 0 = nothing is appended */
  const void* kv_new;            /* device, 16-byte aligned; read when seqlen_new > 0 */
  const int32_t* cache_seqlens;  /* device [batch]: the lengths before the step; read when seqlen_new > 0 */
  int64_t kv_new_stride[3];      /* elements: batch, row, head */
} ffpa_mla;

/* Launch the latent-cache forward (and, in front of it, the append) on `stream` of the CURRENT device.  Asynchronous; every bad argument — a NULL kv or m, a wrong
 * struct_size, a non-zero reserved, a value width that is no multiple of 64 in [64, head_dim], a pair that is not built — returns a status before any device
 * work.  Returns an ffpa_status. */
int ffpa_attn_varlen_mla_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, void* stream);

/* As ffpa_attn_varlen_fwd_workspace_bytes / _plan / _kernel, for the latent-cache call ("ffpa_fwd_m16_mla_kernel<bf16, 576, dv=512>"; out[0] = row tiles per
 * (sequence, KV head) when the heads are packed into rows). */
size_t ffpa_attn_varlen_mla_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m);
int ffpa_attn_varlen_mla_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, int out[5]);
int ffpa_attn_varlen_mla_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, char* buf, size_t n);

/* *slots = row-tile slots per KV head of the compact grid the plan takes for this call (out[3] of the plan is then slots * heads_kv * KV ranges, and the kernel
 * text carries "(compact grid)"); 0 = the full grid.  Returns an ffpa_status. */
int ffpa_attn_varlen_mla_fwd_compact_slots(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, int* slots);

/*
 * TREE MASK OVER THE LATENT CACHE — the verification step of tree speculative decoding for the models above (their MTP head driven as an EAGLE draft model with a
 * tree of more than one branch): the latent call under an ffpa_tree_mask.  The ntok_i = cu_seqlens_q[i + 1] - cu_seqlens_q[i] draft nodes of sequence i are the
 * LAST rows of its latent cache (L_i = p->seqused_kv[i] clamped to the capacity — with m->seqlen_new > 0, the length behind the append).  Query token t sees
 *        row p                      for every p < L_i - ntok_i (the prefix), and
 *        row L_i - ntok_i + j       iff bit j of tree->bits[i * batch_stride + t] is set (0 <= j < ntok_i); draft positions below row 0 do not exist.
 *   ffpa_tree_mask keeps its meaning (one word per (sequence, token), batch_stride = 0: one tree for the batch, tokens in 1 ... 64 and >= max_seqlen_q, the token
 *   index clamped on the device); p->causal is ignored: the launch, its plan, its KV ranges, the row chunks of a group wider than the tile and the compact grid are
 *   ffpa_attn_varlen_mla_fwd's UNDER THE CAUSAL FLAG for the same (p, kv, m).  One token per sequence keeps its mask: a clear bit 0 hides the token's own row.
 *   A token that sees no row gives O = 0, LSE = -inf.  All ones below the diagonal IS the causal latent launch and all ones the non-causal one, to the bit.
 * The kernel is the latent kernel's text with the tree hook on (ffpa_fwd_m16_mla_tree_kernel): only the element test of the 32-key tiles that hold a draft row —
 * at most three, plus the tail — reads the words.  The append is the latent call's (m->seqlen_new > 0), or ffpa_attn_mla_append_varlen in front for a ragged step.
 * Every bad argument — those of ffpa_attn_varlen_mla_fwd, then a NULL tree, a wrong struct_size, NULL or misaligned bits, tokens outside [max_seqlen_q, 64], a
 * batch_stride in (0, tokens) — returns a status before any device work.  Returns an ffpa_status.
 */
int ffpa_attn_varlen_mla_tree_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, void* stream);

/* As ffpa_attn_varlen_mla_fwd_workspace_bytes / _plan / _kernel / _compact_slots, for the tree-mask latent call ("ffpa_fwd_m16_mla_tree_kernel<bf16, 576,
 * dv=512>"; the plan is ffpa_attn_varlen_mla_fwd_plan's with p->causal = 1). */
size_t ffpa_attn_varlen_mla_tree_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree);
int ffpa_attn_varlen_mla_tree_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, int out[5]);
int ffpa_attn_varlen_mla_tree_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, char* buf, size_t n);
int ffpa_attn_varlen_mla_tree_fwd_compact_slots(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, int* slots);

/*
 * LATENT APPEND OF A RAGGED STEP — the launch in front of ffpa_attn_varlen_mla_fwd when the sequences of a step bring different numbers of new latent rows.
 * kv_new [total_q, heads_kv, head_dim] by kv_new_stride = {row, head} is packed by cu_seqlens_q (device int32 [batch + 1], ascending from 0) exactly as the
 * step's q: token row t belongs to the sequence b with cu_seqlens_q[b] <= t < cu_seqlens_q[b + 1], found on the device, as its token i = t - cu_seqlens_q[b].
 * ONE kernel on `stream`:
 *   * row t is written — once, as 16-byte chunks — at cache position pos = max(cache_seqlens[b], 0) + i of the latent pool kv_cache: row pos % page_size of page
 *     kv->block_table[b * bt_stride + pos / page_size] (ids clamped to [0, num_pages); pages by kv->k_page_stride, rows and heads inside a page by
 *     kv_cache_stride = {row, head}; kv->v_page_stride is not read).  A position at or past pages_per_row * page_size is dropped.  Rows from
 *     cu_seqlens_q[batch] on (total_q may exceed it) are padding: nothing is written for them.
 *   * seqused[b] = min(max(cache_seqlens[b], 0) + (cu_seqlens_q[b + 1] - cu_seqlens_q[b]), capacity) for every b < batch — sequences without a token too, and
 *     with total_q < batch or total_q == 0 as well: the lengths the attention launch that follows reads (its seqused_kv).  cache_seqlens is not modified;
 *     seqused must be another buffer.
 * No rotary and no positions: MLA rotates k_pe / q_pe before the concatenation.  A contiguous cache is a pool of one page per sequence, as in the forward call.
 */
typedef struct ffpa_mla_append_varlen_params {
  uint32_t struct_size;          /* sizeof(ffpa_mla_append_varlen_params), checked */
  uint32_t reserved;             /* 0, checked */
  const void* kv_new;            /* device [total_q, heads_kv, head_dim], 16-byte aligned; may be NULL when total_q == 0 */
  void* kv_cache;                /* the latent pool, written in place; 16-byte aligned */
  const int32_t* cu_seqlens_q;   /* device [batch + 1] */
  const int32_t* cache_seqlens;  /* device [batch]: the lengths before the step, not modified */
  int32_t* seqused;              /* out, device [batch] */
  int64_t kv_new_stride[2];      /* elements: row, head (head-dim stride 1; multiples of 8) */
  int64_t kv_cache_stride[2];    /* elements: row, head inside a page */
  int32_t batch;
  int32_t total_q;               /* >= 0: token rows of kv_new (the grid); 0 = only seqused is written */
  int32_t heads_kv;
  int32_t head_dim;              /* a multiple of 8 in [8, 1024] */
  int32_t dtype;                 /* enum ffpa_dtype (16-bit elements move as raw bytes) */
  int32_t reserved2;             /* 0, checked */
} ffpa_mla_append_varlen_params;

/* Launch the ragged latent append on `stream` of the CURRENT device.  Asynchronous: no allocation, no synchronisation; every bad argument — a NULL params, kv or
 * pointer, a wrong struct_size, a non-zero reserved, a misaligned base, seqused == cache_seqlens, head_dim % 8, a page_size that is no multiple of 64 — returns a
 * status before any device work.  Returns an ffpa_status. */
int ffpa_attn_mla_append_varlen(const ffpa_mla_append_varlen_params* p, const ffpa_paged_kv* kv, void* stream);

/*
 * FP8 LATENT CACHE — ffpa_attn_varlen_mla_fwd over a pool that holds OCP e4m3 codes (1 byte per element, "float8_e4m3fn"; NOT the fnuz format, NOT e5m2) with ONE
 * per-tensor scale: K = kv_scale * K8, the serving engines' kv_cache_dtype = "fp8" for the latent cache of the MLA models.  ffpa_attn_varlen_mla_fwd with these
 * changes:
 *   * p->k is the FP8 pool.  p->dtype stays the dtype of q, o and kv_new (bf16 / fp16).  p->k_stride, kv->k_page_stride and the append's strides are in ELEMENTS OF
 *     THE POOL (bytes); rows, heads and pages must be multiples of 16 elements apart (FFPA_ERR_BAD_STRIDE) and the base 16-byte aligned.
 *   * there is no FP8 arithmetic.  Every e4m3 value is exactly a bf16 and exactly an fp16: the kernel widens a tile on its way into LDS and runs the 16-bit latent
 *     kernel's MFMAs on it; the scale never touches an element — the scores are (softmax_scale * kv_scale) * q.K8 and O = kv_scale * sum p K8[:, :head_dim_v].
 *     With a power-of-two kv_scale the call returns the bits of ffpa_attn_varlen_mla_fwd on the dequantised pool.
 *   * m->kv_new (p->dtype) is QUANTISED by the append in front of the attention launch, one store per element:
 *         code = rne_e4m3(clamp(float32(x) * float32(1 / kv_scale), -448, +448)),   NaN stays NaN, +-inf saturates to +-448.
 *   * the plan is the latent call's with the cache priced at one byte per element (the non-temporal rule sees half the bytes).
 * The kernel name reads ffpa_fwd_m16_mla_fp8_kernel<bf16, 576, dv=512>...  FP8 pools in the tree-mask and the sparse call: ffpa_attn_varlen_mla_tree_fp8_fwd and
 * ffpa_attn_varlen_mla_sparse_fp8_fwd (below).  Per-block scales inside the row — the 656-byte row layout of DeepSeek-V3.2 — are served by the sparse call alone:
 * ffpa_attn_varlen_mla_sparse_ds_fwd (below).  Not served: that layout in this call and in the tree-mask call, an FP8 q, a kv_scale that lives on the device, FP8
 * in the two-cache (non-MLA) calls.
 */
typedef struct ffpa_mla_fp8 {
  uint32_t struct_size; /* sizeof(ffpa_mla_fp8), checked */
  uint32_t reserved;    /* 0, checked */
  float kv_scale;       /* finite and > 0 (FFPA_ERR_BAD_SHAPE): the dequantisation factor, K = kv_scale * K8 */
  float reserved2;      /* 0, checked */
} ffpa_mla_fp8;

/* Launch on `stream` of the CURRENT device, as ffpa_attn_varlen_mla_fwd.  Every bad argument — those of ffpa_attn_varlen_mla_fwd, a NULL f8, a wrong struct_size, a
 * non-zero reserved field, a kv_scale that is not finite or not positive, a stride that is no multiple of 16 — returns a status before any device work. */
int ffpa_attn_varlen_mla_fp8_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_mla_fp8* f8, void* stream);
size_t ffpa_attn_varlen_mla_fp8_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_mla_fp8* f8);
int ffpa_attn_varlen_mla_fp8_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_mla_fp8* f8, int out[5]);
int ffpa_attn_varlen_mla_fp8_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_mla_fp8* f8, char* buf, size_t n);
int ffpa_attn_varlen_mla_fp8_fwd_compact_slots(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_mla_fp8* f8, int* slots);

/* The ragged latent append (ffpa_attn_mla_append_varlen) into an FP8 pool: p->dtype is kv_new's (bf16 / fp16), p->kv_cache the FP8 pool, kv_cache_stride and
 * kv->k_page_stride in elements of the pool (multiples of 16); every row is quantised as above, every rule of ffpa_attn_mla_append_varlen holds. */
int ffpa_attn_mla_fp8_append_varlen(const ffpa_mla_append_varlen_params* p, const ffpa_paged_kv* kv, const ffpa_mla_fp8* f8, void* stream);

/*
 * SPARSE (top-k indexed) attention over the MLA latent cache — DeepSeek-V3.2's "DeepSeek Sparse Attention" in its absorbed decode form, FlashMLA's sparse decode
 * call: an indexer has picked, per query token, `topk` latent rows (shared by all heads of the token), and the token attends to those rows only.  The latent
 * call with these changes (no ffpa_paged_kv, no ffpa_mla: this struct carries what they would):
 *   p->q [batch, heads_q, head_dim] holds one query TOKEN per "sequence": batch = the number of tokens T, p->max_seqlen_q must be 1, p->total_q = T and
 *        p->cu_seqlens_q the identity boundaries 0, 1, ..., T (device, [T + 1]).  p->max_seqlen_kv is not read (the plan prices topk keys per token).
 *   p->k is the latent pool: slot r of latent head h starts at k + r * kv_stride[0] + h * kv_stride[1] elements, 0 <= r < num_rows (a page pool whose pages are
 *        evenly spaced is this with r = page * page_size + row).  p->k_stride, p->v, p->v_stride, p->cu_seqlens_kv and p->seqused_kv are NOT READ.
 *   Token t attends to slots indices[t * indices_stride + j], 0 <= j < n_t, n_t = clamp(topk_lens[t], 0, topk) (topk_lens == NULL: n_t = topk); duplicates count
 *        twice.  Entries at and past n_t are never turned into an address, whatever they hold (engines pad with -1).  An entry in front of n_t outside
 *        [0, num_rows) is clamped into the pool: memory-safe, the token's result unspecified.  -1 holes INSIDE a row are not served: compact the row first.
 *   A token with n_t = 0 gives O = 0 and LSE = -inf.  p->o, p->lse, p->softmax_scale, the workspace fields and the flags as in the latent call.
 *   (p->head_dim, head_dim_v) as in the latent call: (576, 512).
 * The kernel is a build of the latent kernel that reads a tile's rows where they lie: each wave reads the ids of its eight keys of a tile with scalar loads and
 * turns them into the source offsets of its LDS-DMA pieces — no gathered copy of the rows.  All offsets are 32-bit and bit 31 marks "no row", so the rows of a head
 * must span at most 2^31 bytes: (num_rows - 1) * kv_stride[0] * 2 + head_dim * 2 <= 2^31 (about 1.86 M contiguous 576-wide rows), else FFPA_ERR_BAD_SHAPE.
 * The plan is the latent call's for T one-token sequences of topk keys (row chunks of a group wider than the tile, KV ranges + merge, the non-temporal fetch).
 */
typedef struct ffpa_mla_sparse {
  uint32_t struct_size;         /* sizeof(ffpa_mla_sparse), checked */
  uint32_t reserved;            /* 0, checked */
  const int32_t* indices;       /* device, 4-byte aligned: [batch][indices_stride] slots, the first topk of a row are the token's list */
  int64_t indices_stride;       /* elements between two tokens' rows (>= topk) */
  const int32_t* topk_lens;     /* optional, device [batch]: valid entries per row (clamped to [0, topk]); NULL = topk */
  int64_t kv_stride[2];         /* elements: between two slots, between two latent heads (multiples of 8; slots must not overlap, < 2^24 apart) */
  int32_t topk;                 /* entries per row, >= 1 */
  int32_t num_rows;             /* slots in the pool, >= 1 (ids are clamped to it) */
  int32_t head_dim_v;           /* value width: the first head_dim_v columns of a latent row */
  int32_t reserved2;            /* 0, checked */
} ffpa_mla_sparse;

/* Launch the sparse latent forward on `stream` of the CURRENT device.  Asynchronous, nothing is read on the host; every bad argument returns a status before any
 * device work.  Returns an ffpa_status. */
int ffpa_attn_varlen_mla_sparse_fwd(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, void* stream);

/* As ffpa_attn_varlen_mla_fwd_workspace_bytes / _plan / _kernel, for the sparse call ("ffpa_fwd_m16_mla_sparse_kernel<bf16, 576, dv=512>"). */
size_t ffpa_attn_varlen_mla_sparse_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s);
int ffpa_attn_varlen_mla_sparse_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, int out[5]);
int ffpa_attn_varlen_mla_sparse_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, char* buf, size_t n);

/*
 * FP8 POOLS IN THE TREE-MASK AND THE SPARSE LATENT CALL — an engine that keeps the latent cache as e4m3 codes keeps it so for every attention call of a step.
 *
 * ffpa_attn_varlen_mla_tree_fp8_fwd is ffpa_attn_varlen_mla_tree_fwd over the pool of ffpa_attn_varlen_mla_fp8_fwd: every rule of the tree-mask latent call (the
 * causal flag is not read, the mask words, tokens <= 64) and every rule of the FP8 latent call (p->k holds e4m3 codes, strides in elements of the pool and
 * multiples of 16, K = kv_scale * K8, m->kv_new quantised by the same append in front of the launch, the plan priced at one byte per element).  Checks in the
 * order: f8, the params and the plan, kv, m, tree, the FP8 stride rule.  The kernel name reads ffpa_fwd_m16_mla_tree_fp8_kernel<bf16, 576, dv=512>...
 *
 * ffpa_attn_varlen_mla_sparse_fp8_fwd is ffpa_attn_varlen_mla_sparse_fwd over such a pool: p->k holds e4m3 codes, s->kv_stride is in elements of the pool (bytes)
 * and both strides must be multiples of 16 (FFPA_ERR_BAD_STRIDE); nothing is appended.  The reach of the addressing is the same 2^31 BYTES per latent head, which
 * a pool of one byte per element fills with twice as many rows: (num_rows - 1) * kv_stride[0] + head_dim <= 2^31 (about 3.7 M contiguous 576-wide rows), else
 * FFPA_ERR_BAD_SHAPE.  Entries at and past a token's count are never turned into an address, entries in front of it are clamped into the pool, as in the 16-bit
 * call.  Checks in the order: f8, s and the params, the plan, the (head_dim, head_dim_v) pair, the pool's geometry, the FP8 stride rule.  The kernel name reads
 * ffpa_fwd_m16_mla_sparse_fp8_kernel<bf16, 576, dv=512>...
 *
 * Both: with a power-of-two kv_scale the call returns the bits of its 16-bit twin on the dequantised pool under softmax_scale * kv_scale, O scaled by kv_scale.
 */
int ffpa_attn_varlen_mla_tree_fp8_fwd(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, const ffpa_mla_fp8* f8,
                                      void* stream);
size_t ffpa_attn_varlen_mla_tree_fp8_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree,
                                                         const ffpa_mla_fp8* f8);
int ffpa_attn_varlen_mla_tree_fp8_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree, const ffpa_mla_fp8* f8,
                                           int out[5]);
int ffpa_attn_varlen_mla_tree_fp8_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree,
                                             const ffpa_mla_fp8* f8, char* buf, size_t n);
int ffpa_attn_varlen_mla_tree_fp8_fwd_compact_slots(const ffpa_varlen_fwd_params* p, const ffpa_paged_kv* kv, const ffpa_mla* m, const ffpa_tree_mask* tree,
                                                    const ffpa_mla_fp8* f8, int* slots);
int ffpa_attn_varlen_mla_sparse_fp8_fwd(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, const ffpa_mla_fp8* f8, void* stream);
size_t ffpa_attn_varlen_mla_sparse_fp8_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, const ffpa_mla_fp8* f8);
int ffpa_attn_varlen_mla_sparse_fp8_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, const ffpa_mla_fp8* f8, int out[5]);
int ffpa_attn_varlen_mla_sparse_fp8_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, const ffpa_mla_fp8* f8, char* buf, size_t n);

/*
 * THE 656-BYTE FP8 LATENT ROWS OF DEEPSEEK-V3.2 IN THE SPARSE CALL — the row format in which the engines that serve that model keep its latent cache (vLLM's
 * "fp8_ds_mla", the FP8 KV layout of FlashMLA's sparse decode).  One row of one latent head:
 *     bytes   0 ... 511   the 512 latent ("NoPE") columns as OCP e4m3 codes
 *     bytes 512 ... 527   four little-endian float32 scales, one per 128 columns
 *     bytes 528 ... 655   the 64 rotary columns as bf16, not quantised
 * and what the kernel computes on is, to the bit, column c < 512 = bf16_rne(float32(code[c]) * scale[c / 128]) — one float32 multiply, one rounding — next to the
 * rotary columns as they are.  A scale outside [2^-100, 2^100] or not finite gives unspecified values for its 128 columns and nothing else: no address depends on
 * a scale.
 *
 * ffpa_attn_varlen_mla_sparse_ds_fwd is ffpa_attn_varlen_mla_sparse_fwd over such a pool: p->k is the BYTE pool, s->kv_stride is in bytes; there is no ffpa_mla_fp8
 * (the scales lie in the rows) and nothing is folded into the softmax scale: the call returns the bits of ffpa_attn_varlen_mla_sparse_fwd on the unpacked pool.
 * The checks are those of ffpa_attn_varlen_mla_sparse_fp8_fwd — s and the params, the plan, the (head_dim, head_dim_v) pair — then, in this order: p->dtype must
 * be bf16 (FFPA_ERR_BAD_DTYPE: the rotary bytes reach the kernel's image as they are), (head_dim, head_dim_v) = (576, 512) (FFPA_ERR_BAD_HEADDIM), both strides
 * multiples of 16 with slots at least 656 bytes apart (FFPA_ERR_BAD_STRIDE), a 16-byte aligned pool base (FFPA_ERR_MISALIGNED), and the reach of the addressing:
 * (num_rows - 1) * kv_stride[0] + 656 <= 2^31 (about 3.27 M contiguous rows), else FFPA_ERR_BAD_SHAPE.  Entries at and past a token's count are never turned
 * into an address — on the scale's load as little as on the codes' —, entries in front of it are clamped into the pool.  The plan is the sparse FP8 call's.  The
 * kernel name reads ffpa_fwd_m16_mla_sparse_ds_kernel<bf16, 576, dv=512>...
 * Not served: an fp16 q, ue8m0 / power-of-two scale variants of the row, this layout in the dense latent call and the tree-mask call, -1 holes inside an index row.
 */
int ffpa_attn_varlen_mla_sparse_ds_fwd(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, void* stream);
size_t ffpa_attn_varlen_mla_sparse_ds_fwd_workspace_bytes(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s);
int ffpa_attn_varlen_mla_sparse_ds_fwd_plan(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, int out[5]);
int ffpa_attn_varlen_mla_sparse_ds_fwd_kernel(const ffpa_varlen_fwd_params* p, const ffpa_mla_sparse* s, char* buf, size_t n);

/*
 * THE STORE OF SUCH ROWS, BY SLOT — engines write this cache through a slot mapping, not through sequence lengths.  ONE kernel on `stream`: row t of kv_new
 * [tokens, heads_kv, 576] (bf16, by kv_new_stride = {token, head} in elements) is packed into slot slots[t] of the pool (kv_cache_stride = {slot, head} in
 * bytes).  For each of the four 128-column tiles x of the first 512 columns:
 *     a = amax(|float32(x)|) with non-finite elements counted as 0;   s = max(a / 448, 2^-100) in float32;
 *     code = rne_e4m3(clamp(float32(x) / s, -448, +448)),   NaN stays NaN (x's sign), +-inf saturates;   both divisions correctly rounded,
 * then the four s and the rotary columns' bytes as they are.  A slot < 0 (the engines' padding) or >= num_rows writes nothing; two tokens with one slot are the
 * caller's error (one of them wins).  Nothing is read back: the launch captures into a graph.
 */
typedef struct ffpa_mla_ds_store_params {
  uint32_t struct_size;       /* sizeof(ffpa_mla_ds_store_params), checked */
  uint32_t reserved;          /* 0, checked */
  const void* kv_new;         /* device [tokens, heads_kv, 576] bf16, 16-byte aligned; may be NULL when tokens == 0 */
  const int32_t* slots;       /* device [tokens] */
  void* kv_cache;             /* the byte pool, written in place; 16-byte aligned */
  int64_t kv_new_stride[2];   /* elements: token, head (multiples of 8) */
  int64_t kv_cache_stride[2]; /* bytes: slot, head (multiples of 16; slots >= 656 apart) */
  int32_t tokens;             /* >= 0 */
  int32_t heads_kv;
  int32_t num_rows;           /* slots in the pool */
  int32_t head_dim;           /* 576 */
  int32_t dtype;              /* FFPA_DTYPE_BF16 */
  int32_t reserved2;          /* 0, checked */
} ffpa_mla_ds_store_params;

/* Launch the store on `stream` of the CURRENT device.  Asynchronous; every bad argument returns a status before any device work.  Returns an ffpa_status. */
int ffpa_attn_mla_ds_store(const ffpa_mla_ds_store_params* p, void* stream);

/*
 * THE INPUTS OF THE SPARSE LATENT CALLS, MADE ON THE DEVICE — from an indexer's float32 score per (query token, logical key position) to (indices [T, topk],
 * topk_lens [T]) of ffpa_mla_sparse, in ONE kernel on `stream`, a workgroup per token row.  Exactly one of `scores` and `positions` is non-NULL.
 *   Token t -> (sequence b, token i of its S): cu_seqlens_q [B + 1] and the ragged calls' binary search (rows at and past cu_seqlens_q[B] are padding: count 0, a
 *     row of -1), or — cu_seqlens_q NULL — T % B == 0, S = T / B, b = t / S, i = t % S.
 *   scores [T, N_or_topk] (row_stride in elements, unit stride inside a row): token t sees the columns [0, n), n = clamp(cache_seqlens[b] - (S - 1 - i), 0, N)
 *     with `causal`, clamp(cache_seqlens[b], 0, N) without; columns at and past n are never selected, whatever they hold.  n <= topk: all of [0, n) are selected.
 *     Otherwise the topk largest in the order of a stable descending sort in which NaN is the largest value, -0.0 equals +0.0 and, among equal scores, the
 *     lower position wins.  The selected positions are written in ASCENDING position order; topk_lens[t] = min(n, topk).
 *   positions [T, topk] (N_or_topk == topk): the entries >= 0 keep their order and move to the front; topk_lens[t] is their number.  cache_seqlens is not read
 *     for a length here (the caller's own top-k has applied it).
 *   Either way position p of sequence b is written as block_table[b * block_table_stride + min(p / page_size, W - 1)] * page_size + p % page_size (int32, page
 *     ids not validated: the sparse call clamps slots into the pool) — block_table NULL: as p itself —, and the entries at and past the count are -1.
 * Nothing is read back: the launch captures into a graph in front of the sparse call.  Checks, in this order: p NULL (FFPA_ERR_NULL_POINTER); struct_size,
 * reserved (FFPA_ERR_BAD_ABI); both or neither of scores / positions (FFPA_ERR_NULL_POINTER); T < 0, N_or_topk outside [1, 2^30], topk < 1, positions with
 * topk != N_or_topk, B < 1, T % B != 0 without cu_seqlens_q, causal outside {0, 1}, and — with a block_table — page_size < 1 or W < 1 (FFPA_ERR_BAD_SHAPE);
 * negative strides, indices_stride < topk (FFPA_ERR_BAD_STRIDE); then, T > 0: cache_seqlens / indices / topk_lens NULL (FFPA_ERR_NULL_POINTER), a pointer not
 * 4-byte aligned (FFPA_ERR_MISALIGNED), the device.
 */
typedef struct ffpa_mla_sparse_topk_params {
  uint32_t struct_size;          /* sizeof(ffpa_mla_sparse_topk_params), checked */
  uint32_t reserved;             /* 0, checked */
  const float* scores;           /* device [T, N_or_topk] float32, or NULL */
  const int32_t* positions;      /* device [T, topk] int32, or NULL */
  const int32_t* cache_seqlens;  /* device [B]: the lengths with the step's rows in the cache */
  const int32_t* cu_seqlens_q;   /* device [B + 1], or NULL: T / B tokens per sequence */
  const int32_t* block_table;    /* device [B, W], or NULL: positions are written as they are */
  int32_t* indices;              /* device [T, topk], written */
  int32_t* topk_lens;            /* device [T], written */
  int64_t row_stride;            /* elements: rows of scores / positions */
  int64_t block_table_stride;    /* elements: rows of block_table */
  int64_t indices_stride;        /* elements: rows of indices (>= topk) */
  int32_t T;                     /* >= 0 */
  int32_t N_or_topk;             /* columns of scores / of positions */
  int32_t topk;
  int32_t B;
  int32_t W;                     /* columns of block_table */
  int32_t page_size;
  int32_t causal;                /* 0 / 1 */
  int32_t reserved2;             /* 0, checked */
} ffpa_mla_sparse_topk_params;

/* Launch the selection on `stream` of the CURRENT device.  Asynchronous; every bad argument returns a status before any device work.  Returns an ffpa_status. */
int ffpa_attn_mla_sparse_topk_slots(const ffpa_mla_sparse_topk_params* p, void* stream);

/*
 * KV-CACHE APPEND + ROTARY (FlashAttention's flash_attn_with_kvcache(k=, v=, rotary_cos=, rotary_sin=)) — the launch that goes in front of the attention
 * launch of a decode / chunked-prefill step.  ONE kernel on `stream`:
 *   * new key i of sequence b (k, v: [batch, seqlen_new, heads_kv, D] by k_stride / v_stride = {batch, row, head}) is written at cache position
 *     pos = max(cache_seqlens[b], 0) + i: row pos of sequence b in a contiguous cache (kv == NULL: k_cache / v_cache [batch, capacity, heads_kv, D] by
 *     k_cache_stride / v_cache_stride = {batch, row, head}), or row pos % page_size of page block_table[b * bt_stride + pos / page_size] of a paged pool (kv != NULL:
 *     the pools of ffpa_attn_varlen_paged_fwd, the batch stride is ignored, pages by kv->k_page_stride / v_page_stride, ids clamped to [0, num_pages)).
 *     A position >= capacity (contiguous: `capacity`; paged: pages_per_row * page_size) is dropped.  Two sequences that append into one shared page race: the
 *     caller's problem, as with FlashAttention.
 *   * rotary_dim > 0: the first rotary_dim dims of the new keys are stored rotated, and q ([batch, seqlen_q, heads_q, D] by q_stride) is written rotated to q_rot
 *     (by q_rot_stride; q is not modified); dims from rotary_dim on are copied; v is never rotated.  Key i sits at position pos, query token i at
 *     max(cache_seqlens[b], 0) + i when causal, at max(cache_seqlens[b], 0) otherwise; positions are clamped to seqlen_ro - 1.  rotary_cos / rotary_sin:
 *     [seqlen_ro, rotary_dim / 2] contiguous in q's dtype; interleaved pairs dims (2j, 2j + 1), else (j, j + rotary_dim / 2) (GPT-NeoX).  fp32 arithmetic
 *     (x cos - y sin, x sin + y cos), one rounding to the dtype.
 *   * seqused[b] = min(max(cache_seqlens[b], 0) + seqlen_new, capacity): the lengths the attention launch that follows reads (its seqused_kv).
 *     cache_seqlens itself is not modified; seqused must be another buffer.
 * Every row moves as 16-byte loads and stores: D, rotary_dim / 2 and every stride are multiples of 8 elements, the bases 16-byte aligned.
 */
typedef struct ffpa_kv_append_params {
  uint32_t struct_size; /* sizeof(ffpa_kv_append_params), checked */
  uint32_t abi_version; /* FFPA_ATTN_ABI_VERSION                   */

  const void* q;          /* [batch, seqlen_q, heads_q, D]; read only with rotary_dim > 0 */
  const void* k;          /* [batch, seqlen_new, heads_kv, D]; may be NULL when seqlen_new == 0 */
  const void* v;
  void* k_cache;          /* written in place */
  void* v_cache;
  void* q_rot;            /* out, [batch, seqlen_q, heads_q, D]: rotated q (rotary_dim > 0 only, else may be NULL) */
  int32_t* seqused;       /* out, device [batch] */
  const int32_t* cache_seqlens; /* device [batch], not modified */
  const void* rotary_cos; /* [seqlen_ro, rotary_dim / 2]; rotary_dim > 0 only */
  const void* rotary_sin;

  int32_t batch;
  int32_t heads_q;
  int32_t heads_kv;
  int32_t head_dim;   /* a multiple of 8 in [8, 1024] */
  int32_t seqlen_q;   /* >= 0 */
  int32_t seqlen_new; /* >= 0; 0 = nothing appended (seqused still written) */
  int32_t capacity;   /* keys a sequence's contiguous cache holds; ignored when paged */
  int32_t seqlen_ro;  /* rows of rotary_cos / rotary_sin (>= the capacity) */

  int64_t q_stride[3];       /* elements: batch, row, head (head-dim stride 1) */
  int64_t k_stride[3];
  int64_t v_stride[3];
  int64_t q_rot_stride[3];
  int64_t k_cache_stride[3]; /* batch (ignored when paged), row, head */
  int64_t v_cache_stride[3];

  int32_t rotary_dim;         /* 0 = no rotary; else a multiple of 16 <= head_dim */
  int32_t rotary_interleaved; /* 1: pairs (2j, 2j + 1); 0: pairs (j, j + rotary_dim / 2) */
  int32_t causal;             /* query positions: see above */
  int32_t dtype;              /* enum ffpa_dtype: q, k, v, the caches, q_rot, cos / sin */
} ffpa_kv_append_params;

/* Launch the append on `stream` of the CURRENT device (kv: the paged pool, NULL = contiguous cache).  Asynchronous: no allocation, no synchronisation; every
 * bad argument returns a status before any device work.  Returns an ffpa_status. */
int ffpa_attn_kvcache_append(const ffpa_kv_append_params* p, const ffpa_paged_kv* kv, void* stream);

/*
 * KV-CACHE APPEND + ROTARY FOR A RAGGED STEP (FlashAttention's flash_attn_varlen_func with seqused_k and block_table, plus its cache append) — the append above
 * for the batch a continuous-batching engine steps with: a prompt chunk, a few speculative verifications and dozens of one-token decodes, packed as token rows.
 * q [total_q, heads_q, D] and k, v [total_q, heads_kv, D] by q_stride / k_stride / v_stride = {row, head} are packed by cu_seqlens_q (device int32
 * [batch + 1], ascending from 0): token row t belongs to the sequence b with cu_seqlens_q[b] <= t < cu_seqlens_q[b + 1], found on the device, as its token
 * i = t - cu_seqlens_q[b].  Empty sequences are legal anywhere; rows from cu_seqlens_q[batch] on (total_q may exceed it) are padding: nothing is written for them.
 * ONE kernel on `stream`:
 *   * key i of sequence b is written at cache position pos = max(cache_seqlens[b], 0) + i — the cache addressing (contiguous or paged, ids clamped, positions at
 *     or past the capacity dropped) is that of the append above; the block table is never read past its row.
 *   * rotary_dim > 0: the first rotary_dim dims of the new keys are stored rotated and q is written rotated to q_rot ([total_q, heads_q, D] by q_rot_stride).
 *     positions == NULL: key i at pos, query token i at pos when causal, at max(cache_seqlens[b], 0) otherwise (the rule above).  positions != NULL (device
 *     int32 [total_q]): the key AND the query token of row t at positions[t] — the key is still written at its slot pos (a tree draft: the position is the
 *     depth, not the slot).  Positions are clamped to [0, seqlen_ro - 1].  The pairing, the arithmetic and the rounding are those of the append above: on a
 *     uniform batch the two calls write the same bytes.
 *   * seqused[b] = min(max(cache_seqlens[b], 0) + (cu_seqlens_q[b + 1] - cu_seqlens_q[b]), capacity) for every b < batch, sequences without a token too.
 */
typedef struct ffpa_kv_append_varlen_params {
  uint32_t struct_size; /* sizeof(ffpa_kv_append_varlen_params), checked */
  uint32_t abi_version; /* FFPA_ATTN_ABI_VERSION                          */

  const void* q;          /* [total_q, heads_q, D]; read only with rotary_dim > 0 */
  const void* k;          /* [total_q, heads_kv, D] */
  const void* v;
  void* k_cache;          /* written in place */
  void* v_cache;
  void* q_rot;            /* out, [total_q, heads_q, D]: rotated q (rotary_dim > 0 only, else may be NULL) */
  int32_t* seqused;       /* out, device [batch] */
  const int32_t* cache_seqlens; /* device [batch], not modified */
  const int32_t* cu_seqlens_q;  /* device [batch + 1] */
  const int32_t* positions;     /* device [total_q] or NULL; read only with rotary_dim > 0 */
  const void* rotary_cos; /* [seqlen_ro, rotary_dim / 2]; rotary_dim > 0 only */
  const void* rotary_sin;

  int32_t batch;
  int32_t heads_q;
  int32_t heads_kv;
  int32_t head_dim;   /* a multiple of 8 in [8, 1024] */
  int32_t total_q;    /* >= 0: token rows of q / k / v (the grid); 0 = only seqused is written */
  int32_t capacity;   /* keys a sequence's contiguous cache holds; ignored when paged */
  int32_t seqlen_ro;  /* rows of rotary_cos / rotary_sin (>= the capacity) */
  int32_t rotary_dim; /* 0 = no rotary; else a multiple of 16 <= head_dim */

  int64_t q_stride[2];       /* elements: row, head (head-dim stride 1) */
  int64_t k_stride[2];
  int64_t v_stride[2];
  int64_t q_rot_stride[2];
  int64_t k_cache_stride[3]; /* batch (ignored when paged), row, head */
  int64_t v_cache_stride[3];

  int32_t rotary_interleaved; /* 1: pairs (2j, 2j + 1); 0: pairs (j, j + rotary_dim / 2) */
  int32_t causal;             /* query positions without `positions`: see above */
  int32_t dtype;              /* enum ffpa_dtype: q, k, v, the caches, q_rot, cos / sin */
  int32_t reserved;           /* 0 */
} ffpa_kv_append_varlen_params;

/* Launch the ragged append on `stream` of the CURRENT device (kv: the paged pool, NULL = contiguous cache [batch, capacity, heads_kv, D]).  Asynchronous: no
 * allocation, no synchronisation; every bad argument returns a status before any device work.  Returns an ffpa_status. */
int ffpa_attn_kvcache_append_varlen(const ffpa_kv_append_varlen_params* p, const ffpa_paged_kv* kv, void* stream);

/*
 * MERGE OF TWO ATTENTION STATES (FlashInfer's / vLLM's merge_attn_states) — the last launch of a cascade (shared-prefix) attention step: two attentions of the
 * same queries over two disjoint key sets, each normalised on its own, combined into the attention over the union.  Per (token t, head h) row, in fp32:
 *     m = max(lse_a, lse_b),  w_x = exp(lse_x - m),  O = (w_a O_a + w_b O_b) / (w_a + w_b),  LSE = m + ln(w_a + w_b)
 * with ONE rounding of O to the dtype.  A side whose LSE is -inf (it saw no key) has weight 0 and its O is not read into the sum (a NaN there does not leak);
 * both sides -inf gives O = 0, LSE = -inf — the packed call's empty-row contract.
 *   * o_a, o_b, o: [tokens, heads, head_dim] by {token, head} element strides (head-dim stride 1), one dtype (bf16 / fp16); head_dim a multiple of 8 in [8, 1024];
 *     every stride a multiple of 8 elements and every base 16-byte aligned (16-byte loads and stores).
 *   * lse_a, lse_b, lse: fp32 [heads, tokens] by a head stride (token stride 1) — the layout ffpa_attn_varlen_fwd stores; natural-log units.  lse may be NULL.
 * The outputs must not overlap the inputs.
 */
typedef struct ffpa_merge_states_params {
  uint32_t struct_size; /* sizeof(ffpa_merge_states_params), checked */
  uint32_t abi_version; /* FFPA_ATTN_ABI_VERSION                      */

  const void* o_a;      /* [tokens, heads, head_dim] */
  const void* o_b;
  void* o;              /* out */
  const float* lse_a;   /* [heads, tokens] fp32 */
  const float* lse_b;
  float* lse;           /* out, may be NULL */

  int32_t tokens;       /* >= 0 (0: nothing to do) */
  int32_t heads;        /* >= 0 (0: nothing to do) */
  int32_t head_dim;     /* a multiple of 8 in [8, 1024] */
  int32_t dtype;        /* enum ffpa_dtype: o_a, o_b, o */

  int64_t o_a_stride[2]; /* elements: token, head */
  int64_t o_b_stride[2];
  int64_t o_stride[2];
  int64_t lse_a_stride_head; /* elements */
  int64_t lse_b_stride_head;
  int64_t lse_stride_head;   /* >= tokens when heads > 1 (rows of the output do not overlap); ignored when lse == NULL */
} ffpa_merge_states_params;

/* Launch the merge on `stream` of the CURRENT device.  Asynchronous: no allocation, no synchronisation; every bad argument returns a status before any device
 * work.  Returns an ffpa_status. */
int ffpa_attn_merge_states(const ffpa_merge_states_params* p, void* stream);

/*
 * PLAN OF A SHARED-PREFIX (CASCADE) STEP OVER THE MLA LATENT CACHE — the one launch between the append and the two attention launches of
 * ffpa_attn_with_kvcache_mla_cascade.  The batch of `batch` sequences (seqlen_q query tokens each) is cut into `groups` groups of consecutive sequences by
 * cu_group_seqs [groups + 1] (non-decreasing, from 0 to batch; an empty group is allowed; NULL: groups must be 1 and the group holds every sequence).  The
 * sequences of a group share their first keys: pages [0, P_g / page_size) of their block-table rows are the same pages, read through the row of the group's
 * FIRST sequence.  With len'_b = clamp(lens[b], 0, capacity) the launch makes, on the device,
 *     P_g = page_size * floor(clamp(min(stated_g, min over b in g of (len'_b - (seqlen_q - 1 if causal else 0))), 0, capacity) / page_size)    (empty group: 0)
 * (stated_g = shared_prefix_len[g], or shared_prefix_len_host for every group when that pointer is NULL) and stores
 *     cu_q_prefix [groups + 1]  = cu_group_seqs * seqlen_q        — the packed queries as `groups` sequences, for the prefix pass
 *     prefix_lens [groups]      = P_g
 *     prefix_table [groups, pages_per_seq] : row g = block_table[first sequence of g] (an empty group: some in-range row)
 *     suffix_table [batch, pages_per_seq]  : [b, j] = block_table[b, min(j + P_g / page_size, pages_per_seq - 1)]
 *     suffix_lens [batch]       = len'_b - P_g
 * Everything is int32 and 4-byte aligned; the outputs are dense and must overlap neither the inputs nor one another (FFPA_ERR_BAD_SHAPE).  No atomics, no
 * workspace.  A cu_group_seqs that breaks its contract gives unspecified values, never an access outside the arrays.
 */
typedef struct ffpa_mla_cascade_plan_params {
  uint32_t struct_size; /* sizeof(ffpa_mla_cascade_plan_params), checked */
  uint32_t abi_version; /* FFPA_ATTN_ABI_VERSION                          */

  const int32_t* cu_group_seqs;     /* [groups + 1], or NULL (groups == 1) */
  const int32_t* shared_prefix_len; /* [groups] on the device, or NULL: shared_prefix_len_host */
  const int32_t* lens;              /* [batch]: the keys every sequence holds (after the step's append), not clamped */
  const int32_t* block_table;       /* [batch, pages_per_seq] by bt_stride, column stride 1 */
  int32_t* cu_q_prefix;             /* out [groups + 1] */
  int32_t* prefix_lens;             /* out [groups] */
  int32_t* prefix_table;            /* out [groups, pages_per_seq] */
  int32_t* suffix_table;            /* out [batch, pages_per_seq] */
  int32_t* suffix_lens;             /* out [batch] */

  int64_t bt_stride;                /* elements between rows of block_table, >= pages_per_seq when batch > 1 */
  int32_t batch;                    /* >= 1 */
  int32_t groups;                   /* >= 1 */
  int32_t pages_per_seq;            /* >= 1 */
  int32_t page_size;                /* a positive multiple of 64 */
  int32_t seqlen_q;                 /* >= 1, batch * seqlen_q < 2^31 */
  int32_t causal;                   /* 0 / 1 */
  int32_t capacity;                 /* keys a sequence can hold: in (0, pages_per_seq * page_size] */
  int32_t shared_prefix_len_host;   /* >= 0; read when shared_prefix_len == NULL */
} ffpa_mla_cascade_plan_params;

/* Launch the plan on `stream` of the CURRENT device.  Asynchronous: no allocation, no synchronisation; every bad argument returns a status before any device
 * work.  Returns an ffpa_status. */
int ffpa_attn_mla_cascade_plan(const ffpa_mla_cascade_plan_params* p, void* stream);

/* Capability / build queries.  Replaces the module attributes
 * CUDA_FWD_AVAILABLE, F16_ACC_AVAILABLE, ... (csrc/cuffpa/ffpa_api.cc:283-305). */
enum ffpa_query {
  FFPA_QUERY_ABI_VERSION = 0,
  FFPA_QUERY_FWD_AVAILABLE = 1,   /* 1 if the gfx950 kernels are in this build */
  FFPA_QUERY_MIN_HEAD_DIM = 2,    /* 8    */
  FFPA_QUERY_MAX_HEAD_DIM = 3,    /* 1024 */
  FFPA_QUERY_HEAD_DIM_MULTIPLE = 4, /* 8: kernels are built per multiple of 64; a head dim in between runs on the next one with
                                       the missing columns read as zeros in-kernel (no padded copies) */
  FFPA_QUERY_FP16_AVAILABLE = 5,
  FFPA_QUERY_DROPOUT_AVAILABLE = 6,
  FFPA_QUERY_DEBUG_KERNELS = 7,   /* 1 if FFPA_FLAG_DEBUG_SAFE_PATH kernels are built: only in the test-only twin library
                                     libffpa_attn_hip_test.so, never in the product library */
  /* what the launch plan's pricing reads from the CURRENT device (MI355X figures without one): the split rules are priced per device,
     not per SKU constant */
  FFPA_QUERY_DEVICE_CUS = 8,        /* compute units */
  FFPA_QUERY_DEVICE_CLOCK_MHZ = 9,  /* engine clock */
  FFPA_QUERY_DEVICE_HBM_GBPS = 10,  /* HBM peak (4 transfers x memory clock x bus width: HBM3 / HBM3E) */
  FFPA_QUERY_VARLEN_AVAILABLE = 11  /* 1 if ffpa_attn_varlen_fwd's kernels are in this build */
};
int ffpa_attn_query(int what);

/* Tile geometry the kernel uses for a head dim (for benches / roofline maths).
 * Returns 0 and fills rows-per-workgroup / keys-per-tile / dynamic LDS bytes,
 * or FFPA_ERR_BAD_HEADDIM. */
int ffpa_attn_fwd_tile_config(int head_dim, int* block_rows, int* block_keys,
                              int* lds_bytes);

/* Human-readable text for the last non-zero status on this thread. */
const char* ffpa_attn_last_error(void);

/* "ffpa-attn-amd <semver> gfx950" */
const char* ffpa_attn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FFPA_ATTN_H_ */
