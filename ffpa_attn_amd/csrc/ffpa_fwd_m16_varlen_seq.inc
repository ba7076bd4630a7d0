// ffpa_fwd_m16_varlen_seq.inc — the sequence lookup of the packed-sequence kernels (ffpa_fwd_m16_varlen_kernel, ffpa_fwd_m16_kernel.h; its paged twin
// ffpa_fwd_m16_paged_kernel, ffpa_paged_inst.hip): workgroup -> (KV range, sequence, row tile, head), the sequence's FwdArgs `a` and its KV split.  Text moved out
// of the kernel, nothing changed; FFPA_M16_VARLEN_WINDOW (a constant of the enclosing kernel's build) = a sliding window: `right` joins the causal offset and the KV
// ranges share out the tiles from the window's first one on; under FFPA_M16_PAGED the keys' length is seqused_k's (clamped to the block table's row) and K / V keep the pool's base.
  int vid = blockIdx.x;
  if (!(a_in.flags & kFlagNoXcdRemap)) vid = xcd_logical_id(vid, gridDim.x, a_in.xcd_group);
  int split = 0;
  if (a_in.nsplit > 1) {  // (the KV ranges of a pair are neighbours in the launch order: one XCD, one after the other)
    const int pair = vid / a_in.nsplit;
    split = vid - pair * a_in.nsplit;
    vid = pair;
  }
  // Order of the (sequence, head) pairs: head CHUNK-major, then sequence, then the head inside its chunk (va.head_chunk consecutive heads: Hq / 8 when that is
  // whole, else 1).  The XCD remap hands every XCD a contiguous range of pairs (all row tiles of a pair on one XCD: its K / V stream stays in one L2), and
  // sequences differ in length by orders of magnitude — sequence-major (the dense order) gives one XCD the longest sequence and another the shortest (measured:
  // 400 vs 960 TFLOPS on the bench's 256 ... 4864-token batch).  Chunk-major gives every XCD the same heads of EVERY sequence; and the heads of a chunk — under
  // GQA heads of ONE KV group — walk the same sequence side by side, so that the group's K / V stream is fetched once per L2, not once per head
  // ... side by side at the level of ROW TILES: (chunk, sequence, row tile, head in chunk) — a head's tiles alone fill an XCD's 32 CUs for a whole round, so heads
  // that merely follow each other stream the sequence's K / V once each (measured: no fewer HBM bytes than head-major order); interleaved per tile, the same row
  // tile of the chunk's heads runs at the same time on the same keys
  int chunk, seq, qt, head_in_chunk;
  int seq_tiles = a_in.nqt;  // row tiles of this sequence in the grid (compact grid: the sequence's own count)
  if (va.compact_tiles > 0) {
    const int per_chunk = va.compact_tiles * va.head_chunk;
    chunk = vid / per_chunk;
    const int in_chunk = vid - chunk * per_chunk;
    const int slot = in_chunk / va.head_chunk;
    head_in_chunk = in_chunk - slot * va.head_chunk;
    // slot -> (sequence, row tile): the sequences' tile counts, 64 sequences per step
    seq = -1, qt = 0;
    int before = 0;
    for (int s0 = 0; s0 < a_in.B; s0 += 64) {
      const int i = s0 + lane;
      int n = 0;
      if (i < a_in.B) {
        const int len = va.cu_q[i + 1] - va.cu_q[i];
#ifdef FFPA_M16_MLA_ON
        // (the latent-cache build, ffpa_mla_inst.hip: the row tiles of a packed launch are the chunks of the sequence's pack x len rows — the count the row test
        // below and the causal reversal use; a preprocessor test, so that every other kernel's text is what it was)
        const int rows = va.pack ? va.pack * len : len;
        n = rows > 0 ? (rows + BR - 1) / BR : 0;
#else
        n = len > 0 ? (len + BR - 1) / BR : 0;
#endif
      }
      int incl = n;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
      }
      const int total = __shfl(incl, 63);
      if (slot < before + total) {
        const unsigned long long m = __ballot(slot < before + incl);
        const int l = __ffsll((long long)m) - 1;
        seq = s0 + l;
        seq_tiles = __shfl(n, l);
        qt = slot - (before + __shfl(incl, l) - seq_tiles);
        break;
      }
      before += total;
    }
    if (seq < 0) return;  // (a slot past the batch's last row tile: the bound is not tight)
    seq = __builtin_amdgcn_readfirstlane(seq);
    seq_tiles = __builtin_amdgcn_readfirstlane(seq_tiles);
    qt = __builtin_amdgcn_readfirstlane(qt);
  } else {
    const int per_seq = a_in.nqt * va.head_chunk, per_chunk = a_in.B * per_seq;
    chunk = vid / per_chunk;
    const int in_chunk = vid - chunk * per_chunk;
    seq = in_chunk / per_seq;
    const int in_seq = in_chunk - seq * per_seq;
    qt = in_seq / va.head_chunk;
    head_in_chunk = in_seq - qt * va.head_chunk;
  }
  if (a_in.causal) qt = seq_tiles - 1 - qt;  // longest rows first
  const int bh = seq * a_in.Hq + chunk * va.head_chunk + head_in_chunk;
  FwdArgs a = a_in;
  int q_lo;  // packed: the sequence's first row of q / o (LSE [Hq, T_q]: its column); dense: the batch element's first LSE row
  int ntok = 1;  // tokens of this sequence (>= 1): packed rows are (row / ntok, row % ntok) = (head of the group, token)
  if (va.cu_q == nullptr) {
    // DENSE launches in this kernel's workgroup order (ffpa_attn_fwd -> ffpa_capi.hip: causal + GQA, no bias, no dropout, every row sees a key): the
    // arguments are the dense call's as they are — "sequence" = batch element, batch strides live —, only the order of the workgroups is this kernel's
    q_lo = seq * a_in.Hq * a_in.Nq;
    // (KV ranges in this mode: a causal launch of one round of workgroups whose long row tiles would run alone at the end — ffpa_capi.hip pick_tile_ranges; the
    // workspace rows are the dense call's [split, batch, head, row]: ws_head_rows = Nq, ws_split_rows = B x Hq x Nq, merged by ffpa_fwd_merge_kernel)
  } else {
    q_lo = va.cu_q[seq];
#ifndef FFPA_M16_PAGED
    const int k_lo = va.cu_k[seq];
    const int ntok_seq = va.cu_q[seq + 1] - q_lo;
    int nkv_seq = va.cu_k[seq + 1] - k_lo;
    if (va.used_k != nullptr) {
      const int used = va.used_k[seq];
      nkv_seq = nkv_seq < used ? nkv_seq : used;
    }
#else
    // (paged: the lengths are seqused_k's, clamped to what the sequence's row of the block table can hold; no contiguous key range)
    const int ntok_seq = va.cu_q[seq + 1] - q_lo;
#if FFPA_M16_KV_GATHER
    // (gathered keys, ffpa_mla_sparse_inst.hip: the token's count of valid entries; no counts = every entry of its row; a preprocessor test, so that every other
    // kernel's text is what it was)
    int nkv_seq = va.used_k != nullptr ? va.used_k[seq] : pa.cap;
#else
    int nkv_seq = va.used_k[seq];
#endif
    nkv_seq = nkv_seq < pa.cap ? nkv_seq : pa.cap;
#endif
    ntok = ntok_seq > 0 ? ntok_seq : 1;
    const int nq_seq = va.pack ? va.pack * ntok_seq : ntok_seq;  // (packed: the rows of a sequence are (head of the group, token), head-major)
    if (qt * BR >= nq_seq) return;  // (max_seqlen_q sized the grid: this sequence is shorter)
    // (batch strides are zero: the launch side)
    a.Nq = nq_seq;
    a.Nkv = nkv_seq > 0 ? nkv_seq : 0;
    a.causal_offset = a.Nkv - ntok_seq;  // (tail-aligned per sequence; a single packed token runs without the causal flag — it sees every key of its sequence)
    if (FFPA_M16_VARLEN_WINDOW) a.causal_offset += va.win_right;  // (a sliding window's `right` rides in the causal limit: VarlenArgs::window)
    if (va.pack) a.causal_row_mod = ntok_seq;
    if (a_in.nsplit > 1 && (int64_t)q_lo + ntok_seq > va.ws_head_rows) return;  // (a caller whose total_q is smaller than its boundaries say: nothing is stored outside the scratch it sized)
    a.q = (const T*)a_in.q + (int64_t)q_lo * va.q_tok_stride;
    a.o = (T*)a_in.o + (int64_t)q_lo * va.o_tok_stride;
#ifndef FFPA_M16_PAGED
    a.k = (const T*)a_in.k + (int64_t)k_lo * a_in.sk[2];
    a.v = (const T*)a_in.v + (int64_t)k_lo * a_in.sv[2];
#endif
  }
  if (a_in.nsplit > 1) {
    int tiles = (a.Nkv + BC - 1) / BC;
    if (a.causal) {
      // under the causal flag a row tile walks the KV tiles up to ITS diagonal (the tile text's clamp, restated): those are what its ranges share out —
      // every row tile of an under-filled prefill launch splits its own visible keys evenly (one-row-tile launches: all keys of the sequence, as before)
      const int last_row = a.causal_row_mod ? a.causal_row_mod - 1 : qt * BR + BR - 1;
      const int64_t last = (int64_t)last_row + a.causal_offset;
      const int ntc = last < 0 ? 0 : (int)(last / BC) + 1;
      tiles = tiles < ntc ? tiles : ntc;
    }
    if (FFPA_M16_VARLEN_WINDOW) {
      // under a sliding window the row tile's walk starts at the tile of its first row's left bound (the tile text, restated): the ranges share out [t_lo, tiles)
      tiles -= m16_window_first_tile(a.causal_row_mod ? 0 : qt * BR, a.causal_offset, va.win_span, BC);
      tiles = tiles > 0 ? tiles : 0;
    }
    a.tiles_per_split = (tiles + a_in.nsplit - 1) / a_in.nsplit;  // (fewer tiles than ranges leaves ranges empty: dead partials, weight 0 in the merge)
  }
