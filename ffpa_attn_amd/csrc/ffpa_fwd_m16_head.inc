// ffpa_fwd_m16_head.inc — the compile-time geometry and the per-lane identities of ffpa_fwd_m16_kernel / ffpa_fwd_m16_pair_kernel (included into both bodies:
// ffpa_fwd_m16_kernel.h; T, D, MK, DROP and the FwdArgs `a` are the enclosing kernel's).  Text moved out of the kernel, nothing changed.
  static_assert(MK >= 0 && MK <= 3 && (!DROP || MK <= 1), "mask kinds 0 ... 3; dropout builds: MK = 0 (no bias) and MK = 1 (any bias or mask)");
  constexpr bool MASK = MK == 1 || MK == 2;  // builds that honour mask ranges (kv_bounds)
  constexpr bool kBias = MK == 1 || MK == 3;  // builds whose S^T accumulators start from bias / scale
  using E = Elem<T>;
  using M = FFPA_M16_MFMA;
  using v8 = typename E::v8;
  using v4 = typename E::v4;
  static_assert(D % 64 == 0 && D <= 1024, "O^T (D / ND / 2 registers per lane) must fit the AGPRs");
  // D > 512: the head dim is split over two waves (ND = 2, as in ffpa_fwd_split_d_kernel): wave (qb, dh) = (wave / 2, wave % 2) owns rows
  // 32 qb .. + 32 and columns dh * D/2 .. of both contractions; the two partial S^T tiles of a row block are summed through LDS.
  constexpr int ND = (D <= 512) ? 1 : 2;
  constexpr int DW = D / ND;    // columns owned by one wave
#ifdef FFPA_M16_PAGED
  constexpr int BC = m16_block_keys(D, true), BR = 128 / ND;  // (the paged kernel: 64-key tiles at D = 256 / 320 too — a 64-key page holds a whole tile)
#else
  constexpr int BC = m16_block_keys(D, kBias), BR = 128 / ND;
#endif
  constexpr int KS = DW / 32;   // QK contraction steps per wave
  constexpr int NKB = BC / 16;  // 16-key S^T blocks per tile
  constexpr int NKS = BC / 32;  // PV contraction steps per tile
  constexpr int NDB = DW / 16;  // 16-column O^T blocks per wave
  constexpr int RB = D * 2;
  constexpr int TILE = BC * RB;
  constexpr int PPW = BC * D * 2 / 4096;  // 1 KiB DMA pieces per wave per tile
  // D = 512 with masks: a tile row is one whole piece -> wave-uniform rows, scalar addressing (the per-lane offset tables of the other form
  // would not fit next to the mask path's registers).  Everything else keeps tile-invariant per-lane offsets in registers: measured equal
  // or better (D = 512 unmasked: + 0 ... 2 %; D = 1024: 927 vs 776 TFLOPS — the scalar row form loses 16 % there on this build).
  constexpr bool kRowDma = RB % 1024 == 0 && ND == 1 && (MK == 1 || MK == 2 || DROP);
  static_assert(!kRowDma || RB == 1024, "the scalar row form is used where a tile row is exactly one piece");
  constexpr int KPW = BC / 4;                // keys staged per wave per tile
  constexpr int PF1 = FFPA_M16_PF1, PF2 = FFPA_M16_PF2;
  constexpr int kPreReq = ND == 2 ? FFPA_M16_K_PRE_ND2 : FFPA_M16_K_PRE;
  constexpr int kPre = ((kPreReq < PPW ? kPreReq : PPW) / 4) * 4;
  constexpr int N1 = KS * NKB;   // K fragments per tile
  constexpr int N2 = NDB * NKS;  // V^T fragments per tile
  // the softmax pipeline of the split-D tiles (header comment above the FFPA_M16_PP_* piece counts): needs an even number of pieces per wave (D % 128 == 0), and it stages K as two
  // 16-key halves — piece i < kH of a wave belongs to K1 (keys 0 .. 15), the rest to K2
  constexpr bool kPipe = ND == 2 && PPW % 2 == 0 && NKB == 2 && (MK == 0 || MK == 2 || MK == 3) && !DROP;
  constexpr bool kKS = kPipe;  // the two-half K piece map
  constexpr int kH = PPW / 2;  // K1 / K2 pieces per wave
  constexpr int ppVQ = PPW * FFPA_M16_PP_VQ / 16, ppVS = PPW - ppVQ;     // V(j): in Q(j), in S(j)
  constexpr int ppK1Q = PPW * FFPA_M16_PP_K1Q / 16, ppK1P = kH - ppK1Q;  // K1(j+1): in P(j-1) (first), in Q(j) (rest)
  constexpr int ppK2S = PPW * FFPA_M16_PP_K2S / 16, ppK2P = kH - ppK2S;  // K2(j+1): in S(j) (first), in P(j) (rest)
  static_assert(!kPipe || (ppVQ >= 0 && ppVS >= 0 && ppK1Q >= 0 && ppK1P >= 0 && ppK2S >= 0 && ppK2P >= 0), "piece counts per phase");
  static_assert(!kPipe || (ppVQ + ppK1Q <= KS && ppVS + ppK2S <= KS && ppK2P + ppK1P <= N2), "at most one piece per fragment");
  // (a step that walks past the phase's last fragment would silently drop the pieces behind it: a tile image with stale rows)
  static_assert(!kPipe || ((ppVQ + ppK1Q - 1) * FFPA_M16_PP_QSTEP < KS && (ppVS + ppK2S - 1) * FFPA_M16_PP_SSTEP < KS && (ppK2P + ppK1P - 1) * FFPA_M16_PP_PSTEP < N2),
                "every piece of a phase must ride on one of its fragments");
  // counted waits: order of issue inside a step — Q: K1 rest, V first; S: V rest, K2 first; P: K2 rest, K1 first (of the tile after next), touch
  constexpr int ppWaitA1 = ppVQ + (ppK1Q > 0 ? 0 : 0);  // K1(j+1) has landed: the V pieces of Q(j) stay in flight (+ the touch when K1Q == 0)
  constexpr int ppWaitA2 = ppK2S;                       // V(j) has landed
  constexpr int ppWaitB = ppK1P;                        // K2(j+1) has landed (+ the touch)
  constexpr int kStep1 = N1 / PPW > 0 ? N1 / PPW : 1;  // one V piece every this many K fragments
  constexpr int kStep2 = N2 / PPW > 0 ? N2 / PPW : 1;  // one K piece every this many V^T fragments
  static_assert(kStep1 >= 1 && kStep2 >= 1 && N1 % PPW == 0 && N2 % PPW == 0, "DMA pieces must fit the MFMA loops");
  constexpr int NH = BC > 64 ? BC / 64 : 1;         // 64-key halves of a tile (ds_read immediates are 16 bits: one address base per half)
  constexpr int KV = (D % 128 == 0) ? 4 : 2;        // K fragment address variants: the swizzle reaches slot bits 0 .. 3 / 0 .. 2
  constexpr int KVB = (D % 128 == 0) ? 256 : 128;   //   and the bytes KV contraction steps advance
  constexpr int VV = (D % 128 == 0) ? 8 : 4;        // V^T fragment address variants
  constexpr int VVB = (D % 128 == 0) ? 256 : 128;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  FFPA_LDS char* const Kt = (FFPA_LDS char*)smem;
  FFPA_LDS char* const Vt = Kt + TILE;
  FFPA_LDS char* const Xb = Kt + 2 * TILE;  // ND == 2: partial-S exchange, 4 KiB per wave (6 KiB in the builds without an additive bias)
  FFPA_LDS char* const Bl = Kt + 2 * TILE + m16_exchange_bytes(D, MK);  // key-bias row cache (FwdArgs.bias_lds bytes, when enabled)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = lane & 15;
  const int c = lane >> 4;
  const int qb = wave / ND;  // row block of this wave
  const int dh = wave % ND;  // which D / ND slice of the head dim it owns

