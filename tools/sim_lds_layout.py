"""Host-side simulation of the kernel's LDS addressing (developer tool).

Re-derives, in plain Python, where the LDS-DMA puts every 16-byte slot of a K / V tile and which
bytes each lane's ds_read_b128 / ds_read_b64_tr_b16 touches, and checks that
  * K fragment (lane l, step s, key block kb) = K[kb*32 + pi(l%32)][dh*DW + 16 s + 8 (l/32) .. +8] with
    pi(a) = 16 (a/4 % 2) + a%4 + 4 (a/8): MFMA row a of S^T = K.Q^T is fed key pi(a), so that the C layout
    (row (r&3) + 8 (r>>2) + 4 (l/32) in register r) hands lane half h = l/32 the 16 CONTIGUOUS keys 16 h + r
  * V^T fragment (lane l, column block db, step ks, element jj) =
        V[32 (ks/2) + 16 (l/32) + 8 (ks%2) + jj][dh*DW + 32 db + l%32]   (the same key <-> slot map)
    under the transpose-read rule  result[lane i][e] = data of lane 4e + i/4, element i%4
    (cdna_hip_programming.md §2 "ds_read_b64_tr_b16")
and reports the worst bank conflict per LDS instruction group (MI355X_MICROARCH.md §LDS).
"""
import sys


def k_sw(D, key):
  return (key & 15) if D % 128 == 0 else ((key >> 1) & 7)


def v_sw(D, key):
  return ((key & 3) << 2) if D % 128 == 0 else (((key >> 1) & 1) << 2)


def pi(a):
  return 16 * ((a >> 2) & 1) + (a & 3) + 4 * (a >> 3)


def check(D, ND=None):
  ND = ND or (1 if D <= 512 else 2)
  DW, BC = D // ND, ((128 if D <= 320 else 64) if ND == 1 else 32)
  RB, SPR = D * 2, D // 8
  PIECES = BC * D * 2 // 1024
  PPW = PIECES // 4
  # ---- DMA image: lds[slot index] = (key, source slot)
  for is_v in (False, True):
    lds = {}
    for wave in range(4):
      for i in range(PPW):
        p = wave * PPW + i
        for lane in range(64):
          if (D * 2) % 1024 == 0:
            RPP = D * 2 // 1024
            key = p // RPP
            sw = v_sw(D, key) if is_v else k_sw(D, key)
            src_byte = ((lane ^ sw) << 4) + (p % RPP) * 1024
          else:
            g = p * 64 + lane
            key, slot = divmod(g, SPR)
            src_byte = (slot ^ (v_sw(D, key) if is_v else k_sw(D, key))) << 4
          assert 0 <= src_byte < RB, (D, is_v, src_byte)
          dst = p * 1024 + lane * 16
          assert dst not in lds
          lds[dst] = (key, src_byte)
    assert len(lds) == BC * RB // 16
    img = {}  # lds byte -> (key, source byte) at 2-byte granularity
    for dst, (key, sb) in lds.items():
      for b in range(0, 16, 2):
        img[dst + b] = (key, sb + b)
    if not is_v:
      kimg = img
    else:
      vimg = img
  worst_k = worst_v = 1
  for dh in range(ND):
    # ---- K fragments
    for kb in range(BC // 32):
      for s in range(DW // 16):
        addrs = []
        for lane in range(64):
          l31, h = lane & 31, lane >> 5
          kx = k_sw(D, pi(l31))
          c0 = dh * (DW // 8)
          kaddr = pi(l31) * RB + (((c0 + 2 * (s & 7) + h) ^ kx) << 4)
          a = kaddr + (s >> 3) * 256 + kb * 32 * RB
          addrs.append(a)
          for e in range(8):
            key, sb = kimg[a + 2 * e]
            assert key == kb * 32 + pi(l31) and sb == (dh * DW + 16 * s + 8 * h + e) * 2, (D, lane, s, kb, e, key, sb)
        # ds_read_b128: 4 groups of 16 lanes, bank = (a/4) % 64, 4 dwords each
        for grp in ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
                    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]):
          for half in (0, 32):
            banks = {}
            for l in grp:
              banks.setdefault((addrs[l + half] // 16) % 16, set()).add(addrs[l + half])
            worst_k = max(worst_k, max(len(v) for v in banks.values()))
    # ---- V^T fragments
    for db in range(DW // 32):
      for ks in range(BC // 16):
        for hh in range(2):
          lane_addr = []
          for lane in range(64):
            h, j4 = lane >> 5, (lane & 15) >> 2
            vsw = v_sw(D, j4) * 16
            vcol = dh * DW * 2 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8
            vaddr = (16 * h + j4) * RB + ((vcol + (db & 3) * 64) ^ vsw)
            lane_addr.append(vaddr + (db >> 2) * 256 + (32 * (ks >> 1) + 8 * (ks & 1) + 4 * hh) * RB)
          for lane in range(64):
            l31, h = lane & 31, lane >> 5
            i, base = lane & 15, lane & ~15
            for e in range(4):
              src_lane = base + 4 * e + (i >> 2)
              key, sb = vimg[lane_addr[src_lane] + 2 * (i & 3)]
              jj = 4 * hh + e
              want_key = 32 * (ks >> 1) + 16 * h + 8 * (ks & 1) + jj
              want_col = dh * DW + db * 32 + l31
              assert (key, sb) == (want_key, want_col * 2), (D, lane, db, ks, hh, e, key, sb, want_key, want_col)
          # ds_read_b64_tr_b16: 2 groups of 32 lanes, bank = (a/4) % 64, 2 dwords each
          for half in (0, 32):
            banks = {}
            for l in range(32):
              a = lane_addr[l + half]
              banks.setdefault((a // 8) % 32, set()).add(a)
            worst_v = max(worst_v, max(len(v) for v in banks.values()))
  print(f"D={D:5d} ND={ND} BC={BC}: K/V fragment maps OK; worst bank conflict: ds_read_b128 {worst_k}-way, tr_b16 {worst_v}-way")
  return worst_k, worst_v


def m16_k_sw(D, key):
  return (key & 15) if D % 128 == 0 else ((key >> 1) & 7)


def m16_v_sw(D, key):
  return ((key & 7) << 1) if D % 128 == 0 else (((key >> 1) & 3) << 1)


def check_m16(D):
  """The 16x16x32-MFMA build (csrc/ffpa_fwd_m16_kernel.h); wave (qb, dh) owns columns dh * DW .. + DW (DW = D for D <= 512, D / 2 above):
    K fragment (lane l, step s, 16-key block kb) = K[16 kb + l % 16][dh DW + 32 s + 8 (l / 16) .. + 8]
    V^T fragment (lane l, column block db, key step ks, element e) = V[32 ks + 16 (e / 4) + 4 (l / 16) + e % 4][dh DW + 16 db + l % 16]
  and both instruction groups conflict-free."""
  ND = 1 if D <= 512 else 2
  DW = D // ND
  BC = 32 if ND == 2 else (128 if D <= 320 else 64)
  RB, SPR = D * 2, D // 8
  PPW = BC * D * 2 // 4096
  row_dma = RB % 1024 == 0
  RPP = RB // 1024 if row_dma else 1
  imgs = []
  for is_v in (False, True):
    sw = m16_v_sw if is_v else m16_k_sw
    img = {}
    for wave in range(4):
      for i in range(PPW):
        for lane in range(64):
          if row_dma:
            jk, half = divmod(i, RPP)
            key = 16 * (jk >> 2) + 4 * wave + (jk & 3)
            src = ((lane ^ sw(D, 4 * wave + (jk & 3))) << 4) + half * 1024
            assert sw(D, key) == sw(D, 4 * wave + (jk & 3))
            dst = key * RB + half * 1024 + lane * 16
          else:
            g = (wave * PPW + i) * 64 + lane
            key, slot = divmod(g, SPR)
            src = (slot ^ sw(D, key)) << 4
            dst = (wave * PPW + i) * 1024 + lane * 16
          assert 0 <= src < RB and key < BC, (D, is_v, key, src)
          for b in range(0, 16, 2):
            assert dst + b not in img
            img[dst + b] = (key, src + b)
    assert len(img) == BC * RB // 2
    imgs.append(img)
  kimg, vimg = imgs
  KV, KVB = (4, 256) if D % 128 == 0 else (2, 128)
  VV, VVB = (8, 256) if D % 128 == 0 else (4, 128)
  worst_k = worst_v = 1
  for dh in range(ND):
    c0 = dh * (DW // 8)
    for kb in range(BC // 16):
      for s in range(DW // 32):
        addrs = []
        for lane in range(64):
          n, c = lane & 15, lane >> 4
          base = (64 * (kb // 4) + n) * RB + (((c0 + 4 * (s % KV) + c) ^ m16_k_sw(D, n)) << 4)
          a = base + (s // KV) * KVB + (kb % 4) * 16 * RB
          assert (s // KV) * KVB + (kb % 4) * 16 * RB < 65536
          addrs.append(a)
          for e in range(8):
            assert kimg[a + 2 * e] == (16 * kb + n, (dh * DW + 32 * s + 8 * c + e) * 2), (D, lane, s, kb, e)
        for grp in ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]):
          for half in (0, 32):
            banks = {}
            for l in grp:
              banks.setdefault((addrs[l + half] // 16) % 16, set()).add(addrs[l + half])
            worst_k = max(worst_k, max(len(v) for v in banks.values()))
    for db in range(DW // 16):
      for ks in range(BC // 32):
        for second in (0, 1):
          la = []
          for lane in range(64):
            n, c = lane & 15, lane >> 4
            vkey = 4 * c + (n >> 2)
            base = (64 * (ks // 2) + vkey) * RB + (((c0 + 2 * (db % VV) + ((n & 3) >> 1)) ^ m16_v_sw(D, vkey)) << 4) + 8 * (n & 1)
            off = (db // VV) * VVB + ((ks % 2) * 32 + 16 * second) * RB
            assert off < 65536
            la.append(base + off)
          for lane in range(64):
            i, base_lane, c = lane & 15, lane & ~15, lane >> 4
            for e in range(4):
              src_lane = base_lane + 4 * e + (i >> 2)
              got = vimg[la[src_lane] + 2 * (i & 3)]
              want = (32 * ks + 16 * second + 4 * c + e, (dh * DW + 16 * db + i) * 2)
              assert got == want, (D, lane, db, ks, second, e, got, want)
          for half in (0, 32):
            banks = {}
            for l in range(32):
              banks.setdefault((la[l + half] // 8) % 32, set()).add(la[l + half])
            worst_v = max(worst_v, max(len(v) for v in banks.values()))
  print(f"D={D:5d} 16x16x32 build ND={ND} BC={BC}: K/V fragment maps OK; worst bank conflict: ds_read_b128 {worst_k}-way, tr_b16 {worst_v}-way")
  return worst_k, worst_v


def mla_sw(D, key):
  """The source-side swizzle of the SHARED image of the MLA build (csrc/ffpa_fwd_m16_tile.inc under FFPA_M16_MLA_ON): the V map of the 16x16x32 build."""
  return m16_v_sw(D, key)


# What the shared image can be swizzled with: the two maps the K and V images of the 16x16x32 build use today, and no swizzle at all.
MLA_CANDIDATES = {"k map": m16_k_sw, "v map": m16_v_sw, "none": lambda D, key: 0}


def check_m16_shared(D=576, sw=None, quiet=False):
  """The MLA build's ONE latent tile image (D % 128 == 64, D > 512: 32-key tiles, D split over two waves): both products read the image the DMA wrote once —
    K fragment (lane l, step s, 16-key block kb) = L[16 kb + l % 16][dh DW + 32 s + 8 (l / 16) .. + 8]                       (ds_read_b128)
    V^T fragment (lane l, column block db, element e) = L[16 (e / 4) + 4 (l / 16) + e % 4][dh DW + 16 db + l % 16]           (two ds_read_b64_tr_b16)
  against ONE source-side swizzle ``sw(D, key)`` (default: ``mla_sw``).  Replays every ds_read_b128 16-lane group and every transpose-read 32-lane half under the
  bank rule of ``check_m16`` -> (worst K conflict, worst V^T conflict, K conflict cycles, V^T conflict cycles): ways of the worst group (1 = conflict-free) and
  the extra cycles summed over all groups of one tile (a group of m-way conflict costs m - 1)."""
  sw = sw or mla_sw
  assert D > 512 and D % 128 == 64, "the MLA hook lives in the un-pipelined split-D loop"
  ND, BC = 2, 32
  DW = D // ND
  RB, SPR = D * 2, D // 8
  PPW = BC * D * 2 // 4096
  img = {}
  for wave in range(4):
    for i in range(PPW):
      for lane in range(64):
        g = (wave * PPW + i) * 64 + lane
        key, slot = divmod(g, SPR)
        src = (slot ^ sw(D, key)) << 4
        dst = (wave * PPW + i) * 1024 + lane * 16
        assert 0 <= src < RB and key < BC, (D, key, src)
        for b in range(0, 16, 2):
          assert dst + b not in img
          img[dst + b] = (key, src + b)
  assert len(img) == BC * RB // 2
  KV, KVB, VV, VVB = 2, 128, 4, 128
  worst_k = worst_v = 1
  cyc_k = cyc_v = 0
  for dh in range(ND):
    c0 = dh * (DW // 8)
    for kb in range(BC // 16):
      for s in range(DW // 32):
        addrs = []
        for lane in range(64):
          n, c = lane & 15, lane >> 4
          a = n * RB + (((c0 + 4 * (s % KV) + c) ^ sw(D, n)) << 4) + (s // KV) * KVB + kb * 16 * RB
          addrs.append(a)
          for e in range(8):
            assert img[a + 2 * e] == (16 * kb + n, (dh * DW + 32 * s + 8 * c + e) * 2), (D, lane, s, kb, e)
        for grp in ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]):
          for half in (0, 32):
            banks = {}
            for l in grp:
              banks.setdefault((addrs[l + half] // 16) % 16, set()).add(addrs[l + half])
            m = max(len(v) for v in banks.values())
            worst_k, cyc_k = max(worst_k, m), cyc_k + m - 1
    for db in range(DW // 16):
      for second in (0, 1):
        la = []
        for lane in range(64):
          n, c = lane & 15, lane >> 4
          vkey = 4 * c + (n >> 2)
          la.append(vkey * RB + (((c0 + 2 * (db % VV) + ((n & 3) >> 1)) ^ sw(D, vkey)) << 4) + 8 * (n & 1) + (db // VV) * VVB + 16 * second * RB)
        for lane in range(64):
          i, base_lane, c = lane & 15, lane & ~15, lane >> 4
          for e in range(4):
            got = img[la[base_lane + 4 * e + (i >> 2)] + 2 * (i & 3)]
            want = (16 * second + 4 * c + e, (dh * DW + 16 * db + i) * 2)
            assert got == want, (D, lane, db, second, e, got, want)
        for half in (0, 32):
          banks = {}
          for l in range(32):
            banks.setdefault((la[l + half] // 8) % 32, set()).add(la[l + half])
          m = max(len(v) for v in banks.values())
          worst_v, cyc_v = max(worst_v, m), cyc_v + m - 1
  if not quiet:
    print(f"D={D:5d} MLA shared image ND={ND} BC={BC}: K/V fragment maps OK; worst bank conflict: ds_read_b128 {worst_k}-way ({cyc_k} cycles), "
          f"tr_b16 {worst_v}-way ({cyc_v} cycles)")
  return worst_k, worst_v, cyc_k, cyc_v


def check_mla_fp8_writes(D=576, sw=None, quiet=False):
  """The FP8 build of the MLA kernel (csrc/ffpa_fwd_m16_tile.inc under FFPA_M16_KV_FP8) has no LDS-DMA: lane l of piece p = wave PPW + i loads the EIGHT e4m3
  bytes at  key x row bytes + ((slot ^ sw(key)) << 3)  of the FP8 tile (g = 64 p + l, key = g / SPR, slot = g % SPR), widens them to eight 16-bit elements and
  writes them with ONE ds_write_b128 at  p x 1024 + 16 l.  Checks that
    * the image those writes leave is, byte for byte, the image the LDS-DMA pieces of the 16-bit build leave (``check_m16_shared``'s: element e of the 16-byte
      slot at dst comes from column 8 (slot ^ sw) + e of row key) — so every fragment read that function verifies holds for this build too;
    * the writes are conflict-free under the bank rule of ds_write_b128 (MI355X_MICROARCH.md section LDS): 8 groups of 8 contiguous lanes, bank = (a / 4) % 32,
      4 dwords per lane
  -> (worst conflict of a group in ways: 1 = free, extra cycles summed over the tile's groups)."""
  sw = sw or mla_sw
  assert D > 512 and D % 128 == 64, "the MLA hook lives in the un-pipelined split-D loop"
  BC = 32
  RB8, RB16, SPR = D, D * 2, D // 8
  PPW = BC * D * 2 // 4096
  dma, fp8 = {}, {}
  worst, cycles = 1, 0
  for wave in range(4):
    for i in range(PPW):
      dsts = []
      for lane in range(64):
        g = (wave * PPW + i) * 64 + lane
        key, slot = divmod(g, SPR)
        dst = (wave * PPW + i) * 1024 + lane * 16
        src16 = (slot ^ sw(D, key)) << 4  # the 16-bit build's source offset inside the row, bytes
        src8 = (slot ^ sw(D, key)) << 3   # the FP8 build's
        assert key < BC and 0 <= src8 and src8 + 8 <= RB8 and src16 + 16 <= RB16, (D, key, src8)
        for e in range(8):
          dma[dst + 2 * e] = (key, (src16 + 2 * e) // 2)  # (row, column) of the element at this LDS byte
          fp8[dst + 2 * e] = (key, src8 + e)               # byte e of the pair widens to element e of the slot
        dsts.append(dst)
      for grp in range(8):
        banks = {}
        for lane in range(8 * grp, 8 * grp + 8):
          for dw in range(4):
            banks.setdefault(((dsts[lane] + 4 * dw) // 4) % 32, set()).add(dsts[lane] + 4 * dw)
        m = max(len(v) for v in banks.values())
        worst, cycles = max(worst, m), cycles + m - 1
  assert len(dma) == BC * D and fp8 == dma, "the widened writes must leave the image of the LDS-DMA pieces"
  if not quiet:
    print(f"D={D:5d} MLA FP8 build BC={BC}: the ds_write_b128 image equals the LDS-DMA image; worst write conflict {worst}-way ({cycles} cycles)")
  return worst, cycles


def mla_gather_image(D, ids, count, num_rows, row_stride, esz, key0=0, sw=None):
  """The LDS image of ONE gathered tile of the sparse MLA builds, as csrc/ffpa_fwd_m16_paged_body.inc forms it under FFPA_M16_KV_GATHER (FFPA_M16_GATHER_LOAD /
  FFPA_M16_GATHER_FORM, restated): wave w keeps the ids of keys key0 + 8 w .. + 7 (entries read at min(n, topk - 1)), clamps them into [0, num_rows), gives keys at
  and past ``count`` bit 31 instead of a row offset, and lane l of its piece i reads  row offset + ((slot ^ sw(key)) << (3 | 4))  through ONE descriptor of
  ``span`` bytes — a piece spans at most two rows with a compile-time boundary lane.  ``esz``: bytes per pool element (2: the LDS-DMA build, 16 bytes per lane; 1:
  the FP8 build, 8 bytes per lane widened to 16).  ``row_stride`` in elements.  -> {LDS byte offset of an element: (pool row, column) or None (a zero)}, and
  asserts that every offset without the sentinel lies wholly inside the span and every offset with it outside."""
  sw = sw or mla_sw
  BC, SPR = 32, D // 8
  PPW = BC * D * 2 // 4096
  assert PPW * 64 == 8 * SPR
  row_bytes = row_stride * esz
  span = (num_rows - 1) * row_bytes + D * esz
  assert span <= 1 << 31
  topk = len(ids)
  img = {}
  for wave in range(4):
    g_ro = []
    left = count - (key0 + 8 * wave)
    for gk in range(8):
      n = key0 + 8 * wave + gk
      rid = ids[min(n, topk - 1)]
      rid = min(max(rid, 0), num_rows - 1)
      oob = min(max(gk + 1 - left, 0), 1)
      g_ro.append(((rid * row_bytes) & 0xffffffff) | (oob << 31))
    for i in range(PPW):
      lo, hi = i * 64 // SPR, (i * 64 + 63) // SPR
      for lane in range(64):
        g = (wave * PPW + i) * 64 + lane
        key, slot = divmod(g, SPR)
        g_sl = (slot ^ sw(D, key)) << (3 if esz == 1 else 4)
        off = (g_sl + (g_ro[lo] if lane < hi * SPR - i * 64 else g_ro[hi])) & 0xffffffff
        assert key - 8 * wave == (lo if lane < hi * SPR - i * 64 else hi), "the boundary lane splits the piece where its rows change"
        dst = (wave * PPW + i) * 1024 + lane * 16
        live = off + 8 * esz <= span  # (the descriptor's range check of a raw buffer: the whole access inside num_records)
        assert live == (off < (1 << 31)), (wave, i, lane, off, span)
        for e in range(8):
          img[dst + 2 * e] = (off // row_bytes, (off % row_bytes) // esz + e) if live else None
  assert len(img) == BC * D
  return img


def check_mla_fp8_gather_writes(D=576, cases=None, quiet=False):
  """The FP8 build of the SPARSE MLA kernel (csrc/ffpa_mla_sparse_fp8_inst.hip: FFPA_M16_KV_GATHER and FFPA_M16_KV_FP8 together): for a gathered tile with
  arbitrary row ids — in and out of the pool, duplicates, garbage at and past the count — the image its widened ds_write_b128s leave equals, element for element,
  the image the LDS-DMA pieces of the 16-bit sparse build leave for the same ids over the same rows (``mla_gather_image`` with 1 and 2 bytes per element; the row
  stride in elements is the same, so the FP8 pool's row bytes are half).  The writes themselves are ``check_mla_fp8_writes``': lane l of piece p at p x 1024 + 16
  l, conflict-free.  ``cases``: (ids, count, num_rows, row_stride, key0) tuples; default: a seeded set.  -> the number of cases checked."""
  import random

  if cases is None:
    rng = random.Random(24)
    cases = []
    for num_rows, row_stride in ((1024, D), (1024, 592), (7, 1152), (1, D), (3_700_000, D)):
      for count in (0, 1, 7, 8, 9, 31, 32, 33, 64, 97):
        topk = max(count, 1) + rng.choice((0, 3, 40))
        ids = [rng.randrange(num_rows) for _ in range(count)] + [rng.choice((-1, -(1 << 31), (1 << 31) - 1, num_rows, num_rows + 5)) for _ in range(topk - count)]
        if count > 2:
          ids[1] = -3  # (in front of the count and outside the pool: clamped, not followed)
          ids[2] = num_rows + 11
        for key0 in range(0, max(count, 1) + 32, 32):
          cases.append((ids, count, num_rows, row_stride, key0))
  for ids, count, num_rows, row_stride, key0 in cases:
    if (num_rows - 1) * row_stride * 2 + D * 2 <= 1 << 31:
      a = mla_gather_image(D, ids, count, num_rows, row_stride, 2, key0)
    else:  # (a pool only the FP8 build reaches: the 16-bit image of the rows it names, without that build's span)
      a = None
    b = mla_gather_image(D, ids, count, num_rows, row_stride, 1, key0)
    if a is not None:
      assert a == b, ("the FP8 gather must leave the 16-bit gather's image", count, num_rows, row_stride, key0)
    for dst, src in b.items():  # (either way: keys at and past the count are zeros, every other element is a column of a row of the pool)
      key = dst // (D * 2)
      if key0 + key >= count:
        assert src is None
      else:
        assert src is not None and 0 <= src[0] < num_rows and 0 <= src[1] < D
  worst, _ = check_mla_fp8_writes(D, quiet=True)
  assert worst == 1
  if not quiet:
    print(f"D={D:5d} MLA sparse FP8 build: {len(cases)} gathered tiles leave the 16-bit gather's image; ds_write_b128 pattern unchanged (conflict-free)")
  return len(cases)


def variants(D):
  """(D, ND) pairs the library instantiates: the prefill tiles and the short-query (split over 2 / 4 waves) tiles."""
  return [(D, 1 if D <= 512 else 2), (D, 4 if D % 128 == 0 else 2)]


if __name__ == "__main__":
  if "--mla" in sys.argv[1:]:  # the shared image of the MLA build: every candidate map, then the one the kernel uses
    for name, fn in MLA_CANDIDATES.items():
      print(f"{name:6s}", end=" ")
      check_m16_shared(576, fn)
    print("kernel", end=" ")
    check_m16_shared(576)
    check_mla_fp8_writes(576)
    check_mla_fp8_gather_writes(576)
    sys.exit(0)
  for D in ([int(x) for x in sys.argv[1:]] or [64, 128, 192, 256, 320, 384, 448, 512, 576, 640, 704, 768, 832, 896, 960, 1024]):
    for d, nd in dict.fromkeys(variants(D)):
      check(d, nd)
    check_m16(D)
