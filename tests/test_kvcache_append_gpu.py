"""ffpa_attn_with_kvcache(k=, v=, rotary_cos=, rotary_sin=) on the GPU: the cache rows it writes against a torch restatement (V and unrotated dims bit-exact, rotated
dims within one ulp of the fp32 formula), every other row of NaN-filled pools untouched, O / LSE bit-identical to the torch route (rotate, scatter, add the
lengths, attend) and matching the oracle with each query at FlashAttention's position, graph capture with everything written in place, torch.compile."""

import pytest
import torch

from test_fwd_gpu import _check_vs_oracle

pytestmark = pytest.mark.gpu

GQA = (32, 8)
MHA = (8, 8)


def _rotate(x, cos, sin, pos, rd, interleaved):
  """x [n, H, D] at positions pos [n]: the first rd dims rotated in fp32 (x cos - y sin, y cos + x sin), one rounding; the rest unchanged."""
  if rd == 0 or x.size(0) == 0:
    return x.clone()
  xf = x.float()
  c = cos[pos].float()[:, None, :]
  s = sin[pos].float()[:, None, :]
  out = xf.clone()
  if interleaved:
    x0, x1 = xf[..., 0:rd:2], xf[..., 1:rd:2]
    out[..., 0:rd:2] = x0 * c - x1 * s
    out[..., 1:rd:2] = x1 * c + x0 * s
  else:
    h = rd // 2
    x0, x1 = xf[..., :h], xf[..., h:rd]
    out[..., :h] = x0 * c - x1 * s
    out[..., h:rd] = x1 * c + x0 * s
  return out.to(x.dtype)


def _tables(seqlen_ro, rd, dtype, seed):
  g = torch.Generator(device="cuda").manual_seed(seed)
  ang = torch.rand((seqlen_ro, max(rd // 2, 1)), generator=g, device="cuda") * 6.2831853
  return torch.cos(ang).to(dtype)[:, : rd // 2].contiguous(), torch.sin(ang).to(dtype)[:, : rd // 2].contiguous()


def _row_index(b, pos, page, table):
  """(page, row) of cache position pos of sequence b: the pool's index (contiguous: page = b); table: a host list of rows"""
  if table is None:
    return b, pos
  return table[b][pos // page], pos % page


def _make_case(lens, snew, page, hkv, d, dtype, seed, paged):
  """Caches whose rows below each sequence's length hold data and every other row NaN.  Paged: shuffled pages, sequence 4 shares its first page with sequence 3
  (a common prefix both have filled), the table entries past a sequence's last written page point at spare NaN pages.  Returns (kc, vc, table, cap)."""
  B = len(lens)
  ppr = 3
  cap = ppr * page
  g = torch.Generator(device="cuda").manual_seed(seed)
  if not paged:
    kc = torch.full((B, cap, hkv, d), float("nan"), dtype=dtype, device="cuda")
    vc = torch.full_like(kc, float("nan"))
    for b, n in enumerate(lens):
      kc[b, :n] = torch.randn((n, hkv, d), generator=g, device="cuda").to(dtype)
      vc[b, :n] = torch.randn((n, hkv, d), generator=g, device="cuda").to(dtype)
    return kc, vc, None, cap
  need = [max(1, -(-min(n + snew, cap) // page)) for n in lens]
  shared = min(lens[3], lens[4]) // page
  n_pages = sum(need) - shared + 3
  ids = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
  table = torch.empty((B, ppr), dtype=torch.int32)
  nxt = 0
  for b in range(B):
    for j in range(need[b]):
      if b == 4 and j < shared:
        table[b, j] = table[3, j]
      else:
        table[b, j] = ids[nxt]
        nxt += 1
  spare = ids[nxt:]
  for b in range(B):
    for j in range(need[b], ppr):
      table[b, j] = spare[(b + j) % len(spare)]
  kc = torch.full((n_pages, page, hkv, d), float("nan"), dtype=dtype, device="cuda")
  vc = torch.full_like(kc, float("nan"))
  for b, n in enumerate(lens):
    for j in range(-(-n // page)):
      if b == 4 and j < shared:
        continue
      rows = min(page, n - j * page)
      p = int(table[b, j])
      kc[p, :rows] = torch.randn((rows, hkv, d), generator=g, device="cuda").to(dtype)
      vc[p, :rows] = torch.randn((rows, hkv, d), generator=g, device="cuda").to(dtype)
  return kc, vc, table.cuda(), cap


def _torch_route(q, kc, vc, k, v, lens, table, cap, cos, sin, rd, interleaved, causal):
  """What a caller writes without the append: rotary in torch, the new rows scattered into the cache, the lengths added.  Returns (q_rot, kc', vc', used,
  written) on copies of the caches; written: the (page, row) of every row it wrote."""
  B, Sq = q.shape[:2]
  snew = k.size(1)
  page = kc.size(1)
  kc, vc = kc.clone(), vc.clone()
  table = table.tolist() if table is not None else None
  written = []
  q_rot = q
  if rd:
    qpos = torch.tensor([[n + (i if causal else 0) for i in range(Sq)] for n in lens], dtype=torch.long, device="cuda").clamp_max(cos.size(0) - 1)
    q_rot = _rotate(q.reshape(B * Sq, *q.shape[2:]), cos, sin, qpos.flatten(), rd, interleaved).view_as(q)
  for b, n in enumerate(lens):
    m = max(0, min(snew, cap - max(n, 0)))
    if m == 0:
      continue
    pos = torch.arange(max(n, 0), max(n, 0) + m, device="cuda")
    kr = _rotate(k[b, :m], cos, sin, pos, rd, interleaved) if rd else k[b, :m]
    for i in range(m):
      pg, row = _row_index(b, max(n, 0) + i, page, table)
      kc[pg, row] = kr[i]
      vc[pg, row] = v[b, i]
      written.append((pg, row))
  used = torch.tensor([min(max(n, 0) + snew, cap) for n in lens], dtype=torch.int32, device="cuda")
  return q_rot, kc, vc, used, written


def _assert_caches(kc, vc, kc_ref, vc_ref, written, dtype, name):
  """V: every element bit-identical (NaN sentinels included).  K: bit-identical outside the written rows; inside them within one ulp of the torch fp32 formula."""
  assert torch.equal(vc.view(torch.int16), vc_ref.view(torch.int16)), f"{name}: V pool"
  diff = kc.view(torch.int16) != kc_ref.view(torch.int16)
  mask = torch.zeros(kc.shape[:2], dtype=torch.bool, device="cuda")
  for pg, row in written:
    mask[pg, row] = True
  assert not (diff & ~mask[:, :, None, None]).any(), f"{name}: K rows outside the appended ones changed"
  if diff.any():
    got, want = kc[diff].float(), kc_ref[diff].float()
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    assert ((got - want).abs() <= want.abs().clamp_min(2.0 ** -14) * ulp).all(), f"{name}: rotated K beyond one ulp"


def _gathered(c, b, n, table, page):
  if table is None:
    return c[b, :n]
  ids = table[b].long().repeat_interleave(page)[:n]
  return c[ids, torch.arange(n, device=c.device) % page]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("layout", ["contiguous", "page64", "page256"])
@pytest.mark.parametrize("d", [128, 320, 456, 512, 576, 1024])
def test_append_writes_the_rows_and_attends_like_the_torch_route(d, layout, dtype):
  """Lengths 0 / 1 / page - 1 / page + 1 / page + 3 (sequences 3 and 4 share their first page) / capacity - 2 / capacity: appends that cross a page boundary, one
  that runs past the capacity (its tail dropped), one into a full cache (dropped).  Snew 1 / 4 / 17 x (interleaved rotary over every dim it can, NeoX over 128,
  none) x GQA / MHA x causal / not."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache
  from ffpa_attn_amd import hip as hipmod

  paged = layout != "contiguous"
  page = {"contiguous": 64, "page64": 64, "page256": 256}[layout]
  rd_full = d // 16 * 16
  for step, (snew, (hq, hkv), rd, interleaved, causal) in enumerate(((1, GQA, rd_full, True, False), (4, MHA, 128, False, True), (17, GQA, 0, True, True))):
    name = f"D{d} {layout} {dtype} Snew{snew} rd{rd} {'inter' if interleaved else 'neox'} causal{causal}"
    lens = [0, 1, page - 1, page + 1, page + 3, 3 * page - 2, 3 * page]
    B = len(lens)
    kc, vc, table, cap = _make_case(lens, snew, page, hkv, d, dtype, seed=d + step, paged=paged)
    g = torch.Generator(device="cuda").manual_seed(100 + step)
    sq = 2 if snew == 1 else snew  # (Sq may differ from Snew: two queries at the decode step's position)
    q = torch.randn((B, sq, hq, d), generator=g, device="cuda").to(dtype)
    k = torch.randn((B, snew, hkv, d), generator=g, device="cuda").to(dtype)
    v = torch.randn((B, snew, hkv, d), generator=g, device="cuda").to(dtype)
    cos, sin = _tables(cap + 5, rd, dtype, seed=step) if rd else (None, None)
    seqlens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    q_rot, kc_ref, vc_ref, used, written = _torch_route(q, kc, vc, k, v, lens, table, cap, cos, sin, rd, interleaved, causal)
    q0 = q.clone()
    out, lse = ffpa_attn_with_kvcache(q, kc, vc, k=k, v=v, rotary_cos=cos, rotary_sin=sin, cache_seqlens=seqlens, block_table=table, causal=causal,
                                      rotary_interleaved=interleaved, num_splits=1, return_softmax_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(q, q0) and torch.equal(seqlens.cpu(), torch.tensor(lens, dtype=torch.int32)), f"{name}: q / cache_seqlens modified"
    _assert_caches(kc, vc, kc_ref, vc_ref, written, dtype, name)
    # the rotated q and the lengths straight from the op, unconditionally: every rotary form against the fp32 formula
    q_op, used_op = torch.ops.ffpa_attn._kvcache_append_hip(q, kc.clone(), vc.clone(), k, v, seqlens, table, cos, sin, interleaved, causal)
    torch.cuda.synchronize()
    assert torch.equal(used_op, used), f"{name}: lengths"
    if rd:
      assert q_op.shape == q.shape and torch.equal(q_op[..., rd:], q[..., rd:]), f"{name}: q dims past rotary_dim"
      ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
      got, want = q_op[..., :rd].float(), q_rot[..., :rd].float()
      assert ((got - want).abs() <= want.abs().clamp_min(2.0 ** -14) * ulp).all(), f"{name}: rotated q beyond one ulp"
    # (b): the attention launch alone on the torch route's cache — the same bits whenever the rotated rows are (always without rotary)
    out_b, lse_b = ffpa_attn_with_kvcache(q_rot, kc_ref, vc_ref, cache_seqlens=used, block_table=table, causal=causal, num_splits=1, return_softmax_lse=True)
    if rd == 0:
      assert torch.equal(kc.view(torch.int16), kc_ref.view(torch.int16)), name
    if torch.equal(kc.view(torch.int16), kc_ref.view(torch.int16)):
      assert torch.equal(out, out_b) and torch.equal(lse, lse_b), f"{name}: O / LSE differ from the torch route"
    if snew != 4:
      continue
    # the oracle, every sequence on its gathered keys, queries at FlashAttention's positions (bottom-right causal over L = min(len + Snew, capacity))
    bk = hipmod.varlen_launch_plan(B, hq, hkv, sq, cap, d, total_q=B * sq, page_size=page if paged else 0, num_splits=1)["block_keys"]
    for b in range(B):
      n = int(used[b])
      qb = q_rot[b].transpose(0, 1)[None]
      kb = _gathered(kc_ref, b, n, table, page).transpose(0, 1).repeat_interleave(hq // hkv, 0)[None]
      vb = _gathered(vc_ref, b, n, table, page).transpose(0, 1).repeat_interleave(hq // hkv, 0)[None]
      _check_vs_oracle(out[b].transpose(0, 1)[None], lse[b][None], qb, kb, vb, causal=causal, causal_offset=(n - sq) if causal else None, block_keys=bk,
                       name=f"{name} b{b}")


@pytest.mark.parametrize("causal", [False, True])
def test_query_positions_follow_flash_attention(causal):
  """Rotary over the whole head dim with a small seqlen_ro: query token i sits at cache_seqlens + i when causal and at cache_seqlens otherwise — checked through
  the output against fp32 SDPA on explicitly rotated q / k."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  B, hq, hkv, d, cap, snew = 2, 8, 2, 128, 256, 4
  lens = [10, 200]
  dtype = torch.bfloat16
  kc = torch.randn((B, cap, hkv, d), device="cuda").to(dtype)
  vc = torch.randn((B, cap, hkv, d), device="cuda").to(dtype)
  q = torch.randn((B, snew, hq, d), device="cuda").to(dtype)
  k = torch.randn((B, snew, hkv, d), device="cuda").to(dtype)
  v = torch.randn((B, snew, hkv, d), device="cuda").to(dtype)
  cos, sin = _tables(cap, d, dtype, seed=9)
  out = ffpa_attn_with_kvcache(q, kc, vc, k=k, v=v, rotary_cos=cos, rotary_sin=sin, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device="cuda"),
                               causal=causal, rotary_interleaved=False)
  for b, n in enumerate(lens):
    qpos = torch.arange(n, n + snew, device="cuda") if causal else torch.full((snew,), n, device="cuda")
    qr = _rotate(q[b], cos, sin, qpos, d, False).float().transpose(0, 1)
    kk = kc[b, : n + snew].float().transpose(0, 1).repeat_interleave(hq // hkv, 0)
    vv = vc[b, : n + snew].float().transpose(0, 1).repeat_interleave(hq // hkv, 0)
    L = n + snew
    mask = None
    if causal:
      mask = torch.arange(L, device="cuda")[None, :] <= torch.arange(snew, device="cuda")[:, None] + (L - snew)
    ref = torch.nn.functional.scaled_dot_product_attention(qr[None], kk[None], vv[None], attn_mask=mask)[0].transpose(0, 1)
    assert torch.allclose(out[b].float(), ref, atol=2e-2, rtol=2e-2), (b, (out[b].float() - ref).abs().max().item())


def test_zero_new_tokens_and_out_of_range_lengths():
  """Snew = 0 appends nothing; negative lengths act as 0; a length past the capacity writes nothing and attends to the capacity."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  B, hq, hkv, d, cap = 3, 8, 8, 256, 128
  dtype = torch.float16
  kc = torch.randn((B, cap, hkv, d), device="cuda").to(dtype)
  vc = torch.randn((B, cap, hkv, d), device="cuda").to(dtype)
  q = torch.randn((B, 1, hq, d), device="cuda").to(dtype)
  lens = torch.tensor([-5, 7, 1000], dtype=torch.int32, device="cuda")
  k0, v0 = kc.clone(), vc.clone()
  z = torch.empty((B, 0, hkv, d), dtype=dtype, device="cuda")
  out = ffpa_attn_with_kvcache(q, kc, vc, k=z, v=z, cache_seqlens=lens)
  assert torch.equal(kc, k0) and torch.equal(vc, v0)
  assert torch.equal(out, ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=torch.tensor([0, 7, cap], dtype=torch.int32, device="cuda")))
  k = torch.randn((B, 2, hkv, d), device="cuda").to(dtype)
  ffpa_attn_with_kvcache(q, kc, vc, k=k, v=k, cache_seqlens=lens)
  torch.cuda.synchronize()
  assert torch.equal(kc[0, :2], k[0]) and torch.equal(kc[1, 7:9], k[1]) and torch.equal(kc[2], k0[2]) and torch.equal(kc[0, 2:], k0[0, 2:])


@pytest.mark.parametrize("paged", [False, True])
def test_append_step_captures_into_a_hip_graph(paged):
  """One decode step with k / v / rotary captured once; N replays with cache_seqlens, k, v and q written in place between them equal N eager steps."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  kc, vc, table, cap = _make_case([5, 63, 130, 64, 70, 0, 1], 8, 64, 8, 512, torch.bfloat16, seed=21, paged=paged)
  B, hq, hkv, d = 7, 32, 8, 512
  cos, sin = _tables(cap, 256, torch.bfloat16, seed=4)
  kc_e, vc_e = kc.clone(), vc.clone()
  lens = torch.tensor([5, 63, 130, 64, 70, 0, 1], dtype=torch.int32, device="cuda")
  q = torch.zeros((B, 1, hq, d), dtype=torch.bfloat16, device="cuda")
  k = torch.zeros((B, 1, hkv, d), dtype=torch.bfloat16, device="cuda")
  v = torch.zeros_like(k)
  kw = dict(rotary_cos=cos, rotary_sin=sin, block_table=table, causal=True, rotary_interleaved=False)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    ffpa_attn_with_kvcache(q, kc.clone(), vc.clone(), k=k, v=v, cache_seqlens=lens, **kw)  # (warm-up outside the capture)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = ffpa_attn_with_kvcache(q, kc, vc, k=k, v=v, cache_seqlens=lens, **kw)
  g = torch.Generator(device="cuda").manual_seed(5)
  for step in range(6):
    qs = torch.randn(q.shape, generator=g, device="cuda").to(q.dtype)
    ks = torch.randn(k.shape, generator=g, device="cuda").to(k.dtype)
    vs = torch.randn(v.shape, generator=g, device="cuda").to(v.dtype)
    q.copy_(qs), k.copy_(ks), v.copy_(vs)
    graph.replay()
    eager = ffpa_attn_with_kvcache(qs, kc_e, vc_e, k=ks, v=vs, cache_seqlens=lens.clone(), **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, eager), step
    assert torch.equal(kc.view(torch.int16), kc_e.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_e.view(torch.int16)), step
    lens += 1  # (the caller advances the lengths, in place)


def test_append_under_torch_compile():
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  kc, vc, table, cap = _make_case([5, 63, 130, 64, 70, 0, 1], 4, 64, 4, 256, torch.float16, seed=8, paged=True)
  B, hq, hkv, d = 7, 16, 4, 256
  cos, sin = _tables(cap, 128, torch.float16, seed=2)
  lens = torch.tensor([5, 63, 130, 64, 70, 0, 1], dtype=torch.int32, device="cuda")
  q = torch.randn((B, 4, hq, d), device="cuda").to(torch.float16)
  k = torch.randn((B, 4, hkv, d), device="cuda").to(torch.float16)
  v = torch.randn((B, 4, hkv, d), device="cuda").to(torch.float16)

  def f(q, kc, vc, k, v, lens, table):
    o = ffpa_attn_with_kvcache(q, kc, vc, k=k, v=v, rotary_cos=cos, rotary_sin=sin, cache_seqlens=lens, block_table=table, causal=True)
    return o * 2

  kc_c, vc_c = kc.clone(), vc.clone()
  eager = f(q, kc, vc, k, v, lens, table)
  compiled = torch.compile(f)(q, kc_c, vc_c, k, v, lens, table)
  torch.cuda.synchronize()
  assert torch.equal(eager, compiled)
  assert torch.equal(kc.view(torch.int16), kc_c.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_c.view(torch.int16))
