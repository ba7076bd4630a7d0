"""The paged-KV call on the GPU (ffpa_attn_varlen_paged_fwd, ffpa_attn_with_kvcache(block_table=...)): the same bits as the contiguous seqused_k launch on the
gathered cache, the oracle on per-sequence keys, nothing read outside the used keys, graph capture with the table and lengths written in place, torch.compile."""

import numpy as np
import pytest
import torch

from test_fwd_gpu import _check_vs_oracle, hip  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

GQA = (32, 8)
MHA = (8, 8)


def _paged_case(lens, page, hkv, d, dtype, seed=0, nan_unused=False):
  """A pool whose pages are shuffled, in which sequence 4 shares its first pages with sequence 3 (a common prefix), one spare table entry per row pointing at a
  valid unused page; returns (pool_k, pool_v, table, seqused, the same cache gathered [B, capacity, Hkv, D])."""
  g = torch.Generator(device="cuda").manual_seed(seed)
  B = len(lens)
  need = [max(1, -(-n // page)) for n in lens]
  ppr = max(need) + 1
  shared = min(lens[3], lens[4]) // page if B > 4 else 0  # (whole pages both sequences fill: sequence 4 reads them from sequence 3's ids)
  n_pages = sum(need) - shared + 4
  ids = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
  table = torch.empty((B, ppr), dtype=torch.int32)
  nxt = 0
  for i in range(B):
    for j in range(need[i]):
      if i == 4 and j < shared:
        table[i, j] = table[3, j]
      else:
        table[i, j] = ids[nxt]
        nxt += 1
  spare = ids[nxt:]
  for i in range(B):
    for j in range(need[i], ppr):
      table[i, j] = spare[(i + j) % len(spare)]
  pk = torch.randn((n_pages, page, hkv, d), dtype=dtype, device="cuda", generator=g)
  pv = torch.randn((n_pages, page, hkv, d), dtype=dtype, device="cuda", generator=g)
  if nan_unused:
    used = set()
    for i in range(B):
      for j in range(-(-lens[i] // page)):
        used.add(int(table[i, j]))
    for p in range(n_pages):
      if p not in used:
        pk[p] = float("nan")
        pv[p] = float("nan")
    for i in range(B):
      if lens[i] % page:
        last = int(table[i, lens[i] // page])
        # rows past the length in the last page: NaN unless another sequence uses them (a shared prefix page)
        if not any(int(table[o, lens[i] // page]) == last and lens[o] > lens[i] for o in range(B) if o != i):
          pk[last, lens[i] % page:] = float("nan")
          pv[last, lens[i] % page:] = float("nan")
  table = table.cuda()
  cap = ppr * page
  kc = pk[table.long()].reshape(B, cap, hkv, d)
  vc = pv[table.long()].reshape(B, cap, hkv, d)
  return pk, pv, table, torch.tensor(lens, dtype=torch.int32, device="cuda"), kc, vc


def _lens(page):
  return [0, 1, page - 1, page + 1, page, 3000]  # (sequences 3 and 4 share their first page)


def _launch_pair(hip, q, cu_q, sq, causal, pk, pv, table, used, kc, vc, splits):
  B, cap, hkv, d = kc.shape
  scale = q.size(2) ** -0.5
  flags = hip.FLAG_FORCE_SPLITS if splits > 1 else 0
  plan_p, plan_c = {}, {}
  o_p, lse_p = hip.varlen_forward(q, pk, pv, cu_q, None, sq, cap, causal, scale, seqused_k=used, block_table=table, num_splits=splits, flags=flags, plan_out=plan_p)
  ck = torch.arange(0, (B + 1) * cap, cap, dtype=torch.int32, device="cuda")
  o_c, lse_c = hip.varlen_forward(q, kc.reshape(B * cap, hkv, d), vc.reshape(B * cap, hkv, d), cu_q, ck, sq, cap, causal, scale, seqused_k=used,
                                  num_splits=splits, flags=flags, plan_out=plan_c)
  assert plan_p["kernel"].startswith("ffpa_fwd_m16_paged_kernel") and plan_c["kernel"].startswith("ffpa_fwd_m16_varlen_kernel"), (plan_p, plan_c)
  assert plan_p["splits"] == plan_c["splits"] == splits, (plan_p, plan_c)
  return o_p, lse_p, o_c, lse_c, plan_p, plan_c


def _same_bits(o_p, lse_p, o_c, lse_c, dtype, name):
  assert torch.equal(lse_p, lse_c), name
  if dtype == torch.bfloat16:
    assert torch.equal(o_p, o_c), name
  else:
    # fp16: the same accumulators; the very last instruction (O / l rounded to fp16) is hipcc's per-element choice between v_fma_mixlo_f16 (one rounding) and
    # v_mul_f32 + v_cvt (two), made differently in the two kernels (tests/test_m16_gpu.py)
    diff = (o_p.float() - o_c.float()).abs()
    assert torch.all(diff <= torch.maximum(o_p.float().abs(), o_c.float().abs()).clamp_min(2.0 ** -14) * 2.0 ** -10), name
    assert (diff > 0).float().mean().item() <= 2e-3, name


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("page", [64, 128, 256])
@pytest.mark.parametrize("d", [128, 256, 320, 456, 512, 576, 1024])
def test_paged_launch_is_the_contiguous_launch_on_the_gathered_cache(hip, d, page, dtype):
  """Shuffled pages, a shared prefix, lengths 0 / 1 / page - 1 / page + 1 / page / 3000; decode (1 token), speculative decoding (4 tokens), a causal 200-token
  prefill chunk; MHA and GQA 32 / 8; 1, 2, 3 and 7 KV ranges forced on both sides.  Where the tiles are the same (every kernel head dim but 256 / 320; 456 runs on
  the 512 build) the bits are the contiguous launch's; at 256 / 320 (64-key tiles here, 128 there) they agree to rounding."""
  lens = _lens(page)
  B = len(lens)
  for hq, hkv in (MHA, GQA):
    pk, pv, table, used, kc, vc = _paged_case(lens, page, hkv, d, dtype, seed=d + page)
    for sq, causal in ((1, False), (4, True), (200, True)):
      g = torch.Generator(device="cuda").manual_seed(sq)
      q = torch.randn((B * sq, hq, d), dtype=dtype, device="cuda", generator=g)
      cu_q = torch.arange(0, (B + 1) * sq, sq, dtype=torch.int32, device="cuda")
      for splits in (1, 2, 3, 7):
        name = f"D{d} page{page} {hq}/{hkv} sq{sq} splits{splits} {dtype}"
        o_p, lse_p, o_c, lse_c, plan_p, _ = _launch_pair(hip, q, cu_q, sq, causal, pk, pv, table, used, kc, vc, splits)
        assert torch.isfinite(o_p).all(), name
        if (d + 63) // 64 * 64 in (256, 320):
          assert plan_p["block_keys"] == 64
          tol = 2e-2 if dtype == torch.bfloat16 else 4e-3
          assert torch.allclose(o_p.float(), o_c.float(), atol=tol, rtol=tol), name
          fin = torch.isfinite(lse_c)
          assert torch.equal(fin, torch.isfinite(lse_p)) and torch.allclose(lse_p[fin], lse_c[fin], atol=1e-4, rtol=1e-5), name
        else:
          _same_bits(o_p, lse_p, o_c, lse_c, dtype, name)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("d, page, heads", [(128, 64, GQA), (320, 128, MHA), (512, 64, GQA), (576, 256, GQA), (1024, 64, MHA)])
def test_with_kvcache_against_the_oracle(d, page, heads, dtype):
  """ffpa_attn_with_kvcache(block_table=...) on [B, Sq, Hq, D] against the CPU oracle on each sequence's gathered keys: decode and a causal 4-token step
  (bottom-right aligned), output [B, Sq, Hq, D] and LSE [B, Hq, Sq]."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  hq, hkv = heads
  lens = [5, page + 1, 700]
  pk, pv, table, used, kc, vc = _paged_case(lens, page, hkv, d, dtype, seed=7)
  for sq, causal in ((1, False), (4, True)):
    q = torch.randn((len(lens), sq, hq, d), dtype=dtype, device="cuda")
    out, lse = ffpa_attn_with_kvcache(q, pk, pv, cache_seqlens=used, block_table=table, causal=causal, return_softmax_lse=True, num_splits=1)
    torch.cuda.synchronize()
    assert out.shape == (len(lens), sq, hq, d) and lse.shape == (len(lens), hq, sq)
    for b, n in enumerate(lens):
      qb = q[b].transpose(0, 1)[None]                                    # [1, Hq, Sq, D]
      kb = kc[b, :n].transpose(0, 1).repeat_interleave(hq // hkv, 0)[None]  # [1, Hq, n, D]
      vb = vc[b, :n].transpose(0, 1).repeat_interleave(hq // hkv, 0)[None]
      ob = out[b].transpose(0, 1)[None]
      _check_vs_oracle(ob, lse[b][None], qb, kb, vb, causal=causal, causal_offset=(n - sq) if causal else None, block_keys=32 if d > 512 else 64,
                       name=f"b{b} sq{sq}")


@pytest.mark.parametrize("d, page", [(512, 64), (1024, 128), (200, 256)])
def test_nothing_outside_the_used_keys_is_read(hip, d, page):
  """Unused pages, the table entries past a sequence's last page (valid ids of NaN pages) and the rows past its length in its last page hold NaN: the outputs
  are finite and equal to the clean run's."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  lens = _lens(page)
  clean = _paged_case(lens, page, 8, d, torch.bfloat16, seed=3)
  dirty = _paged_case(lens, page, 8, d, torch.bfloat16, seed=3, nan_unused=True)
  assert torch.isnan(dirty[0]).any()
  for sq, causal in ((1, False), (4, True)):
    q = torch.randn((len(lens), sq, 32, d), dtype=torch.bfloat16, device="cuda")
    for splits in (1, 3):
      a, la = ffpa_attn_with_kvcache(q, clean[0], clean[1], cache_seqlens=clean[3], block_table=clean[2], causal=causal, num_splits=splits, return_softmax_lse=True)
      b, lb = ffpa_attn_with_kvcache(q, dirty[0], dirty[1], cache_seqlens=dirty[3], block_table=dirty[2], causal=causal, num_splits=splits, return_softmax_lse=True)
      assert torch.isfinite(b).all() and torch.equal(a, b) and torch.equal(la, lb)


def test_paged_call_captures_into_a_hip_graph_and_follows_table_and_lengths():
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  d, page = 512, 64
  pk, pv, table, used, _, _ = _paged_case([100, 300, 900, 5], page, 8, d, torch.bfloat16, seed=11)
  q = torch.randn((4, 1, 32, d), dtype=torch.bfloat16, device="cuda")
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    ffpa_attn_with_kvcache(q, pk, pv, cache_seqlens=used, block_table=table)  # (warm-up outside the capture)
  torch.cuda.current_stream().wait_stream(side)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    out = ffpa_attn_with_kvcache(q, pk, pv, cache_seqlens=used, block_table=table)
  perm = torch.randperm(table.numel(), generator=torch.Generator().manual_seed(1))
  for lens, tbl in (([100, 300, 900, 5], table.clone()), ([64, 0, 1000, 129], table.flatten()[perm.cuda()].view_as(table).clone())):
    used.copy_(torch.tensor(lens, dtype=torch.int32))
    table.copy_(tbl)
    g.replay()
    torch.cuda.synchronize()
    fresh = ffpa_attn_with_kvcache(q, pk, pv, cache_seqlens=used, block_table=table)
    assert torch.equal(out, fresh), lens


def test_paged_op_under_torch_compile():
  import ffpa_attn_amd.hip  # noqa: F401  (registers the op)

  d, page = 256, 128
  pk, pv, table, used, _, _ = _paged_case([10, 500, 129], page, 4, d, torch.float16, seed=5)
  q = torch.randn((3 * 2, 16, d), dtype=torch.float16, device="cuda")
  cu_q = torch.tensor([0, 2, 4, 6], dtype=torch.int32, device="cuda")

  def f(q, k, v, cu, used, tbl):
    o, lse = torch.ops.ffpa_attn._paged_fwd_hip(q, k, v, cu, used, tbl, 2, 1024, d ** -0.5, 1)
    return o * 2, lse

  eager = f(q, pk, pv, cu_q, used, table)
  compiled = torch.compile(f, fullgraph=True)(q, pk, pv, cu_q, used, table)
  assert torch.equal(eager[0], compiled[0]) and torch.equal(eager[1], compiled[1])


def test_contiguous_cache_route_of_with_kvcache(hip):
  """Without a block_table the call is the packed call's seqused_k launch on [B, capacity, Hkv, D]: the same bits."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  B, cap, hkv, hq, d = 3, 1024, 8, 32, 512
  kc = torch.randn((B, cap, hkv, d), dtype=torch.bfloat16, device="cuda")
  vc = torch.randn((B, cap, hkv, d), dtype=torch.bfloat16, device="cuda")
  q = torch.randn((B, 1, hq, d), dtype=torch.bfloat16, device="cuda")
  used = torch.tensor([1, 500, 1024], dtype=torch.int32, device="cuda")
  out, lse = ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=used, return_softmax_lse=True)
  cu = torch.arange(0, (B + 1) * cap, cap, dtype=torch.int32, device="cuda")
  cq = torch.arange(0, B + 1, dtype=torch.int32, device="cuda")
  o2, l2 = hip.varlen_forward(q.reshape(B, hq, d), kc.reshape(B * cap, hkv, d), vc.reshape(B * cap, hkv, d), cq, cu, 1, cap, False, d ** -0.5, seqused_k=used)
  assert torch.equal(out.reshape(B, hq, d), o2) and torch.equal(lse.reshape(B, hq), l2.t())
  assert np.isfinite(out.float().cpu().numpy()).all()
