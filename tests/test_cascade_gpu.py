"""Cascade (shared-prefix) attention and the merge of two attention states on the GPU: the merge kernel against a float64 evaluation of its formula (one ulp of
the output dtype, LSE to 1e-5), ffpa_attn_with_kvcache_cascade against a float64 attention (no further from it than the plain launch, plus one ulp) over paged
and contiguous caches, cascade=False bit-identical to ffpa_attn_with_kvcache, the prefix read from sequence 0 only, graph capture with the table and lengths
written in place, torch.compile and opcheck."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GQA = (32, 8)
MHA = (8, 8)
_MANT = {torch.bfloat16: 7, torch.float16: 10}
_MIN_EXP = {torch.bfloat16: -126, torch.float16: -14}


def _ulp(x: torch.Tensor, dtype) -> torch.Tensor:
  """One ulp of `dtype` at |x| (float64), subnormals included."""
  a = x.abs().clamp_min(2.0 ** _MIN_EXP[dtype])
  return torch.exp2(torch.floor(torch.log2(a)) - _MANT[dtype])


# ---- the merge kernel
def _merge_ref(oa, la, ob, lb):
  """The merge formula in float64: (o [T, H, D], lse [H, T], the fp32 evaluation's own rounding bound per element)."""
  oa, ob = oa.double(), ob.double()
  la, lb = la.double().t()[..., None], lb.double().t()[..., None]  # [T, H, 1]
  m = torch.maximum(la, lb)
  empty = m == -math.inf
  ms = torch.where(empty, torch.zeros_like(m), m)
  wa, wb = torch.exp(la - ms), torch.exp(lb - ms)
  pa = torch.where(wa > 0, wa * torch.nan_to_num(oa), torch.zeros_like(oa))
  pb = torch.where(wb > 0, wb * torch.nan_to_num(ob), torch.zeros_like(ob))
  den = torch.where(empty, torch.ones_like(wa), wa + wb)
  o = torch.where(empty, torch.zeros_like(oa), (pa + pb) / den)
  lse = torch.where(empty, torch.full_like(m, -math.inf), ms + torch.log(den))[..., 0].t()
  # fp32 products, sum and quotient: a few roundings of 2^-24 relative to the terms (what cancels in the sum is the fp32 formula's, not the output's)
  slack = 4 * 2.0 ** -24 * (pa.abs() + pb.abs()) / den
  return o, lse, slack


def _merge_inputs(T, H, D, dtype, seed):
  g = torch.Generator(device="cuda").manual_seed(seed)
  oa = torch.randn((H, T, D), generator=g, device="cuda").to(dtype).transpose(0, 1)  # ([T, H, D] view of a head-major buffer: strides (D, T * D, 1))
  ob = torch.randn((T, H, D), generator=g, device="cuda").to(dtype)
  la_buf = torch.randn((H, T + 11), generator=g, device="cuda") * 4 + 3
  la = la_buf[:, :T]  # (strided LSE: head stride T + 11)
  lb = (torch.randn((H, T), generator=g, device="cuda") * 4 + 3)
  # gaps of +- 80, one side -inf, both -inf (with NaN in the O behind a -inf LSE)
  lb[:, 1] = la[:, 1] + 80
  lb[:, 2] = la[:, 2] - 80
  la[:, 3] = -math.inf
  lb[:, 4] = -math.inf
  la[:, 5] = -math.inf
  lb[:, 5] = -math.inf
  oa[3] = float("nan")
  ob[4] = float("nan")
  oa[5] = float("nan")
  ob[5] = float("nan")
  return oa, la, ob, lb


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [8, 72, 128, 512, 1024])
def test_merge_against_float64(dtype, D):
  from ffpa_attn_amd import ffpa_merge_attn_states

  T, H = 37, 5
  oa, la, ob, lb = _merge_inputs(T, H, D, dtype, seed=D)
  o, lse = ffpa_merge_attn_states(oa, la, ob, lb)
  torch.cuda.synchronize()
  ref_o, ref_lse, slack = _merge_ref(oa, la, ob, lb)
  assert o.shape == (T, H, D) and o.dtype == dtype and lse.shape == (H, T) and lse.dtype == torch.float32
  assert not torch.isnan(o).any()
  err = (o.double() - ref_o).abs()
  bound = _ulp(ref_o, dtype) + slack
  assert (err <= bound).all(), f"max err {err.max().item():.3e}, worst excess {(err - bound).max().item():.3e}"
  assert torch.equal(o[5], torch.zeros_like(o[5])) and (lse[:, 5] == -math.inf).all()
  finite = torch.isfinite(ref_lse)
  assert torch.equal(finite, torch.isfinite(lse)) and (lse[~finite] == -math.inf).all()
  assert ((lse.double() - ref_lse)[finite].abs() <= 1e-5).all(), (lse.double() - ref_lse)[finite].abs().max()
  # a side of -inf: the other side, exactly
  assert torch.equal(o[3], ob[3]) and torch.equal(o[4], oa[4])


def test_merge_of_a_decode_batch_and_of_one_row():
  """Few rows (64-lane workgroups) and many rows (a grid-stride loop): the same formula."""
  from ffpa_attn_amd import ffpa_merge_attn_states

  for T, H, D in ((1, 1, 8), (64 * 4, 32, 512), (4096, 16, 1024)):
    oa, la, ob, lb = _merge_inputs(max(T, 8), H, D, torch.bfloat16, seed=T)
    oa, la, ob, lb = oa[:T], la[:, :T], ob[:T], lb[:, :T]
    o, lse = ffpa_merge_attn_states(oa, la, ob, lb)
    torch.cuda.synchronize()
    ref_o, ref_lse, slack = _merge_ref(oa, la, ob, lb)
    assert ((o.double() - ref_o).abs() <= _ulp(ref_o, torch.bfloat16) + slack).all(), (T, H, D)


def test_merge_opcheck():
  import ffpa_attn_amd.hip  # noqa: F401

  oa, la, ob, lb = _merge_inputs(9, 4, 128, torch.float16, seed=3)
  la, lb = la.contiguous(), lb.contiguous()
  oa, ob = torch.nan_to_num(oa.contiguous()), torch.nan_to_num(ob)
  torch.library.opcheck(torch.ops.ffpa_attn._merge_states_hip.default, (oa, la, ob, lb))


# ---- cascade attention
def _case(B, P, suffix, Sq, hq, hkv, D, dtype, page, seed, nan_unused=True, diverge=False):
  """A shared-prefix batch: sequence b holds P shared keys then suffix[b] keys of its own.  page > 0: a pool of shuffled pages, the P / page prefix pages in
  every row of the table (diverge: rows 1 .. B - 1 point at OTHER pages of different content there); page 0: a contiguous cache whose slabs repeat slab 0's
  first P rows (diverge: different content there).  Unused pages and rows past a length are NaN.  Returns (k_cache, v_cache, table | None, lens, capacity,
  keys(b) -> (K [L, Hkv, D], V) in float64 with the prefix taken from sequence 0)."""
  g = torch.Generator(device="cuda").manual_seed(seed)
  lens = [P + s for s in suffix]
  if page:
    npre = P // page
    own = max(1, -(-max(suffix) // page))
    ppr = npre + own
    n_pages = npre + B * own + (B - 1) * npre + 3
    ids = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    table = torch.empty((B, ppr), dtype=torch.int32)
    shared = ids[:npre]
    nxt = npre
    for b in range(B):
      if diverge and b > 0:
        table[b, :npre] = torch.tensor(ids[nxt:nxt + npre], dtype=torch.int32)
        nxt += npre
      else:
        table[b, :npre] = torch.tensor(shared, dtype=torch.int32)
      table[b, npre:] = torch.tensor(ids[nxt:nxt + own], dtype=torch.int32)
      nxt += own
    kc = torch.randn((n_pages, page, hkv, D), generator=g, device="cuda").to(dtype)
    vc = torch.randn((n_pages, page, hkv, D), generator=g, device="cuda").to(dtype)
    if nan_unused:
      used_rows = torch.zeros((n_pages, page), dtype=torch.bool)
      for b in range(B):
        for j in range(lens[b]):
          used_rows[table[b, j // page], j % page] = True
      mask = (~used_rows).cuda()
      kc[mask] = float("nan")
      vc[mask] = float("nan")
    cap = ppr * page
    table = table.cuda()

    def keys(b):
      idx = torch.arange(lens[b])
      pg = torch.where(idx < P, table[0].cpu()[idx // page], table[b].cpu()[idx // page])
      return kc[pg.cuda(), (idx % page).cuda()].double(), vc[pg.cuda(), (idx % page).cuda()].double()
  else:
    cap = P + max(suffix) + 5
    table = None
    kc = torch.randn((B, cap, hkv, D), generator=g, device="cuda").to(dtype)
    vc = torch.randn((B, cap, hkv, D), generator=g, device="cuda").to(dtype)
    if not diverge:
      kc[1:, :P] = kc[0, :P]
      vc[1:, :P] = vc[0, :P]
    if nan_unused:
      for b in range(B):
        kc[b, lens[b]:] = float("nan")
        vc[b, lens[b]:] = float("nan")

    def keys(b):
      return torch.cat([kc[0, :P], kc[b, P:lens[b]]]).double(), torch.cat([vc[0, :P], vc[b, P:lens[b]]]).double()
  return kc, vc, table, torch.tensor(lens, dtype=torch.int32, device="cuda"), cap, keys


def _reference(q, keys, lens, causal, scale):
  """float64 attention of q [B, Sq, Hq, D] against keys(b), bottom-right causal; rows without a key: 0 / -inf."""
  B, Sq, Hq, D = q.shape
  out = torch.zeros((B, Sq, Hq, D), dtype=torch.float64, device=q.device)
  lse = torch.full((B, Hq, Sq), -math.inf, dtype=torch.float64, device=q.device)
  for b in range(B):
    K, V = keys(b)
    L = K.size(0)
    if L == 0:
      continue
    rep = Hq // K.size(1)
    K, V = K.repeat_interleave(rep, dim=1), V.repeat_interleave(rep, dim=1)
    s = torch.einsum("qhd,khd->hqk", q[b].double(), K) * scale
    if causal:
      i = torch.arange(Sq, device=q.device)[:, None]
      j = torch.arange(L, device=q.device)[None, :]
      s = s.masked_fill(j > i + L - Sq, -math.inf)
    m = s.amax(-1, keepdim=True)
    ok = torch.isfinite(m)
    p = torch.where(ok, torch.exp(s - torch.where(ok, m, torch.zeros_like(m))), torch.zeros_like(s))
    den = p.sum(-1, keepdim=True)
    o = torch.einsum("hqk,khd->qhd", p / torch.where(den > 0, den, torch.ones_like(den)), V)
    out[b] = o
    lse[b] = torch.where(ok[..., 0], m[..., 0] + torch.log(den[..., 0]), torch.full_like(m[..., 0], -math.inf))
  return out, lse


def _suffix(Sq, causal):
  # under causal every suffix holds at least the Sq query tokens (the documented contract); without, one sequence has an empty suffix
  return [Sq, 70, 129, 200, Sq + 5] if causal else [0, 70, 129, 200, 1]


def _check_accuracy(cas, plain, ref, dtype):
  err_p = (plain.double() - ref).abs().max()
  err_c = (cas.double() - ref).abs()
  bound = err_p + _ulp(ref, dtype)
  assert not torch.isnan(cas).any()
  assert (err_c <= bound).all(), f"cascade max err {err_c.max().item():.3e}, plain max err {err_p.item():.3e}"


@pytest.mark.parametrize("page", [0, 64, 256])
@pytest.mark.parametrize("D", [128, 512, 1024])
@pytest.mark.parametrize("heads", [MHA, GQA], ids=["mha", "gqa"])
@pytest.mark.parametrize("Sq", [1, 4])
@pytest.mark.parametrize("causal", [False, True])
def test_cascade_against_float64(page, D, heads, Sq, causal):
  from ffpa_attn_amd import ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_cascade

  hq, hkv = heads
  dtype = torch.bfloat16 if (D + Sq) % 3 else torch.float16
  B, P = 5, 256
  kc, vc, table, lens, cap, keys = _case(B, P, _suffix(Sq, causal), Sq, hq, hkv, D, dtype, page, seed=D + Sq + page)
  q = torch.randn((B, Sq, hq, D), device="cuda").to(dtype)
  kw = dict(cache_seqlens=lens, block_table=table, causal=causal, return_softmax_lse=True)
  cas, lse_c = ffpa_attn_with_kvcache_cascade(q, kc, vc, shared_prefix_len=P, cascade=True, **kw)
  plain, lse_p = ffpa_attn_with_kvcache(q, kc, vc, **kw)
  torch.cuda.synchronize()
  ref, ref_lse = _reference(q, keys, lens.tolist(), causal, D ** -0.5)
  _check_accuracy(cas, plain, ref, dtype)
  fin = torch.isfinite(ref_lse)
  assert torch.equal(torch.isfinite(lse_c), fin)
  assert ((lse_c.double() - ref_lse)[fin].abs() <= 1e-3).all()


@pytest.mark.parametrize("B, Sq, D, packed", [(5, 1, 512, True), (40, 1, 512, False), (5, 4, 1024, False), (4, 4, 128, True)])
def test_prefix_pass_gqa_pack_taken_and_not(B, Sq, D, packed):
  """The prefix pass is one sequence of B * Sq tokens: a KV group's query heads ride in the rows of one tile while group * B * Sq fits it, else one workgroup
  per query head.  Both give the float64 answer."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_cascade, hip

  hq, hkv = GQA
  P, page = 512, 64
  plan = hip.varlen_launch_plan(1, hq, hkv, B * Sq, P, D, page_size=page)
  assert (plan["workgroups"] == hkv) == packed, plan
  suffix = [Sq + (37 * b) % 300 for b in range(B)]
  kc, vc, table, lens, cap, keys = _case(B, P, suffix, Sq, hq, hkv, D, torch.bfloat16, page, seed=B + D)
  q = torch.randn((B, Sq, hq, D), device="cuda").to(torch.bfloat16)
  cas = ffpa_attn_with_kvcache_cascade(q, kc, vc, cache_seqlens=lens, block_table=table, shared_prefix_len=P, causal=True, cascade=True)
  plain = ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, block_table=table, causal=True)
  torch.cuda.synchronize()
  ref, _ = _reference(q, keys, lens.tolist(), True, D ** -0.5)
  _check_accuracy(cas, plain, ref, torch.bfloat16)


@pytest.mark.parametrize("page", [0, 64])
@pytest.mark.parametrize("interleaved", [True, False])
def test_cascade_with_append_and_rotary(page, interleaved):
  """k / v appended (K and q rotated) in front of both passes: the cache is written as the plain call writes it, and the answer is the float64 attention of
  the rotated q over the appended cache."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_cascade

  hq, hkv, D, Sq, B, P = 32, 8, 512, 2, 5, 256
  dtype = torch.bfloat16
  suffix = [3, 70, 129, 200, 8]
  kc, vc, table, lens, cap, _ = _case(B, P, [s + Sq for s in suffix], Sq, hq, hkv, D, dtype, page, seed=11 + page, nan_unused=False)
  lens = lens - Sq  # (the cache holds P + suffix keys; the step appends Sq more)
  g = torch.Generator(device="cuda").manual_seed(5)
  q = torch.randn((B, Sq, hq, D), generator=g, device="cuda").to(dtype)
  k = torch.randn((B, Sq, hkv, D), generator=g, device="cuda").to(dtype)
  v = torch.randn((B, Sq, hkv, D), generator=g, device="cuda").to(dtype)
  ang = torch.rand((cap, 64), generator=g, device="cuda") * 6.2831853
  cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
  kw = dict(k=k, v=v, rotary_cos=cos, rotary_sin=sin, cache_seqlens=lens, block_table=table, causal=True, rotary_interleaved=interleaved)
  kc_p, vc_p, kc_r, vc_r = kc.clone(), vc.clone(), kc.clone(), vc.clone()
  cas = ffpa_attn_with_kvcache_cascade(q, kc, vc, shared_prefix_len=P, cascade=True, **kw)
  plain = ffpa_attn_with_kvcache(q, kc_p, vc_p, **kw)
  q_rot, used = torch.ops.ffpa_attn._kvcache_append_hip(q, kc_r, vc_r, k, v, lens, table, cos, sin, interleaved, True)
  torch.cuda.synchronize()
  assert torch.equal(kc.view(torch.int16), kc_p.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_p.view(torch.int16))
  L = used.tolist()

  def keys(b):
    if page:
      idx = torch.arange(L[b], device="cuda")
      pg = table[b][idx // page].long()
      return kc_r[pg, idx % page].double(), vc_r[pg, idx % page].double()
    return kc_r[b, :L[b]].double(), vc_r[b, :L[b]].double()

  ref, _ = _reference(q_rot, keys, L, True, D ** -0.5)
  _check_accuracy(cas, plain, ref, dtype)


@pytest.mark.parametrize("page", [0, 64])
def test_cascade_false_and_trivial_cascades_are_the_plain_launch(page):
  from ffpa_attn_amd import ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_cascade

  hq, hkv, D, Sq, B, P = 32, 8, 512, 4, 5, 256
  kc, vc, table, lens, cap, _ = _case(B, P, _suffix(Sq, True), Sq, hq, hkv, D, torch.bfloat16, page, seed=7)
  q = torch.randn((B, Sq, hq, D), device="cuda").to(torch.bfloat16)
  kw = dict(cache_seqlens=lens, block_table=table, causal=True, return_softmax_lse=True)
  plain, lse = ffpa_attn_with_kvcache(q, kc, vc, **kw)
  for P_, mode in ((P, False), (0, True), (0, None), (0, False), (cap, True)):
    o, l = ffpa_attn_with_kvcache_cascade(q, kc, vc, shared_prefix_len=P_, cascade=mode, **kw)
    assert torch.equal(o, plain) and torch.equal(l, lse), (P_, mode)
  # a batch of one: the rule never cascades
  o1 = ffpa_attn_with_kvcache_cascade(q[:1], kc if page else kc[:1], vc if page else vc[:1], cache_seqlens=lens[:1],
                                      block_table=table[:1] if page else None, causal=True, shared_prefix_len=P)
  assert torch.equal(o1, ffpa_attn_with_kvcache(q[:1], kc if page else kc[:1], vc if page else vc[:1], cache_seqlens=lens[:1],
                                                block_table=table[:1] if page else None, causal=True))


@pytest.mark.parametrize("page", [0, 64])
def test_the_prefix_is_read_from_sequence_0_only(page):
  """Sequences 1 .. B - 1 hold OTHER content in their prefix rows (another page, or other rows of their slab) and unused rows are NaN: the cascade follows
  sequence 0's prefix — it never reads the others' copies."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_cascade

  hq, hkv, D, Sq, B, P = 32, 8, 128, 1, 5, 256
  kc, vc, table, lens, cap, keys = _case(B, P, _suffix(Sq, False), Sq, hq, hkv, D, torch.float16, page, seed=9, diverge=True)
  q = torch.randn((B, Sq, hq, D), device="cuda").to(torch.float16)
  cas = ffpa_attn_with_kvcache_cascade(q, kc, vc, cache_seqlens=lens, block_table=table, shared_prefix_len=P, cascade=True)
  torch.cuda.synchronize()
  ref, _ = _reference(q, keys, lens.tolist(), False, D ** -0.5)
  assert not torch.isnan(cas).any()
  assert ((cas.double() - ref).abs() <= 2e-3 + _ulp(ref, torch.float16)).all(), (cas.double() - ref).abs().max()


def test_cascade_captures_into_a_hip_graph_and_follows_table_and_lengths():
  """One capture; replays after cache_seqlens and the suffix columns of block_table are written in place equal the eager cascade on the new values."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_cascade

  hq, hkv, D, Sq, B, P, page = 32, 8, 512, 1, 5, 256, 64
  kc, vc, table, lens, cap, _ = _case(B, P, [130, 70, 129, 200, 64], Sq, hq, hkv, D, torch.bfloat16, page, seed=13, nan_unused=False)
  q = torch.randn((B, Sq, hq, D), device="cuda").to(torch.bfloat16)
  kw = dict(shared_prefix_len=P, causal=True, cascade=True, return_softmax_lse=True)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    ffpa_attn_with_kvcache_cascade(q, kc, vc, cache_seqlens=lens, block_table=table, **kw)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out, lse = ffpa_attn_with_kvcache_cascade(q, kc, vc, cache_seqlens=lens, block_table=table, **kw)
  npre = P // page
  for step in range(4):
    if step:
      lens.copy_(lens.flip(0) - step)
      suf = table[:, npre:].clone()
      table[:, npre:] = suf.roll(1, dims=0)
    graph.replay()
    eo, el = ffpa_attn_with_kvcache_cascade(q, kc, vc, cache_seqlens=lens.clone(), block_table=table.clone(), **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, eo) and torch.equal(lse, el), step


def test_cascade_under_torch_compile():
  from ffpa_attn_amd import ffpa_attn_with_kvcache_cascade

  hq, hkv, D, Sq, B, P, page = 16, 4, 256, 4, 5, 256, 64
  kc, vc, table, lens, cap, _ = _case(B, P, _suffix(Sq, True), Sq, hq, hkv, D, torch.float16, page, seed=17)
  q = torch.randn((B, Sq, hq, D), device="cuda").to(torch.float16)

  def f(q, kc, vc, lens, table):
    return ffpa_attn_with_kvcache_cascade(q, kc, vc, cache_seqlens=lens, block_table=table, shared_prefix_len=P, causal=True, cascade=True) * 2

  eager = f(q, kc, vc, lens, table)
  compiled = torch.compile(f)(q, kc, vc, lens, table)
  torch.cuda.synchronize()
  assert torch.equal(eager, compiled)
