"""The KV-cache calls on the GPU against a float64 restatement of the whole call (tests/kvcache_ref.py), at the shapes and layouts serving engines use:
the NT (non-temporal fetch) paged kernel of every built head dim, the library's own plan at a decode batch of 32 x 16k keys, strided pools / caches / q / k / v /
block tables / lengths, data past 2^31 elements and 2^32 bytes, the edges of the contract, and a seeded sweep of the family.  Every output is held to
``kvcache_ref.allowance`` (the expression of test_fwd_gpu._check_vs_oracle, statistics from the float64 reference), every LSE to atol 2e-4 / rtol 2e-5, every
cache after an append to the reference's whole storage.

Worst error / allowance the run on MI355X showed, per entry point and dtype: see profiles/r10_kvcache_serving.md (the last test of this module prints them)."""

import contextlib
import os

import pytest
import torch

import kvcache_ref as R
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

RATIOS: dict = {}  # (entry point, dtype) -> worst error / allowance seen by this run


def _note(entry, dtype, ratio):
  key = (entry, R._dt(dtype))
  RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


@contextlib.contextmanager
def _launches(hip, flags=0):
  """Every attention launch inside the block carries ``flags`` too, and its plan (``plan_out``) is appended to the list the block receives."""
  plans, real = [], hip.varlen_forward

  def spy(*args, **kw):
    plan = {}
    kw["flags"] = kw.get("flags", 0) | flags
    kw["plan_out"] = plan
    out = real(*args, **kw)
    plans.append(plan)
    return out

  hip.varlen_forward = spy
  try:
    yield plans
  finally:
    hip.varlen_forward = real


def make_case(**kw) -> dict:
  """A hand-made case in the sweep's vocabulary (kvcache_ref.draw_case), every field explicit or defaulted."""
  c = dict(seed=kw.pop("seed", 0), dtype="bf16", page=64, D=128, entry="plain", layout="separate", table_layout="plain", lens_strided=False, fused_qkv=False,
           heads=(8, 2), B=None, num_splits=0, stream="auto", causal=False, return_lse=True, Sq=1, Snew=None, rotary_dim=0, interleaved=True, pages_per_seq=None,
           capacity=None, seqlen_ro=None, shared_prefix_len=0, lens=[100], bad_unused_ids=False, bad_used_id=False, share_prefix_pages=False)
  c.update(kw)
  c["B"] = len(c["lens"])
  unit = c["page"] or 64
  if c["pages_per_seq"] is None:
    c["pages_per_seq"] = -(-(max(max(c["lens"]), 1) + (c["Snew"] or 0)) // unit) + 1
  if c["capacity"] is None:
    c["capacity"] = c["pages_per_seq"] * unit
  if c["page"]:
    c["capacity"] = c["pages_per_seq"] * c["page"]
  if c["seqlen_ro"] is None:
    c["seqlen_ro"] = c["capacity"]
  c["head_dim_class"] = max(128, (c["D"] + 63) // 64 * 64)
  return c


_STREAM_FLAG = {"auto": lambda h: 0, "on": lambda h: h.FLAG_KV_STREAM, "off": lambda h: h.FLAG_NO_KV_STREAM}


def run_case(hip, c: dict) -> list:
  """A case through the public call against the float64 reference: output, LSE, the cache's whole storage, the caller's view.  -> the plans of its launches."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_cascade

  t = R.materialize(c, "cuda")
  ref, kview_w, vview_w, ks_w, vs_w, rotated = R.reference(c, t)
  ptrs = (t["k_cache"].data_ptr(), t["v_cache"].data_ptr())
  kw = dict(cache_seqlens=t["lens"], block_table=t["table"], causal=c["causal"], num_splits=c["num_splits"], return_softmax_lse=c["return_lse"])
  if t["k"] is not None:
    kw.update(k=t["k"], v=t["v"], rotary_cos=t["cos"], rotary_sin=t["sin"], rotary_interleaved=c["interleaved"])
  q_before = t["q"].clone()
  with _launches(hip, _STREAM_FLAG[c["stream"]](hip)) as plans:
    if c["entry"] == "cascade":
      res = ffpa_attn_with_kvcache_cascade(t["q"], t["k_cache"], t["v_cache"], shared_prefix_len=c["shared_prefix_len"], cascade=True, **kw)
    else:
      res = ffpa_attn_with_kvcache(t["q"], t["k_cache"], t["v_cache"], **kw)
  torch.cuda.synchronize()
  out, lse = res if c["return_lse"] else (res, None)
  name = f"case {c}"
  assert torch.equal(t["q"], q_before), f"q was modified: {name}"
  assert (t["k_cache"].data_ptr(), t["v_cache"].data_ptr()) == ptrs
  eff = R.effective_lens(c)
  ratio = R.check(out, lse, ref, v=R.visible_values(vview_w, eff, t["table"]), dtype=c["dtype"], name=name)
  _note(c["entry"] if c["entry"] != "append" or not c["rotary_dim"] else "append_rotary", c["dtype"], ratio)
  # the cache: the whole owning storage is the reference's (an entry that appends nothing: untouched), and the write is visible through the caller's view
  R.check_cache(t["k_storage"], ks_w, t["k_cache"], kview_w, rotated, c["rotary_dim"], name)
  if t["v_storage"] is not t["k_storage"]:
    R.check_cache(t["v_storage"], vs_w, t["v_cache"], vview_w, [], 0, name)
  assert torch.equal(t["v_cache"].view(torch.int16), vview_w.view(torch.int16)), name
  return plans


# ----------------------------------------------------------------------------- a. the NT paged kernel of every built head dim
@pytest.mark.parametrize("d", list(R.PAGED_HEAD_DIM_CLASSES) + [200, 456])
def test_nt_paged_kernel_of_every_head_dim_against_float64(hip, d):
  """FLAG_KV_STREAM through the paged entry: bf16 and fp16, MHA and packed GQA, 1 and 4 tokens, num_splits 1 and the library's own, shuffled pages, lengths
  0 / 1 / page - 1 / page + 1 / 3000 / 5000.  The plan names the NT build; the output is float64's to the allowance and, unsplit, the plain build's to the bit."""
  page = 128
  lens = [0, 1, page - 1, page + 1, 3000, 5000]
  B = len(lens)
  for dtype in ("bf16", "fp16"):
    for hq, hkv in ((4, 4), (8, 2)):
      c = make_case(D=d, dtype=dtype, page=page, heads=(hq, hkv), lens=lens, seed=d)
      t = R.materialize(c, "cuda")
      vstat = R.visible_values(t["v_cache"], lens, t["table"])
      for sq, causal in ((1, False), (4, True)):
        q = torch.randn((B, sq, hq, d), dtype=R.TORCH_DTYPE[dtype], device="cuda", generator=torch.Generator(device="cuda").manual_seed(sq))
        ref = R.attend(q, t["k_cache"], t["v_cache"], lens, t["table"], causal)
        cu_q = torch.arange(0, (B + 1) * sq, sq, dtype=torch.int32, device="cuda")
        for splits in (1, 0):
          plan = {}
          o, lse = hip.varlen_forward(q.view(B * sq, hq, d), t["k_cache"], t["v_cache"], cu_q, None, sq, c["capacity"], causal, d ** -0.5, seqused_k=t["lens"],
                                      block_table=t["table"], num_splits=splits, flags=hip.FLAG_KV_STREAM, plan_out=plan)
          name = f"D{d} {dtype} {hq}/{hkv} sq{sq} splits{splits} -> {plan}"
          want_kernel = f"ffpa_fwd_m16_paged_kernel<{dtype}, {c['head_dim_class']}, NT>"
          assert plan["kernel"].startswith(want_kernel), name
          assert (" (GQA heads packed into rows)" in plan["kernel"]) == (hq != hkv), name
          print(f"[nt-paged] {name}")
          _note("paged NT", dtype, R.check(o.view(B, sq, hq, d), lse.view(hq, B, sq).permute(1, 0, 2), ref, v=vstat, dtype=dtype, name=name))
          if splits == 1:
            plain = {}
            o2, lse2 = hip.varlen_forward(q.view(B * sq, hq, d), t["k_cache"], t["v_cache"], cu_q, None, sq, c["capacity"], causal, d ** -0.5, seqused_k=t["lens"],
                                          block_table=t["table"], num_splits=1, flags=hip.FLAG_NO_KV_STREAM, plan_out=plain)
            assert ", NT" not in plain["kernel"], plain
            assert torch.equal(o, o2) and torch.equal(lse, lse2), name


# ----------------------------------------------------------------------------- b. the library's own choice at a serving size
@pytest.mark.parametrize("d, heads, page", [(512, (32, 8), 64), (512, (32, 8), 256), (1024, (16, 4), 64)])
def test_decode_batch_of_serving_size_takes_the_nt_kernel_and_is_float64s(hip, d, heads, page):
  """32 sequences of 1k ... 16k keys, one token each (the shape of ``bench.py --workload varlen_decode``), no flag, num_splits = 0: the plan read back is the NT
  paged build with the split count the library picked; every row against float64.  Then the same batch with k / v + rotary, and — the sequences sharing their
  first 8k keys — through the cascade under cascade=None (the rule takes it).  Peak allocation: D 512: 2 x 2.3 GiB pools + clones; D 1024: twice that."""
  import ffpa_attn_amd.kvcache as kvc
  from ffpa_attn_amd import ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_cascade

  hq, hkv = heads
  B, P = 32, 8192
  lens = [1024 + (16384 - 1024 - 1) * i // (B - 1) for i in range(B)]
  for variant in ("plain", "append_rotary", "cascade"):
    ls = [P + n // 2 for n in lens] if variant == "cascade" else lens
    c = make_case(D=d, dtype="bf16", page=page, heads=heads, lens=ls, pages_per_seq=16384 // page + 1, seed=d + page, entry=variant if variant != "append_rotary" else "append",
                  Snew=1 if variant == "append_rotary" else None, rotary_dim=128 if variant == "append_rotary" else 0, interleaved=False,
                  shared_prefix_len=P if variant == "cascade" else 0)
    t = R.materialize(c, "cuda")
    ref, kview_w, vview_w, ks_w, vs_w, rotated = R.reference(c, t)
    kw = dict(cache_seqlens=t["lens"], block_table=t["table"], return_softmax_lse=True)
    took = []
    real_cascade = kvc._cascade
    kvc._cascade = lambda *a, **k: (took.append(1), real_cascade(*a, **k))[1]
    try:
      with _launches(hip) as plans:
        if variant == "cascade":
          assert kvc.cascade_rule(B, 1, hq, hkv, d, P, page)
          out, lse = ffpa_attn_with_kvcache_cascade(t["q"], t["k_cache"], t["v_cache"], shared_prefix_len=P, **kw)
        elif variant == "append_rotary":
          out, lse = ffpa_attn_with_kvcache(t["q"], t["k_cache"], t["v_cache"], k=t["k"], v=t["v"], rotary_cos=t["cos"], rotary_sin=t["sin"], rotary_interleaved=False, **kw)
        else:
          out, lse = ffpa_attn_with_kvcache(t["q"], t["k_cache"], t["v_cache"], **kw)
    finally:
      kvc._cascade = real_cascade
    torch.cuda.synchronize()
    name = f"D{d} {hq}/{hkv} page{page} {variant}: {plans}"
    print(f"[serving] {name}")
    assert len(took) == (1 if variant == "cascade" else 0), name
    main = plans[-1]  # (the cascade: the suffix pass; its prefix pass is one sequence of 32 rows)
    asked = hip.varlen_launch_plan(B, hq, hkv, 1, c["capacity"] - c["shared_prefix_len"], d, total_q=B, page_size=page)
    assert main["kernel"] == asked["kernel"] and main["splits"] == asked["splits"], (main, asked)
    assert main["kernel"].startswith(f"ffpa_fwd_m16_paged_kernel<bf16, {d}, NT> (GQA heads packed into rows)"), name
    assert main["splits"] > 1 and main["kernel"].endswith("+ ffpa_varlen_merge_kernel"), name
    eff = R.effective_lens(c)
    _note(f"serving {variant}", "bf16", R.check(out, lse, ref, v=R.visible_values(vview_w, eff, t["table"]), dtype="bf16", name=name))
    R.check_cache(t["k_storage"], ks_w, t["k_cache"], kview_w, rotated, c["rotary_dim"], name)
    R.check_cache(t["v_storage"], vs_w, t["v_cache"], vview_w, [], 0, name)
    del t, ref, kview_w, vview_w, ks_w, vs_w
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- c. layouts
@pytest.mark.parametrize("page", [128, 0])
@pytest.mark.parametrize("layout", R.POOL_LAYOUTS)
def test_every_layout_through_attention_append_and_cascade(hip, layout, page):
  """K / V as halves of one tensor (either axis), head-major storage, rows wider than the head dim, a batch-padded cache; q / k / v as slices of a fused QKV
  buffer; the block table as a column range of a wider one and with a non-unit column stride; the lengths as ``buf[::2]``.  Paged and contiguous (where
  ``kv[:, 0]`` of ``[B, 2, capacity, Hkv, D]`` and the head-major cache are not viewable flat: the documented copy, made after the in-place append)."""
  for i, (entry, rd) in enumerate((("plain", 0), ("append", 0), ("append", 64), ("cascade", 32))):
    for tl in (("wide_slice", "transposed") if page else ("plain",)):
      snew = None if entry == "plain" else 3
      P = (256 if page else 70) if entry == "cascade" else 0
      c = make_case(D=192, dtype=("bf16", "fp16")[i % 2], page=page, heads=(8, 2), layout=layout, table_layout=tl, lens_strided=True, fused_qkv=True, entry=entry, Sq=3, Snew=snew,
                    rotary_dim=rd, interleaved=bool(i % 2), causal=True, lens=[300, 511, 700], shared_prefix_len=P, num_splits=(0, 1, 2, 0)[i], seed=40 + i,
                    capacity=None if page else 1000)
      plans = run_case(hip, c)
      assert plans and all("kernel" in p for p in plans), plans


def test_layouts_outside_the_contract_are_copied_for_attention_and_refused_for_the_append(hip):
  """A cache whose head dim has stride 2: attention still answers right (the host layer copies); the append, which writes in place, raises ValueError."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  c = make_case(D=128, page=64, heads=(4, 2), lens=[100, 257], Sq=2, causal=True)
  t = R.materialize(c, "cuda")
  wide_k, wide_v = (torch.zeros((*x.shape[:-1], 256), dtype=x.dtype, device="cuda") for x in (t["k_cache"], t["v_cache"]))
  kc, vc = wide_k[..., ::2], wide_v[..., ::2]
  kc.copy_(t["k_cache"]), vc.copy_(t["v_cache"])
  out, lse = ffpa_attn_with_kvcache(t["q"], kc, vc, cache_seqlens=t["lens"], block_table=t["table"], causal=True, return_softmax_lse=True)
  R.check(out, lse, R.attend(t["q"], kc, vc, c["lens"], t["table"], True), v=R.visible_values(vc, c["lens"], t["table"]), dtype="bf16", name="stride-2 head dim")
  new = torch.randn((2, 1, 2, 128), dtype=torch.bfloat16, device="cuda")
  before = wide_k.clone()
  with pytest.raises(ValueError, match="written in place"):
    ffpa_attn_with_kvcache(t["q"], kc, vc, k=new, v=new, cache_seqlens=t["lens"], block_table=t["table"])
  torch.cuda.synchronize()
  assert torch.equal(wide_k.view(torch.int16), before.view(torch.int16))


# ----------------------------------------------------------------------------- d. past 2^31 elements and 2^32 bytes
def test_pool_pages_past_4_gib(hip):
  """A pool of 1100 pages of 256 keys x 8 KV heads x D 1024 (4 MiB per page: 4.3 GiB per tensor) whose used pages are the highest ids, every other page NaN:
  paged attention (NT and plain, unsplit and three ranges), the append with rotary (the write lands at the high offset and nowhere else: the whole pool against
  the reference's), the cascade.  Peak allocation ~ 24 GiB (two pools, their reference clones, one mask)."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_cascade

  n_pages, page, hkv, hq, d, dtype = 1100, 256, 8, 8, 1024, torch.bfloat16
  lens, pps, B, sq = [700, 1500, 1027], 7, 3, 2
  g = torch.Generator(device="cuda").manual_seed(9)
  pk = torch.full((n_pages, page, hkv, d), float("nan"), dtype=dtype, device="cuda")
  pv = torch.full((n_pages, page, hkv, d), float("nan"), dtype=dtype, device="cuda")
  ids = (n_pages - 1 - torch.randperm(B * pps, generator=torch.Generator().manual_seed(9))).to(torch.int32).view(B, pps)
  ids[:, 0] = ids[0, 0]  # the first page (256 keys) is shared: the cascade's prefix
  table = ids.cuda()
  low = int(ids.min())
  assert low * pk.stride(0) >= 2 ** 31 and low * pk.stride(0) * 2 >= 2 ** 32, "the used pages must lie past 2^31 elements / 2^32 bytes"
  pk[low:] = torch.randn((n_pages - low, page, hkv, d), dtype=dtype, device="cuda", generator=g)
  pv[low:] = torch.randn((n_pages - low, page, hkv, d), dtype=dtype, device="cuda", generator=g)
  used = torch.tensor(lens, dtype=torch.int32, device="cuda")
  q = torch.randn((B, sq, hq, d), dtype=dtype, device="cuda", generator=g)
  ref = R.attend(q, pk, pv, lens, table, True)
  vstat = R.visible_values(pv, lens, table)
  cu_q = torch.arange(0, (B + 1) * sq, sq, dtype=torch.int32, device="cuda")
  for flag in (hip.FLAG_KV_STREAM, hip.FLAG_NO_KV_STREAM):
    for splits in (1, 3):
      plan = {}
      o, lse = hip.varlen_forward(q.view(B * sq, hq, d), pk, pv, cu_q, None, sq, pps * page, True, d ** -0.5, seqused_k=used, block_table=table, num_splits=splits,
                                  flags=flag | (hip.FLAG_FORCE_SPLITS if splits > 1 else 0), plan_out=plan)
      assert plan["splits"] == splits and ((", NT" in plan["kernel"]) == (flag == hip.FLAG_KV_STREAM)), plan
      _note("paged > 4 GiB", dtype, R.check(o.view(B, sq, hq, d), lse.view(hq, B, sq).permute(1, 0, 2), ref, v=vstat, dtype=dtype, name=f"high pages {plan}"))
  # the append with rotary, then the cascade over the appended cache
  want_k, want_v = pk.clone(), pv.clone()
  ang = torch.rand((pps * page, d // 4), dtype=torch.float64, device="cuda", generator=g) * 6.283185307179586
  cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
  nk, nv = (torch.randn((B, sq, hkv, d), dtype=dtype, device="cuda", generator=g) for _ in range(2))
  q_rot, eff, rotated = R.append(want_k, want_v, nk, nv, lens, table, cos, sin, False, True, q=q)
  ref2 = R.attend(q_rot.to(dtype), want_k, want_v, eff, table, True)
  out, lse = ffpa_attn_with_kvcache(q, pk, pv, k=nk, v=nv, rotary_cos=cos, rotary_sin=sin, cache_seqlens=used, block_table=table, causal=True, rotary_interleaved=False,
                                    return_softmax_lse=True)
  _note("append > 4 GiB", dtype, R.check(out, lse, ref2, v=vstat, dtype=dtype, name="append at high pages"))
  R.check_cache(pk, want_k, pk, want_k, rotated, d // 2, "K pool after the append")
  R.check_cache(pv, want_v, pv, want_v, [], 0, "V pool after the append")
  assert all(p >= low for p, _ in rotated)
  del want_k, want_v
  torch.cuda.empty_cache()
  used2 = torch.tensor(eff, dtype=torch.int32, device="cuda")
  ref3 = R.attend(q, pk, pv, eff, table, True)
  out, lse = ffpa_attn_with_kvcache_cascade(q, pk, pv, cache_seqlens=used2, block_table=table, shared_prefix_len=page, causal=True, cascade=True, return_softmax_lse=True)
  _note("cascade > 4 GiB", dtype, R.check(out, lse, ref3, v=vstat, dtype=dtype, name="cascade at high pages"))
  del pk, pv
  torch.cuda.empty_cache()


def test_contiguous_cache_and_packed_keys_past_2_31_elements(hip):
  """A contiguous cache [34, 8192, 8, 1024] (2.3e9 elements, 4.6 GiB per tensor) in which only the last two slabs hold keys, the others NaN: attention, the
  append with rotary (whole cache against the reference's), and the same memory as a PACKED call whose last sequences start past row 2^31 / (Hkv D).
  Peak allocation ~ 24 GiB."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  B, cap, hkv, hq, d, dtype, sq = 34, 8192, 8, 16, 1024, torch.bfloat16, 2
  g = torch.Generator(device="cuda").manual_seed(10)
  kc = torch.full((B, cap, hkv, d), float("nan"), dtype=dtype, device="cuda")
  vc = torch.full((B, cap, hkv, d), float("nan"), dtype=dtype, device="cuda")
  lens = [0] * (B - 2) + [1500, 700]
  assert (B - 2) * kc.stride(0) >= 2 ** 31 and (B - 2) * kc.stride(0) * 2 >= 2 ** 32, "the last two slabs must start past 2^31 elements / 2^32 bytes"
  for b in (B - 2, B - 1):  # (64 rows of data past each length: the packed call below reads them as a sequence of its own)
    kc[b, :lens[b] + 64] = torch.randn((lens[b] + 64, hkv, d), dtype=dtype, device="cuda", generator=g)
    vc[b, :lens[b] + 64] = torch.randn((lens[b] + 64, hkv, d), dtype=dtype, device="cuda", generator=g)
  used = torch.tensor(lens, dtype=torch.int32, device="cuda")
  q = torch.randn((B, sq, hq, d), dtype=dtype, device="cuda", generator=g)
  vstat = R.visible_values(vc, lens)
  out, lse = ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=used, causal=True, return_softmax_lse=True)
  _note("contiguous > 2^31", dtype, R.check(out, lse, R.attend(q, kc, vc, lens, None, True), v=vstat, dtype=dtype, name="contiguous cache, last slabs"))
  # the same memory as a packed call: sequence 0 spans the NaN slabs and has no query row; the two that have rows start past 2^31 elements
  T = 1 + sq
  cu_k = torch.tensor([0, (B - 2) * cap, (B - 2) * cap + lens[B - 2], (B - 2) * cap + lens[B - 2] + 64], dtype=torch.int32, device="cuda")
  cu_q = torch.tensor([0, 0, 1, T], dtype=torch.int32, device="cuda")
  assert int(cu_k[-3]) * hkv * d >= 2 ** 31 and int(cu_k[-3]) * hkv * d * 2 >= 2 ** 32  # (both sequences that have rows)
  qp = q[B - 1, :1].expand(T, hq, d).contiguous()
  o, l = hip.varlen_forward(qp, kc.view(B * cap, hkv, d), vc.view(B * cap, hkv, d), cu_q, cu_k, sq, int(cu_k[1]), False, d ** -0.5)
  ref_a = R.attend(qp[None, :1], kc[B - 2:B - 1], vc[B - 2:B - 1], [lens[B - 2]])
  flat_k, flat_v = kc.view(1, B * cap, hkv, d)[:, int(cu_k[2]):int(cu_k[3])], vc.view(1, B * cap, hkv, d)[:, int(cu_k[2]):int(cu_k[3])]
  ref_b = R.attend(qp[None, 1:], flat_k, flat_v, [64])
  _note("packed > 2^31", dtype, R.check(o[None, :1], l[None, :, :1], ref_a, v=vstat, dtype=dtype, name="packed, sequence 1"))
  _note("packed > 2^31", dtype, R.check(o[None, 1:], l[None, :, 1:], ref_b, v=vstat, dtype=dtype, name="packed, sequence 2"))
  # the append (+ rotary) into the last slabs
  want_k, want_v = kc.clone(), vc.clone()
  ang = torch.rand((cap, 8), dtype=torch.float64, device="cuda", generator=g) * 6.283185307179586
  cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
  nk, nv = (torch.randn((B, sq, hkv, d), dtype=dtype, device="cuda", generator=g) for _ in range(2))
  q_rot, eff, rotated = R.append(want_k, want_v, nk, nv, lens, None, cos, sin, True, True, q=q)
  # (every sequence appends: the NaN slabs receive their two keys at rows 0 and 1 — and attend over them)
  ref2 = R.attend(q_rot.to(dtype), want_k, want_v, eff, None, True)
  out, lse = ffpa_attn_with_kvcache(q, kc, vc, k=nk, v=nv, rotary_cos=cos, rotary_sin=sin, cache_seqlens=used, causal=True, return_softmax_lse=True)
  _note("append > 2^31", dtype, R.check(out, lse, ref2, v=R.visible_values(want_v, eff), dtype=dtype, name="append into the last slabs"))
  R.check_cache(kc, want_k, kc, want_k, rotated, 16, "K cache after the append")
  R.check_cache(vc, want_v, vc, want_v, [], 0, "V cache after the append")
  del kc, vc, want_k, want_v
  torch.cuda.empty_cache()


def test_merge_states_past_2_31_elements(hip):
  """ffpa_merge_attn_states with T x H x D = 32896 x 64 x 1024 > 2^31 (4 GiB per state, 12 GiB in all; the last 64 tokens lie past 2^32 bytes): float64 on the first and last 64 tokens and a strided
  sample in between."""
  from ffpa_attn_amd import ffpa_merge_attn_states

  T, H, D, dtype = 32896, 64, 1024, torch.bfloat16
  assert T * H * D >= 2 ** 31 and (T - 64) * H * D * 2 >= 2 ** 32
  g = torch.Generator(device="cuda").manual_seed(12)
  o_a = torch.randn((T, H, D), dtype=dtype, device="cuda", generator=g)
  o_b = torch.randn((T, H, D), dtype=dtype, device="cuda", generator=g)
  lse_a, lse_b = (torch.randn((H, T), dtype=torch.float32, device="cuda", generator=g) * 3 for _ in range(2))
  lse_a[:, -3], lse_b[:, -2] = float("-inf"), float("-inf")
  lse_a[:, -1] = lse_b[:, -1] = float("-inf")
  o, lse = ffpa_merge_attn_states(o_a, lse_a, o_b, lse_b)
  rows = torch.cat((torch.arange(64), torch.arange(64, T - 64, 509), torch.arange(T - 64, T))).cuda()
  la, lb = lse_a[:, rows].double().t(), lse_b[:, rows].double().t()  # [rows, H]
  m = torch.maximum(la, lb)
  live = torch.isfinite(m)
  ms = torch.where(live, m, torch.zeros_like(m))
  wa, wb = torch.exp(la - ms), torch.exp(lb - ms)
  den = torch.where(live, wa + wb, torch.ones_like(wa))
  want = (wa[..., None] * torch.nan_to_num(o_a[rows].double()) + wb[..., None] * torch.nan_to_num(o_b[rows].double())) / den[..., None]
  want = torch.where(live[..., None], want, torch.zeros_like(want))
  got = o[rows].double()
  assert torch.isfinite(got).all()
  # one rounding of an fp32 result to bf16: half the spacing of bf16 at the result (+ 1 % and 1e-6 for the fp32 arithmetic in front of it)
  assert ((got - want).abs() <= 0.5 * R.ulp_of(want, dtype) * 1.01 + 1e-6).all(), (got - want).abs().max().item()
  want_lse = torch.where(live, ms + torch.log(den), torch.full_like(m, float("-inf")))
  gl = lse[:, rows].double().t()
  assert torch.equal(torch.isneginf(gl), torch.isneginf(want_lse))
  fin = torch.isfinite(want_lse)
  assert torch.allclose(gl[fin], want_lse[fin], atol=R.LSE_ATOL, rtol=R.LSE_RTOL)
  del o_a, o_b, o
  torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- the edges of the contract
_EDGES = {
  "lengths 0, negative, the capacity, above it": dict(lens=[0, -4, 256, 300, 17], pages_per_seq=4, page=64, Sq=2, causal=True),
  "more tokens than keys under causal": dict(lens=[2, 0, 5, 200], Sq=6, causal=True, heads=(4, 4)),
  "Snew = 0": dict(entry="append", Snew=0, lens=[10, 200], Sq=2, rotary_dim=32, causal=True),
  "an append across a page boundary and across the capacity": dict(entry="append", Snew=5, Sq=5, lens=[62, 126, 253, 256, 300, -2], pages_per_seq=4, page=64, rotary_dim=64,
                                                                   causal=True, fused_qkv=True),
  "contiguous: an append across the capacity": dict(entry="append", Snew=4, Sq=4, lens=[97, 100, 0, 98], page=0, capacity=100, rotary_dim=16, causal=True, seqlen_ro=100),
  "rotary_dim 16 of D 320, NeoX": dict(entry="append", Snew=2, Sq=2, D=320, rotary_dim=16, interleaved=False, lens=[100, 64]),
  "rotary_dim D / 2 of D 320": dict(entry="append", Snew=2, Sq=2, D=320, rotary_dim=160, interleaved=False, lens=[100, 64], causal=True),
  "rotary_dim D of D 576, interleaved": dict(entry="append", Snew=3, Sq=1, D=576, rotary_dim=576, lens=[100, 64], dtype="fp16"),
  "rotary_dim D of D 576, NeoX": dict(entry="append", Snew=1, Sq=3, D=576, rotary_dim=576, interleaved=False, lens=[100, 64], causal=True),
  "ids outside the pool past the last used page": dict(lens=[1, 64, 65, 300], bad_unused_ids=True, pages_per_seq=8, Sq=2, causal=True),
  "ids outside the pool in used entries (the clamp)": dict(lens=[300, 10], bad_used_id=True, seed=1),
  "ids outside the pool in used entries (the clamp), above": dict(lens=[300, 10], bad_used_id=True, seed=2),
  "two sequences sharing prefix pages": dict(lens=[700, 300, 5], share_prefix_pages=True, page=128, num_splits=2),
  "B = 1, Hq = Hkv = 1": dict(lens=[777], heads=(1, 1), D=64, Sq=3, causal=True),
  "group 16": dict(lens=[400, 3], heads=(16, 1), D=256, Sq=2, causal=True, num_splits=5),
  "group 16, one token, cascade": dict(entry="cascade", lens=[400, 300], heads=(16, 1), D=256, shared_prefix_len=128, page=128),
}


@pytest.mark.parametrize("edge", list(_EDGES))
def test_edges_of_the_contract(hip, edge):
  plans = run_case(hip, make_case(**dict(_EDGES[edge])))
  print(f"[edge] {edge}: {plans}")


# ----------------------------------------------------------------------------- the seeded sweep
_EXTRA = int(os.environ.get("FFPA_KVCACHE_SWEEP_SEEDS", "0"))  # a long run: this many seeds more, after the committed ones


@pytest.mark.parametrize("seed", list(R.SWEEP_SEEDS) + list(range(len(R.SWEEP_SEEDS), len(R.SWEEP_SEEDS) + _EXTRA)))
def test_kvcache_family_sweep(hip, seed):
  """A drawn case (entry point, layout, page size, dtype, head dim, heads, batch, tokens, lengths, causal, num_splits, KV stream flag, LSE): output and LSE against
  float64 under the allowance, the cache's storage after an append, no NaN where a key is visible.  A failure names its seed and prints the case."""
  run_case(hip, R.draw_case(seed))


def test_zz_report_worst_error_over_allowance():
  """Not a check of the kernels: prints, per entry point and dtype, the worst error / allowance this run saw (profiles/r10_kvcache_serving.md)."""
  for (entry, dtype), ratio in sorted(RATIOS.items()):
    print(f"[ratio] {entry:24s} {dtype}: {ratio:.3f}")
  assert all(r <= 1.0 for r in RATIOS.values())
