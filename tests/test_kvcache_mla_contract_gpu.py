"""``ffpa_attn_with_kvcache_mla`` on the GPU where tests/test_kvcache_mla_gpu.py has not looked: the NT build, partial last chunks of a packed group and Sq > 64,
pages of 128 / 256 keys behind a shuffled table, the append at its edges, the layout contract, offsets past 2^31 elements / 2^32 bytes, the library's own plan
at a serving size, torch.compile and a side stream, and the model-like values of tests/model_values.py laid out as latent rows.

Every case: D = 576, head_dim_v = 512, scale 1 / sqrt(192) (the model-like values: 1 / sqrt(576), the scale their families are built for); pools hold NaN wherever
no visible key lives; the reference is float64 attention on the gathered latent rows (``kvcache_ref.attend`` on (pool, pool), value columns ``[:512]``), appends
``kvcache_ref.append`` on a clone of the whole storage; outputs are held to ``kvcache_ref.check`` with the case's own statistics, LSE to ``LSE_ATOL`` / ``LSE_RTOL``,
caches to ``check_cache`` / integer equality of the whole storage.  No tolerance of its own.  Every launch's plan is read through ``plan_out``.

Worst error / allowance per section and dtype, the plans of (a) and (g) and the wall times on MI355X: profiles/r17_mla_contract.md (the last test prints the ratios)."""

import math

import pytest
import torch

import kvcache_mla_cases as C
import kvcache_ref as R
from test_fwd_gpu import hip  # noqa: F401  (fixture)
from test_kvcache_mla_gpu import LENS, SCALE, _case, _launches

pytestmark = pytest.mark.gpu

D, DV = C.D, C.DV
NAN = float("nan")
BAD_IDS = (-1, None, 2 ** 31 - 1, -(2 ** 31))  # (None: num_pages) what table entries past a sequence's last page hold under ``bad_unused``
RATIOS: dict = {}  # (section, dtype) -> worst error / allowance seen by this run


def _note(section, dtype, ratio):
  key = (section, R._dt(dtype))
  RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
  return ratio


def _kernel(dtype, nt=False):
  return f"ffpa_fwd_m16_mla_kernel<{R._dt(dtype)}, 576, dv=512" + (", NT>" if nt else ">")


# ----------------------------------------------------------------------------- cases
def _pool(lens, hq, hkv, sq, dtype, *, page=64, pps=None, seed=0, contiguous=False, layout="batch_padded", bad_unused=False, bad_used=(), table_layout="plain",
          lens_strided=False, fused=False, rows=None, q=None):
  """A latent cache in the vocabulary of test_kvcache_mla_gpu._case, every axis open: ``page`` keys per page (contiguous: the slab's capacity), ``pps`` pages per
  sequence, the pool in ``layout`` (kvcache_ref.lay_out_cache's, or "offset": ``storage[3:]``), the table / lengths in their strided forms, ``q`` (and the new rows
  ``kv``) as slices of one fused ``[B, Sq, Hq + Hkv, D]`` buffer.  Ids 0 and num_pages - 1 belong to no sequence: ``bad_used = [(b, j, id)]`` puts an id outside the
  pool into a USED entry, which reads and writes the clamped page.  ``rows [B, Hkv, L, D]`` (CPU): the latent rows instead of randn.  NaN wherever no key lives."""
  g = torch.Generator(device="cuda").manual_seed(2000 + seed)
  tdt = R.TORCH_DTYPE[R._dt(dtype)]
  B = len(lens)
  if contiguous:
    n_pages, ids, cap = B, None, page
  else:
    pps = pps or -(-max(max(lens), 1) // page) + 1
    n_pages, cap = B * pps + 3, pps * page
    ids = (1 + torch.randperm(n_pages - 2, generator=torch.Generator().manual_seed(seed))[: B * pps]).to(torch.int32).view(B, pps)
    for b, j, bad in bad_used:
      ids[b, j] = bad
  eff = [min(max(n, 0), cap) for n in lens]
  kc = torch.randn((n_pages, page, hkv, D), generator=g, device="cuda", dtype=tdt)
  seen = torch.zeros((n_pages, page), dtype=torch.bool)
  for b, n in enumerate(eff):
    j = torch.arange(n)
    slab = torch.full((n,), b) if contiguous else ids[b].long()[j // page].clamp(0, n_pages - 1)
    seen[slab, j % page] = True
    if rows is not None:
      kc[slab.cuda(), (j % page).cuda()] = rows[b].transpose(0, 1).to(device="cuda", dtype=tdt)
    if bad_unused and not contiguous:
      for jj in range(-(-n // page), pps):
        bad = BAD_IDS[(b + jj) % 4]
        ids[b, jj] = n_pages if bad is None else bad
  kc[~seen.cuda()] = NAN
  if layout == "offset":
    storage = torch.full((n_pages + 3, page, hkv, D), NAN, dtype=tdt, device="cuda")
    pool = storage[3:]
    pool.copy_(kc)
  else:
    pool, _, storage, _ = R.lay_out_cache(kc, kc, layout, fill=NAN)
  table = None if contiguous else R.lay_out_table(ids.cuda(), table_layout)
  kv = None
  if fused:
    buf = torch.randn((B, sq, hq + hkv, D), generator=g, device="cuda", dtype=tdt)
    q, kv = buf[:, :, :hq], buf[:, :, hq:]
  elif q is None:
    q = torch.randn((B, sq, hq, D), generator=g, device="cuda", dtype=tdt)
  t = dict(q=q, kv=kv, pool=pool, storage=storage, table=table, lens=R.lay_out_lens(torch.tensor(lens, dtype=torch.int32, device="cuda"), lens_strided),
           lens_list=list(lens), dtype=R._dt(dtype), sq=sq, heads=(hq, hkv), cap=cap, num_pages=n_pages)
  t["vstat"] = R.visible_values(pool[..., :DV], lens, table)
  return t


def _reference(t, causal, scale=SCALE, lens=None, pool=None):
  pool = t["pool"] if pool is None else pool
  o, lse, pmax, p2sum = R.attend(t["q"], pool, pool, t["lens_list"] if lens is None else lens, t["table"], causal, scale)
  return o[..., :DV].contiguous(), lse, pmax, p2sum


def _call(hip, t, causal=False, *, scale=SCALE, num_splits=0, flags=0, lens=None, kv=None, pool=None):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla(t["q"], t["pool"] if pool is None else pool, DV, kv=kv, cache_seqlens=t["lens"] if lens is None else lens,
                                          block_table=t["table"], softmax_scale=scale, causal=causal, num_splits=num_splits, return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith(_kernel(t["dtype"])[:-1]), plans
  assert out.shape == (len(t["lens_list"]), t["sq"], t["heads"][0], DV) and out.is_contiguous()
  return out, lse, plans[0]


def _check(hip, section, t, causal, ref=None, *, scale=SCALE, vstat=None, **kw):
  """One launch against float64 -> ``(out, lse, plan)``; the ratio is printed before it is judged and kept for the report."""
  ref = _reference(t, causal, scale) if ref is None else ref
  out, lse, plan = _call(hip, t, causal, scale=scale, **kw)
  name = f"{section}: {t['dtype']} heads {t['heads']} Sq {t['sq']} causal={causal} lens {t['lens_list'][:12]} {({k: v for k, v in kw.items() if k in ('num_splits', 'flags')})} -> {plan}"
  ratio = _note(section, t["dtype"], R.check(out, lse, ref, v=t["vstat"] if vstat is None else vstat, dtype=t["dtype"], name=name))
  print(f"[mla-contract] {ratio:.3f} {name}")
  return out, lse, plan


def _same_bits(a, b):
  return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------- a. the NT build
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq", [16, 128])
@pytest.mark.parametrize("sq", [1, 3])
def test_a_nt_build_against_float64_and_the_plain_build_bit_for_bit(hip, dtype, hq, sq):
  """FLAG_KV_STREAM on the ten-length batch, num_splits 1, three forced ranges and the library's own: the plan names the NT build, the output is float64's to the
  allowance and, unsplit, the same bits as the plain build's (FLAG_NO_KV_STREAM) — the non-temporal hint changes how a tile is fetched, not what."""
  causal = sq > 1
  t = _case(LENS, hq, 1, sq, dtype, seed=hq + sq)
  ref = _reference(t, causal)
  for ns in (1, 3, 0):
    out, lse, plan = _check(hip, "a NT", t, causal, ref, num_splits=ns, flags=hip.FLAG_KV_STREAM | (hip.FLAG_FORCE_SPLITS if ns > 1 else 0))
    assert plan["kernel"].startswith(_kernel(dtype, nt=True)), plan
    assert ns == 0 or plan["splits"] == ns, plan
    assert ("ffpa_varlen_merge_kernel" in plan["kernel"]) == (plan["splits"] > 1), plan
    print(f"[plan a] {dtype} Hq {hq} Sq {sq} num_splits {ns}: {plan}")
    if ns == 1:
      plain = _call(hip, t, causal, num_splits=1, flags=hip.FLAG_NO_KV_STREAM)
      assert ", NT" not in plain[2]["kernel"] and plain[2]["splits"] == 1, plain[2]
      assert _same_bits((out, lse), plain), f"NT and plain differ: {int((out != plain[0]).sum())} outputs, {int((lse != plain[1]).sum())} LSEs"


# ----------------------------------------------------------------------------- b. row chunks
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", C.ROW_SHAPES)
def test_b_partial_last_chunks_and_more_than_64_tokens(hip, dtype, hq, hkv, sq):
  """group x Sq rows that are no multiple of 64 (the last chunk's rows >= Nq are clamped for the Q fetch and skipped at the O / LSE / workspace stores), Sq > 64
  packed (a chunk holds part of a head's tokens: row / ntok, row % ntok and causal_row_mod) and unpacked (several row tiles, reversed under causal); lengths 0 ...
  300 with Sq - 1, Sq, Sq + 1; the library's count and two and three forced ranges."""
  group, lens = hq // hkv, C.row_lens(sq)
  t = _pool(lens, hq, hkv, sq, dtype, seed=hq + sq)
  want_tiles = C.row_tiles(hq, hkv, sq)
  assert len(hip.mla_row_chunks(group, sq)) == want_tiles
  for causal in (False, True):
    ref = _reference(t, causal)
    for ns in (0, 2, 3):
      out, lse, plan = _check(hip, "b row chunks", t, causal, ref, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS if ns else 0)
      assert plan["block_rows"] == 64 and plan["block_keys"] == 32 and plan["row_tiles"] == want_tiles, plan
      assert ns == 0 or plan["splits"] == ns, plan
      assert plan["workgroups"] == len(lens) * (hkv if group > 1 else hq) * want_tiles * plan["splits"], plan
      assert ("packed into rows" in plan["kernel"]) == (group > 1) and ("chunked" in plan["kernel"]) == (group > 1 and group * sq > 64), plan
      assert ("ffpa_varlen_merge_kernel" in plan["kernel"]) == (plan["splits"] > 1), plan
      for b, n in enumerate(lens):
        hidden = sq if not causal and n == 0 else max(sq - n, 0) if causal else 0  # the tokens whose position lies below key 0
        assert (out[b, :hidden] == 0).all() and torch.isneginf(lse[b, :, :hidden]).all(), (b, n)
        assert torch.isfinite(lse[b, :, hidden:]).all(), (b, n)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_b_no_pack_gqa_keeps_one_workgroup_per_query_head(hip, dtype):
  t = _case(LENS, 16, 1, 3, dtype, seed=19)
  out, lse, plan = _check(hip, "b no pack", t, True, flags=hip.FLAG_NO_PACK_GQA, num_splits=1)
  assert "packed" not in plan["kernel"] and plan["row_tiles"] == 1 and plan["workgroups"] == len(LENS) * 16, plan


# ----------------------------------------------------------------------------- c. pages of 128 and 256
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("page", [128, 256])
def test_c_pages_of_four_and_eight_tiles_behind_a_shuffled_table(hip, dtype, page):
  """tiles_per_page 4 and 8: the page lookahead crosses a page every 4th / 8th tile, forced ranges start in the middle of a page, and the table entries past a
  sequence's last page hold ids outside the pool (-1, num_pages, INT_MAX, INT_MIN), which are never read."""
  lens = [0, 1, 127, 128, 129, 255, 256, 257, 300, 700]
  for hq in (16, 128):
    for sq in (1, 3):
      t = _pool(lens, hq, 1, sq, dtype, page=page, seed=page + hq + sq, bad_unused=True)
      tab = t["table"].cpu()
      assert all(int(tab[b, j]) < 0 or int(tab[b, j]) >= t["num_pages"] for b, n in enumerate(lens) for j in range(-(-n // page), tab.size(1)))
      ref = _reference(t, sq > 1)
      for ns in (1, 0, 3, 5):
        out, lse, plan = _check(hip, f"c page {page}", t, sq > 1, ref, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS if ns > 1 else 0)
        assert ns == 0 or plan["splits"] == ns, plan
        assert plan["row_tiles"] == math.ceil(hq * sq / 64), plan


# ----------------------------------------------------------------------------- d. the append at its edges
def _append_case(kind, snew, dtype, seed=0):
  page, pps = {"page64": (64, 4), "page256": (256, 2), "contiguous": (128, None)}[kind]
  cap = page * pps if pps else page
  lens = list(dict.fromkeys([cap - 1, cap, cap + 5, -4, page - 2, page - 1]))
  return _pool(lens, 16, 1, snew, dtype, page=page, pps=pps, contiguous=pps is None, seed=seed + snew, fused=True), cap


def _append_and_check(hip, section, t, snew, causal=True, *, lens_arg=None, lens_list=None, kv=None):
  """``kv=`` on a clone of the storage against ``kvcache_ref.append`` on another: used lengths, the whole storage as integers, exactly the kept rows changed,
  ``cache_seqlens`` untouched, the output float64's, and the same bits once more over the written cache without ``kv=``.  -> the written pool view, the plan."""
  lens_list = t["lens_list"] if lens_list is None else lens_list
  kv = t["kv"] if kv is None else kv
  got_storage, want_storage = t["storage"].clone(), t["storage"].clone()
  got_pool, want_pool = R.reviewed(t["pool"], t["storage"], got_storage), R.reviewed(t["pool"], t["storage"], want_storage)
  _, used, _ = R.append(want_pool, want_pool, kv, kv, lens_list, t["table"])
  cap = t["cap"]
  assert used == [min(max(n, 0) + snew, cap) for n in lens_list]
  kept = sum(max(min(max(n, 0) + snew, cap) - min(max(n, 0), cap), 0) for n in lens_list)
  before = t["lens"].clone()
  out, lse, plan = _call(hip, t, causal, kv=kv, pool=got_pool, lens=lens_arg)
  torch.cuda.synchronize()
  assert torch.equal(t["lens"], before), "cache_seqlens was modified"
  R.check_cache(got_storage, want_storage, got_pool, want_pool, [], 0, f"{section}: the cache after the append")
  changed = (want_storage.view(torch.int16) != t["storage"].view(torch.int16)).any(dim=-1).sum().item()
  assert changed == kept * t["heads"][1], (changed, kept)  # (NaN rows became data; rows at or past the capacity went nowhere)
  ref = _reference(t, causal, lens=used, pool=want_pool)
  vstat = R.visible_values(want_pool[..., :DV], used, t["table"])
  name = f"{section}: {t['dtype']} Snew {snew} lens {lens_list} -> {plan}"
  ratio = _note(section, t["dtype"], R.check(out, lse, ref, v=vstat, dtype=t["dtype"], name=name))
  print(f"[mla-contract] {ratio:.3f} {name}")
  again = _call(hip, t, causal, pool=got_pool, lens=torch.tensor(used, dtype=torch.int32, device="cuda"))
  assert _same_bits((out, lse), again), "attending over the written cache without kv= gives other bits"
  return got_pool, plan


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("snew", [1, 3, 5])
@pytest.mark.parametrize("kind", ["page64", "page256", "contiguous"])
def test_d_append_at_the_capacity_at_negative_lengths_and_across_a_page(hip, dtype, snew, kind):
  """Lengths cap - 1, cap, cap + 5 (rows at or past the capacity are dropped, used = cap), -4 (acts as 0), page - 2 and page - 1 (the rows cross into the next
  page); q and kv are slices of one fused buffer."""
  t, cap = _append_case(kind, snew, dtype, seed=60)
  _append_and_check(hip, f"d append {kind}", t, snew)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_d_snew_0_is_the_plain_call_and_an_int_is_every_sequences_length(hip, dtype):
  t = _pool([100, 37, 256], 16, 1, 2, dtype, page=64, pps=5, seed=71)
  storage = t["storage"].clone()
  pool = R.reviewed(t["pool"], t["storage"], storage)
  plain = _call(hip, t, True, pool=pool)
  empty = _call(hip, t, True, pool=pool, kv=t["q"].new_empty((3, 0, 1, D)))
  assert _same_bits(plain, empty) and plain[2] == empty[2]
  assert torch.equal(storage.view(torch.int16), t["storage"].view(torch.int16))
  # cache_seqlens as a Python int: every sequence holds 100 keys
  t = _pool([100, 100, 100], 16, 1, 3, dtype, page=64, pps=3, seed=72, fused=True)
  _check(hip, "d int length", t, True, lens=100)
  _append_and_check(hip, "d int length", t, 3, lens_arg=100)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_d_used_table_entries_outside_the_pool_are_clamped_by_the_kernel_and_the_append(hip, dtype):
  """Sequence 0's second entry is -7 (page 0), sequence 1's third num_pages + 11 (the last page): attention reads the clamped page, and the appended rows — which
  land in those very entries — are written there and nowhere else."""
  n_pages = 2 * 4 + 3
  t = _pool([70, 130], 16, 1, 3, dtype, page=64, pps=4, seed=73, fused=True, bad_used=[(0, 1, -7), (1, 2, n_pages + 11)])
  assert t["num_pages"] == n_pages and int(t["table"][0, 1]) == -7 and int(t["table"][1, 2]) == n_pages + 11
  assert torch.isfinite(t["pool"][0, :6]).all() and torch.isnan(t["pool"][0, 6:]).all() and torch.isfinite(t["pool"][n_pages - 1, :2]).all()
  _check(hip, "d clamped ids", t, True)
  got_pool, _ = _append_and_check(hip, "d clamped ids", t, 3)
  assert torch.isfinite(got_pool[0, :9]).all() and torch.isnan(got_pool[0, 9:]).all() and torch.isfinite(got_pool[n_pages - 1, :5]).all()


# ----------------------------------------------------------------------------- e. layouts
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("page", [128, 0])
@pytest.mark.parametrize("layout", ["wide_row", "head_major", "batch_padded", "offset"])
def test_e_every_layout_of_the_contract_through_attention_and_the_append(hip, dtype, layout, page):
  """The pool with rows wider than D, head-major (two latent heads), batch-padded and at a nonzero storage offset; q and kv as slices of a fused buffer; the block
  table as a column range of a wider one and with a non-unit column stride; the lengths as ``buf[::2]``.  The whole owning storage is compared, so a write
  outside the view shows."""
  for tl in (("wide_slice", "transposed") if page else ("plain",)):
    t = _pool([100, 255, 300], 32, 2, 3, dtype, page=page or 384, pps=4 if page else None, contiguous=not page, layout=layout, table_layout=tl, lens_strided=True,
              fused=True, seed=80 + len(layout))
    assert not t["q"].is_contiguous() and not t["kv"].is_contiguous() and not t["lens"].is_contiguous()
    assert layout == "batch_padded" or not t["pool"].is_contiguous() or t["pool"].storage_offset() > 0
    assert page == 0 or not t["table"].is_contiguous()
    before = t["storage"].clone()
    for ns in (1, 0):
      _check(hip, f"e {layout}", t, True, num_splits=ns)
    assert torch.equal(t["storage"].view(torch.int16), before.view(torch.int16)), "attention wrote to the cache"
    _append_and_check(hip, f"e {layout}", t, 3)


@pytest.mark.parametrize("paged", [True, False])
def test_e_a_pool_outside_the_contract_is_refused_with_and_without_kv(hip, paged):
  """A latent pool whose head dim has stride 2: there is no copying fallback (the cache is read, and written, in place) — ValueError, nothing written."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  t = _pool([100, 200], 16, 1, 2, "bf16", page=64 if paged else 256, pps=4 if paged else None, contiguous=not paged, seed=90, fused=True)
  wide = torch.zeros((*t["pool"].shape[:-1], 2 * D), dtype=torch.bfloat16, device="cuda")
  pool = wide[..., ::2]
  pool.copy_(t["pool"])
  before = wide.clone()
  for kv in (None, t["kv"]):
    with pytest.raises(ValueError, match=r"kv_cache needs head-dim stride 1, strides that are multiples of 8 elements and a 16-byte aligned base \(it is read, and written, in place\)"):
      ffpa_attn_with_kvcache_mla(t["q"], pool, DV, kv=kv, cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE, causal=True)
  torch.cuda.synchronize()
  assert torch.equal(wide.view(torch.int16), before.view(torch.int16))


# ----------------------------------------------------------------------------- f. past 2^31 elements and 2^32 bytes
def test_f_latent_pool_pages_past_4_gib(hip):
  """A pool [14700, 256, 1, 576] bf16 (4.04 GiB) whose used pages are the highest ids, every other page NaN: NT and plain, unsplit and three forced ranges, then
  ``kv=`` with two rows per sequence — the whole pool against the reference's clone.  Peak allocation ~ 10 GiB (the pool, its reference clone, one comparison
  mask of 2 GiB)."""
  n_pages, page, pps, lens, sq, dtype = 14700, 256, 7, [700, 1500, 1027], 2, torch.bfloat16
  B = len(lens)
  g = torch.Generator(device="cuda").manual_seed(9)
  pool = torch.full((n_pages, page, 1, D), NAN, dtype=dtype, device="cuda")
  ids = (n_pages - 1 - torch.randperm(B * pps, generator=torch.Generator().manual_seed(9))).to(torch.int32).view(B, pps)
  low = int(ids.min())
  assert low * pool.stride(0) >= 2 ** 31 and low * pool.stride(0) * 2 >= 2 ** 32, "the used pages must lie past 2^31 elements / 2^32 bytes"
  for b, n in enumerate(lens):  # (data in the visible rows only: the rows behind a length stay NaN until the append writes them)
    j = torch.arange(n)
    pool[ids[b].long()[j // page].cuda(), (j % page).cuda()] = torch.randn((n, 1, D), dtype=dtype, device="cuda", generator=g)
  t = dict(q=torch.randn((B, sq, 16, D), dtype=dtype, device="cuda", generator=g), pool=pool, storage=pool, table=ids.cuda(),
           lens=torch.tensor(lens, dtype=torch.int32, device="cuda"), lens_list=lens, dtype="bf16", sq=sq, heads=(16, 1), cap=pps * page, num_pages=n_pages)
  t["vstat"] = R.visible_values(pool[..., :DV], lens, t["table"])
  ref = _reference(t, True)
  for flag in (hip.FLAG_KV_STREAM, hip.FLAG_NO_KV_STREAM):
    for ns in (1, 3):
      out, lse, plan = _check(hip, "f paged > 4 GiB", t, True, ref, num_splits=ns, flags=flag | (hip.FLAG_FORCE_SPLITS if ns > 1 else 0))
      assert plan["splits"] == ns and ((", NT" in plan["kernel"]) == (flag == hip.FLAG_KV_STREAM)), plan
  kv = torch.randn((B, sq, 1, D), dtype=dtype, device="cuda", generator=g)
  want = pool.clone()
  _, used, _ = R.append(want, want, kv, kv, lens, t["table"])
  ref2 = _reference(t, True, lens=used, pool=want)
  out, lse, plan = _call(hip, t, True, kv=kv)
  _note("f append > 4 GiB", dtype, R.check(out, lse, ref2, v=R.visible_values(want[..., :DV], used, t["table"]), dtype=dtype, name=f"append at high pages {plan}"))
  R.check_cache(pool, want, pool, want, [], 0, "the latent pool after the append")
  assert torch.isnan(pool[:low]).all()
  del pool, want, t, ref, ref2
  torch.cuda.empty_cache()


def test_f_contiguous_latent_cache_past_2_31_elements(hip):
  """A contiguous cache [460, 8192, 1, 576] bf16 (2.17e9 elements, 4.04 GiB) in which only the last two slabs hold keys, every other length 0: attention, then the
  append — every sequence appends, so the NaN slabs receive rows 0 and 1 and nothing else.  Peak allocation ~ 10 GiB (the cache, its reference clone, one
  comparison mask of 2 GiB)."""
  B, cap, sq, dtype = 460, 8192, 2, torch.bfloat16
  g = torch.Generator(device="cuda").manual_seed(10)
  cache = torch.full((B, cap, 1, D), NAN, dtype=dtype, device="cuda")
  lens = [0] * (B - 2) + [1500, 700]
  assert (B - 2) * cache.stride(0) >= 2 ** 31 and (B - 2) * cache.stride(0) * 2 >= 2 ** 32, "the last two slabs must start past 2^31 elements / 2^32 bytes"
  for b in (B - 2, B - 1):
    cache[b, :lens[b]] = torch.randn((lens[b], 1, D), dtype=dtype, device="cuda", generator=g)
  t = dict(q=torch.randn((B, sq, 16, D), dtype=dtype, device="cuda", generator=g), pool=cache, storage=cache, table=None,
           lens=torch.tensor(lens, dtype=torch.int32, device="cuda"), lens_list=lens, dtype="bf16", sq=sq, heads=(16, 1), cap=cap, num_pages=B)
  t["vstat"] = R.visible_values(cache[..., :DV], lens)
  out, lse, plan = _check(hip, "f contiguous > 2^31", t, True)
  assert (out[:B - 2] == 0).all() and torch.isneginf(lse[:B - 2]).all()
  kv = torch.randn((B, sq, 1, D), dtype=dtype, device="cuda", generator=g)
  want = cache.clone()
  _, used, _ = R.append(want, want, kv, kv, lens, None)
  assert used == [2] * (B - 2) + [1502, 702]
  ref2 = _reference(t, True, lens=used, pool=want)
  out, lse, plan = _call(hip, t, True, kv=kv)
  _note("f append > 2^31", dtype, R.check(out, lse, ref2, v=R.visible_values(want[..., :DV], used), dtype=dtype, name=f"append into every slab {plan}"))
  R.check_cache(cache, want, cache, want, [], 0, "the contiguous latent cache after the append")
  assert torch.isfinite(cache[:B - 2, :2]).all() and torch.isnan(cache[:B - 2, 2:]).all()
  del cache, want, t, ref2
  torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- g. the library's own choice at a serving size
@pytest.mark.parametrize("hq", [16, 128])
def test_g_decode_batch_of_serving_size_under_the_librarys_own_plan(hip, hq):
  """32 sequences of 1k ... 16k keys, one token each, pages of 64, 257 pages per sequence, bf16, no flag, num_splits = 0; every row against float64.  Hq 16: one
  reader per latent byte and 32 x 16448 x 576 x 2 B = 578 MiB >= 272 MiB: the NT build, split, with the merge.  Hq 128: two chunks are two readers: not NT.  Then
  the same batch with ``kv=`` (one row each): the whole pool checked.  Peak allocation ~ 3 GiB (a pool of 0.6 GiB in its layout, two clones, one comparison mask)."""
  B, page, pps = 32, 64, 257
  lens = [1024 + (16384 - 1024 - 1) * i // (B - 1) for i in range(B)]
  assert B * pps * page * D * 2 >= 272 << 20
  t = _pool(lens, hq, 1, 1, "bf16", page=page, pps=pps, seed=hq, fused=True)
  out, lse, plan = _check(hip, f"g serving Hq {hq}", t, False)
  print(f"[plan g] Hq {hq}: {plan}")
  assert plan["row_tiles"] == hq // 64 or hq < 64 and plan["row_tiles"] == 1, plan
  if hq == 16:
    assert plan["kernel"].startswith(_kernel("bf16", nt=True) + " (heads packed into rows)"), plan
    assert plan["splits"] > 1 and plan["kernel"].endswith("+ ffpa_varlen_merge_kernel"), plan
  else:
    assert ", NT" not in plan["kernel"] and "chunked" in plan["kernel"], plan
  assert plan["workgroups"] == B * plan["row_tiles"] * plan["splits"], plan
  _, plan_kv = _append_and_check(hip, f"g serving Hq {hq} append", t, 1, causal=False)
  print(f"[plan g] Hq {hq}, kv=: {plan_kv}")
  assert plan_kv == plan, (plan_kv, plan)  # (the append in front changes nothing of the attention launch)
  torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- h. host paths
def test_h_under_torch_compile_fullgraph(hip):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  t = _pool([70, 0, 129], 16, 1, 3, "fp16", page=64, pps=4, seed=88, fused=True)

  def f(q, pool, kv, lens, table):
    o, lse = ffpa_attn_with_kvcache_mla(q, pool, DV, kv=kv, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, causal=True, return_softmax_lse=True)
    return o * 2, lse

  s_eager, s_compiled = t["storage"].clone(), t["storage"].clone()
  p_eager, p_compiled = R.reviewed(t["pool"], t["storage"], s_eager), R.reviewed(t["pool"], t["storage"], s_compiled)
  with _launches(hip) as plans:
    eager = f(t["q"], p_eager, t["kv"], t["lens"], t["table"])
  assert len(plans) == 1 and plans[0]["kernel"].startswith(_kernel("fp16")[:-1]), plans
  compiled = torch.compile(f, fullgraph=True)(t["q"], p_compiled, t["kv"], t["lens"], t["table"])
  torch.cuda.synchronize()
  assert _same_bits(eager, compiled)
  assert torch.equal(s_eager.view(torch.int16), s_compiled.view(torch.int16)) and not torch.equal(s_eager.view(torch.int16), t["storage"].view(torch.int16))
  used = [73, 3, 132]
  want = t["storage"].clone()
  wp = R.reviewed(t["pool"], t["storage"], want)
  R.append(wp, wp, t["kv"], t["kv"], t["lens_list"], t["table"])
  R.check_cache(s_compiled, want, p_compiled, wp, [], 0, "the cache written under torch.compile")
  _note("h compile", "fp16", R.check((compiled[0].double() / 2).to(torch.float16), compiled[1], _reference(t, True, lens=used, pool=wp),
                                     v=R.visible_values(wp[..., :DV], used, t["table"]), dtype="fp16", name="torch.compile"))


@pytest.mark.parametrize("num_splits", [1, 3])
def test_h_a_side_stream_gives_the_bits_of_the_current_stream(hip, num_splits):
  """Append + attention (+ the merge and its scratch, with three forced ranges) enqueued on a stream that is not the default one."""
  t = _pool([5, 200, 1000, 64], 16, 1, 2, "bf16", page=64, pps=17, seed=89, fused=True)
  s_main, s_side = t["storage"].clone(), t["storage"].clone()
  kw = dict(kv=t["kv"], num_splits=num_splits, flags=hip.FLAG_FORCE_SPLITS if num_splits > 1 else 0)
  main = _call(hip, t, True, pool=R.reviewed(t["pool"], t["storage"], s_main), **kw)
  torch.cuda.synchronize()
  stream = torch.cuda.Stream()
  assert stream != torch.cuda.current_stream()
  with torch.cuda.stream(stream):
    side = _call(hip, t, True, pool=R.reviewed(t["pool"], t["storage"], s_side), **kw)
  stream.synchronize()
  assert side[2] == main[2] and main[2]["splits"] == num_splits, (main[2], side[2])
  assert _same_bits(main, side)
  assert torch.equal(s_main.view(torch.int16), s_side.view(torch.int16)) and not torch.equal(s_main.view(torch.int16), t["storage"].view(torch.int16))


# ----------------------------------------------------------------------------- i. model-like values
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("variant", C.MODEL_VARIANTS)
def test_i_model_like_latents(hip, variant, dtype):
  """The families of tests/model_values.py as latent rows in shuffled pages of 64 (their ``k``: an outlier channel of the keys below column 512 is an outlier
  channel of the values; the staircases step at every 32-key tile), heads 16 and 32, one token and three causal, 389 and 513 keys, unsplit and three forced
  ranges — one range then holds the sink and the others do not, so the merge sees LSEs tens of units apart.  Each case first shows its family's property on the
  float64 reference."""
  for case in C.model_cases(variant, R.TORCH_DTYPE[dtype]):
    qf, rows = C.build_model_case(case)
    B, hq, hkv, sq, L, _ = case["shape"]
    t = _pool([L] * B, hq, hkv, sq, dtype, page=64, seed=case["seed"], rows=rows, q=qf.transpose(1, 2).contiguous().cuda())
    ref = _reference(t, case["causal"], C.MODEL_SCALE)
    C.assert_family_property(case, qf, rows, ref)
    for ns in (1, 3):
      out, lse, plan = _check(hip, f"i {variant}", t, case["causal"], ref, scale=C.MODEL_SCALE, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS if ns > 1 else 0)
      assert plan["splits"] == ns and plan["row_tiles"] == math.ceil(hq * sq / 64), plan


# ----------------------------------------------------------------------------- the report
def test_zz_report_worst_error_over_allowance():
  """Not a check of the kernels: prints, per section and dtype, the worst error / allowance this run saw (profiles/r17_mla_contract.md)."""
  for (section, dtype), ratio in sorted(RATIOS.items()):
    print(f"[ratio] {section:32s} {dtype}: {ratio:.3f}")
  assert all(r <= 1.0 for r in RATIOS.values())
