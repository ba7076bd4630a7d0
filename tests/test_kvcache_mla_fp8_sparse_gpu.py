"""``ffpa_attn_with_kvcache_mla_sparse_fp8`` on the GPU: the sparse (top-k indexed) latent call over a pool of OCP e4m3 codes — the gather hook and the FP8 hook
of the latent kernel's text in one build (each wave turns the ids of its eight keys of a tile into the offsets of 8-byte register loads, widens what they return
— exactly — and writes the 16-bit image of the tile to LDS).

Two references.  (1) NO TOLERANCE: with a power-of-two ``kv_scale`` the call returns the bits of ``ffpa_attn_with_kvcache_mla_sparse`` on ``pool8.to(dtype)`` under
``softmax_scale * kv_scale``, O scaled by ``kv_scale`` — the LSE in both dtypes and bf16 O (fp16 O is held by (2) only: the last rounding of an fp16 epilogue is the
compiler's choice per build).  (2) float64 attention on the gathered rows of ``pool8.double() * kv_scale`` with ``kv_scale = 0.37``
(tests/kvcache_mla_sparse_ref.py), outputs held to ``kvcache_ref.check`` / ``allowance`` unchanged, LSE to atol 2e-4 / rtol 2e-5 — no new tolerance: the arithmetic
on the dequantised values is the 16-bit kernel's and the one multiply by ``kv_scale`` lies inside that allowance, as in tests/test_kvcache_mla_fp8_gpu.py.

D = 576, head_dim_v = 512, scale 1 / sqrt(192), pools of 1024 rows; every byte no token selects — rows of the pool, the guard rows around its view, the padding of
padded layouts — holds the FP8 NaN code 0x7F.  Tiles hold 32 keys: the counts 0, 1, 31, 32, 33, 64, 97, 300 are the empty row, one key, each side of a tile, odd
and even tile counts and a partial last tile; forced KV ranges start at odd tiles."""

import contextlib

import pytest
import torch

import kvcache_mla_sparse_ref as SR
import kvcache_ref as R
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D, DV = 576, 512
SCALE = 192 ** -0.5
COUNTS = [0, 1, 31, 32, 33, 64, 97, 300]
HEADS = [(16, 1), (72, 1), (128, 1), (32, 2)]
F8 = torch.float8_e4m3fn
NAN8 = 0x7F
GUARD = 32  # NaN rows in front of and behind the pool's view
KERNEL = "ffpa_fwd_m16_mla_sparse_fp8_kernel"
INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1


@contextlib.contextmanager
def _launches(hip, flags=0, record=True):
  """Every sparse launch inside the block — of either pool format: both go through ``hip.mla_sparse_forward`` — carries ``flags`` too, and (``record``) its plan
  is appended to the list the block receives (not under a graph capture: the plan query is host work, but nothing there needs it)."""
  plans, real = [], hip.mla_sparse_forward

  def spy(*args, **kw):
    kw["flags"] = kw.get("flags", 0) | flags
    if not record:
      return real(*args, **kw)
    plan = {}
    kw["plan_out"] = plan
    out = real(*args, **kw)
    plans.append(plan)
    return out

  hip.mla_sparse_forward = spy
  try:
    yield plans
  finally:
    hip.mla_sparse_forward = real


_CASES: dict = {}


def _case(counts, hq, hkv, dtype, topk=300, rows=1024, seed=0, tail="minus_one"):
  """q, the flat FP8 pool (a view of a uint8 storage with GUARD rows of the NaN code on either side; the NaN code in every row no token selects), random slots
  WITH duplicates, the counts: made once per shape and shared (nothing writes to it).  Selected rows hold ``quantize_latent_rows(randn, 1)``; the first key of the
  token with the most keys is a row of +-448 codes, and the only key of every token of count 1 is a row of zero codes.  ``tail``: what stands at and past a row's
  count — -1, or in-range ids of NaN rows; neither may be read."""
  key = (tuple(counts), hq, hkv, dtype, topk, rows, seed, tail)
  if key in _CASES:
    return _CASES[key]
  from ffpa_attn_amd import quantize_latent_rows

  g = torch.Generator(device="cuda").manual_seed(4000 + seed)
  gc = torch.Generator().manual_seed(seed)
  T = len(counts)
  q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=R.TORCH_DTYPE[dtype])
  codes = quantize_latent_rows(torch.randn((rows, hkv, D), generator=g, device="cuda", dtype=torch.float32), 1.0).view(torch.uint8)
  live = torch.randperm(rows, generator=gc)[: rows // 2]  # slots are drawn from half of the pool: the other half stays NaN
  idx = live[torch.randint(0, live.numel(), (T, topk), generator=gc)]
  seen = torch.zeros(rows, dtype=torch.bool)
  for t, n in enumerate(counts):
    if n >= 2:
      idx[t, n - 1] = idx[t, 0]  # a duplicate in every row that has room for one
    seen[idx[t, :n]] = True
  dead = (~seen).nonzero().flatten()
  for t, n in enumerate(counts):
    idx[t, n:] = -1 if tail == "minus_one" else dead[torch.randint(0, dead.numel(), (topk - n,), generator=gc)]
  codes[~seen.cuda()] = NAN8
  zero_rows = [int(idx[t, 0]) for t, n in enumerate(counts) if n == 1]
  most = max(range(T), key=lambda t: counts[t])
  big_row = next((int(r) for r in idx[most, : counts[most]] if int(r) not in zero_rows), None) if counts[most] > 1 else None
  if big_row is not None:
    codes[big_row] = torch.tensor([0x7E, 0xFE], dtype=torch.uint8, device="cuda").repeat(D // 2)
  for r in zero_rows:
    codes[r] = 0
  storage = torch.full((rows + 2 * GUARD, hkv, D), NAN8, dtype=torch.uint8, device="cuda")
  view = storage[GUARD:-GUARD]
  view.copy_(codes)
  t = dict(q=q, pool=view.view(F8), view=view, storage=storage, idx=idx.to(torch.int32).cuda(), lens=torch.tensor(counts, dtype=torch.int32, device="cuda"),
           counts=list(counts), dtype=dtype, heads=(hq, hkv), topk=topk, zero_rows=zero_rows, big_row=big_row, refs={})
  _CASES[key] = t
  return t


def _ref(t, kv_scale):
  """float64 attention on the dequantised gathered rows -> (reference tuple, vstat), once per (case, scale)."""
  if kv_scale not in t["refs"]:
    deq = t["pool"].double() * kv_scale
    t["refs"][kv_scale] = (SR.reference(t["q"], deq, t["idx"], t["counts"], SCALE, DV), SR.visible_values(deq, t["idx"], t["counts"], DV))
  return t["refs"][kv_scale]


def _fp8(hip, t, *, kv_scale=1.0, num_splits=0, flags=0, q=None, pool=None, idx=None, lens="case"):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse_fp8

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_sparse_fp8(t["q"] if q is None else q, t["pool"] if pool is None else pool, DV, t["idx"] if idx is None else idx,
                                                     kv_scale=kv_scale, topk_lens=t["lens"] if isinstance(lens, str) else lens, softmax_scale=SCALE,
                                                     num_splits=num_splits, return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"{KERNEL}<{t['dtype']}, 576, dv=512"), plans
  return out, lse, plans[0]


def _wide(hip, t, kv_scale, *, num_splits=0, flags=0):
  """The 16-bit sparse call on the dequantised pool: ``pool8.to(dtype)`` under ``softmax_scale * kv_scale``, O scaled by ``kv_scale``."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse

  pool16 = t["pool"].to(R.TORCH_DTYPE[t["dtype"]]).contiguous()
  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_sparse(t["q"], pool16, DV, t["idx"], topk_lens=t["lens"], softmax_scale=SCALE * kv_scale, num_splits=num_splits,
                                                 return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"ffpa_fwd_m16_mla_sparse_kernel<{t['dtype']}, 576, dv=512"), plans
  return out * kv_scale, lse, plans[0]


def _same_bits(a, b):
  return torch.equal(a.view(torch.int16) if a.element_size() == 2 else a.view(torch.int32), b.view(torch.int16) if b.element_size() == 2 else b.view(torch.int32))


def _hold(t, out, lse, ref, vstat, name):
  T, hq = out.shape[:2]
  assert out.shape == (T, hq, DV) and lse.shape == (hq, T) and lse.dtype == torch.float32
  ratio = R.check(out[:, None], lse.t()[:, :, None], ref, v=vstat, dtype=t["dtype"], name=name)
  print(f"[mla sparse fp8] {ratio:.3f} {name}")


# ----------------------------------------------------------------------------- 1. bit identity with the 16-bit sparse kernel on the dequantised pool
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv", HEADS)
@pytest.mark.parametrize("tail", ["minus_one", "nan_rows"])
def test_power_of_two_scales_return_the_bits_of_the_16_bit_sparse_call(hip, dtype, hq, hkv, tail):
  """One batch of eight tokens with the counts 0 ... 300, topk 300; kv_scale 1, 0.25 and 8; the same forced KV ranges (1, 2, 3, 5: ranges start at odd tiles, some
  are empty) and the same non-temporal choice on both arms.  The image the FP8 gather writes is the image the LDS-DMA gather writes, and nothing behind the image
  differs: LSE (both dtypes) and bf16 O are the 16-bit call's bits; the plan names the new kernel with the twin's workgroups and splits."""
  t = _case(COUNTS, hq, hkv, dtype, seed=hq, tail=tail)
  runs = [(1.0, 1, hip.FLAG_NO_KV_STREAM), (1.0, 2, hip.FLAG_KV_STREAM), (0.25, 3, hip.FLAG_NO_KV_STREAM), (0.25, 1, hip.FLAG_KV_STREAM), (8.0, 5, hip.FLAG_KV_STREAM),
          (8.0, 2, hip.FLAG_NO_KV_STREAM)]
  for kv_scale, ns, stream in runs:
    flags = hip.FLAG_FORCE_SPLITS | stream
    out, lse, plan = _fp8(hip, t, kv_scale=kv_scale, num_splits=ns, flags=flags)
    want, want_lse, want_plan = _wide(hip, t, kv_scale, num_splits=ns, flags=flags)
    what = f"{dtype} heads {(hq, hkv)} tail {tail} kv_scale {kv_scale} splits {ns} -> {plan}"
    assert plan["splits"] == ns == want_plan["splits"] and (", NT>" in plan["kernel"]) == (stream == hip.FLAG_KV_STREAM) == (", NT>" in want_plan["kernel"]), what
    assert plan["kernel"] == want_plan["kernel"].replace("_mla_sparse_kernel", "_mla_sparse_fp8_kernel") and plan["workgroups"] == want_plan["workgroups"], what
    assert plan["row_tiles"] == want_plan["row_tiles"] == -(-(hq // hkv) // 64) and plan["block_keys"] == 32, what
    assert out.shape == (len(COUNTS), hq, DV) and (out[0] == 0).all() and torch.isneginf(lse[:, 0]).all()
    assert torch.isfinite(out).all() and torch.isfinite(lse[:, 1:]).all(), what  # (no NaN row, guard row or tail entry was read)
    assert _same_bits(lse, want_lse), f"LSE: {what}: {int((lse != want_lse).sum())} rows differ"
    if dtype == "bf16":
      assert _same_bits(out, want), f"O: {what}: {int((out != want).sum())} elements differ, max {(out.float() - want.float()).abs().max().item():.3e}"


# ----------------------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv", HEADS)
@pytest.mark.parametrize("tail", ["minus_one", "nan_rows"])
def test_a_scale_that_is_no_power_of_two_against_float64(hip, dtype, hq, hkv, tail):
  """kv_scale = 0.37 on the same batch — it holds a row of +-448 codes among the keys of the 300-key token and a token whose only key is a row of zero codes —
  with the library's own split count, with three forced ranges and through the NT build."""
  t = _case(COUNTS, hq, hkv, dtype, seed=hq, tail=tail)
  assert t["big_row"] is not None and ((t["view"][t["big_row"]] & 0x7F) == 0x7E).all() and t["big_row"] in t["idx"][7, :300].tolist()
  assert len(t["zero_rows"]) == 1 and (t["view"][t["zero_rows"][0]] == 0).all() and int(t["idx"][1, 0]) == t["zero_rows"][0]
  ref, vstat = _ref(t, 0.37)
  assert vstat[0] == pytest.approx(448 * 0.37)
  for kw in ({}, dict(num_splits=3, flags=hip.FLAG_FORCE_SPLITS), dict(flags=hip.FLAG_KV_STREAM)):
    out, lse, plan = _fp8(hip, t, kv_scale=0.37, **kw)
    _hold(t, out, lse, ref, vstat, f"float64: {dtype} heads {(hq, hkv)} tail {tail} {kw} -> {plan}")
    assert (out[0] == 0).all() and torch.isneginf(lse[:, 0]).all()
    assert (out[1] == 0).all() and lse[:, 1].abs().max().item() <= R.LSE_ATOL  # the zero row alone: p = 1 on a row of zeros
  # no counts: every row holds topk valid entries
  full = _case([300, 300, 300], hq, hkv, dtype, seed=hq + 7)
  ref, vstat = _ref(full, 0.37)
  out, lse, plan = _fp8(hip, full, kv_scale=0.37, lens=None)
  _hold(full, out, lse, ref, vstat, f"topk_lens=None: {dtype} heads {(hq, hkv)} -> {plan}")


# ----------------------------------------------------------------------------- 3. identities
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("hq", [16, 128])
def test_listing_a_sequences_slots_in_order_is_the_dense_fp8_latent_call(hip, dtype, ns, hq):
  """indices[t] = the slots of sequence t's keys in order (a page-64 FP8 pool behind a shuffled block table): the sparse FP8 launch reads the same codes into the
  same LDS image as ``ffpa_attn_with_kvcache_mla_fp8``, so at the same forced number of ranges the LSE is the same bits in both dtypes and O in bf16."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_fp8, quantize_latent_rows, slots_from_block_table

  lens_l = [1, 33, 64, 97, 300, 0]
  T, page, pps = len(lens_l), 64, 5
  g = torch.Generator(device="cuda").manual_seed(300 + hq)
  q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=R.TORCH_DTYPE[dtype])
  n_pages = T * pps + 1
  pool = quantize_latent_rows(torch.randn((n_pages, page, 1, D), generator=g, device="cuda"), 1.0)
  table = torch.randperm(n_pages, generator=torch.Generator().manual_seed(3))[: T * pps].to(torch.int32).view(T, pps).cuda()
  lens = torch.tensor(lens_l, dtype=torch.int32, device="cuda")
  idx = slots_from_block_table(torch.arange(pps * page, dtype=torch.int32, device="cuda").expand(T, -1), table, page)
  flags = hip.FLAG_FORCE_SPLITS if ns > 1 else 0
  plan_d, real = {}, hip.mla_forward
  hip.mla_forward = lambda *a, **kw: real(*a, **dict(kw, flags=kw.get("flags", 0) | flags, plan_out=plan_d))
  try:
    want, want_lse = ffpa_attn_with_kvcache_mla_fp8(q[:, None], pool, DV, kv_scale=0.37, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, num_splits=ns,
                                                    return_softmax_lse=True)
  finally:
    hip.mla_forward = real
  assert plan_d["kernel"].startswith("ffpa_fwd_m16_mla_fp8_kernel"), plan_d
  t = dict(q=q, pool=pool, idx=idx, lens=lens, dtype=dtype)
  out, lse, plan = _fp8(hip, t, kv_scale=0.37, num_splits=ns, flags=flags)
  assert plan["splits"] == plan_d["splits"] == ns and plan["row_tiles"] == plan_d["row_tiles"], (plan, plan_d)
  assert _same_bits(lse, want_lse[:, :, 0].t().contiguous())
  if dtype == "bf16":
    assert _same_bits(out, want[:, 0].contiguous()), f"{int((out != want[:, 0]).sum())} elements differ"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv", [(16, 1), (128, 1), (32, 2)])
def test_the_nt_build_is_bit_identical_to_the_plain_build(hip, dtype, hq, hkv):
  t = _case(COUNTS, hq, hkv, dtype, seed=hq)
  for ns in (1, 3):
    plain = _fp8(hip, t, kv_scale=0.37, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS | hip.FLAG_NO_KV_STREAM)
    nt = _fp8(hip, t, kv_scale=0.37, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS | hip.FLAG_KV_STREAM)
    assert ", NT>" in nt[2]["kernel"] and ", NT>" not in plain[2]["kernel"] and nt[2]["workgroups"] == plain[2]["workgroups"]
    assert _same_bits(nt[0], plain[0]) and _same_bits(nt[1], plain[1])


# ----------------------------------------------------------------------------- 4. safety of the gather
def test_entries_in_front_of_the_count_outside_the_pool_are_clamped_not_followed(hip):
  """Negative ids and ids >= num_rows in front of a token's count are clamped into the pool's view (rows 0 and num_rows - 1, made finite here): the call stays
  memory-safe, the other tokens' results do not move by a bit, and the bad token's own result is the attention over the clamped rows — finite: the NaN guard
  rows on either side of the view were not read."""
  t = _case([33, 97, 300, 64], 16, 1, "bf16", seed=150)
  storage = t["storage"].clone()
  view = storage[GUARD:-GUARD]
  view[0], view[-1] = 0x38, 0xB8  # (rows of +1 and of -1 where the clamp lands)
  pool = view.view(F8)
  base = _fp8(hip, t, kv_scale=0.37, pool=pool)
  idx = t["idx"].clone()
  idx[1, 5], idx[1, 40], idx[1, 41], idx[1, 42] = INT_MAX, INT_MIN, -1, pool.size(0)
  out, lse, _ = _fp8(hip, t, kv_scale=0.37, idx=idx, pool=pool)
  keep = [0, 2, 3]
  assert _same_bits(out[keep], base[0][keep]) and _same_bits(lse[:, keep], base[1][:, keep])
  assert torch.isfinite(out).all() and torch.isfinite(lse).all()
  clamped = idx.clone()
  clamped[1, 5], clamped[1, 40], clamped[1, 41], clamped[1, 42] = pool.size(0) - 1, 0, 0, pool.size(0) - 1
  want = _fp8(hip, t, kv_scale=0.37, idx=clamped, pool=pool)
  assert _same_bits(out, want[0]) and _same_bits(lse, want[1])
  deq = pool.double() * 0.37
  _hold(t, out, lse, SR.reference(t["q"], deq, clamped, t["counts"], SCALE, DV), SR.visible_values(deq, clamped, t["counts"], DV), "clamped entries")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_entries_at_and_past_the_count_hold_garbage_and_change_nothing(hip, dtype):
  """INT_MIN, INT_MAX and -1 at and past every count — the entry AT the count, the rest of its tile, whole tiles behind it: not a bit moves, at 1 and 3 ranges."""
  t = _case(COUNTS, 16, 1, dtype, seed=16)
  for ns in (1, 3):
    base = _fp8(hip, t, kv_scale=0.37, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS)
    for junk in (INT_MIN, INT_MAX, -1):
      idx = t["idx"].clone()
      for i, n in enumerate(t["counts"]):
        idx[i, n:] = junk
      got = _fp8(hip, t, kv_scale=0.37, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS, idx=idx)
      assert _same_bits(got[0], base[0]) and _same_bits(got[1], base[1]), (junk, ns)
    mixed = t["idx"].clone()
    for i, n in enumerate(t["counts"]):
      mixed[i, n:] = torch.tensor([INT_MIN, INT_MAX, -1, 2 ** 30], dtype=torch.int32, device="cuda").repeat(t["topk"])[: t["topk"] - n]
    got = _fp8(hip, t, kv_scale=0.37, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS, idx=mixed)
    assert _same_bits(got[0], base[0]) and _same_bits(got[1], base[1]), ns


@pytest.mark.parametrize("layout", ["flat", "page1", "page16", "page64", "row_padded", "head_padded"])
def test_pool_layouts_and_strided_arguments(hip, layout):
  """The flat 3-D pool, 4-D pools of page size 1 / 16 / 64, a padded row stride (592 bytes per head row) and a padded head stride — every stride a multiple of 16;
  q as a slice of a fused projection, indices as ``wide[:, 5:5 + topk]`` of a wider tensor (its other columns hold ids far outside the pool), topk_lens as
  ``buf[::2]``.  Everything a storage holds outside the pool's view is the NaN code: the same rows through other strides are the same bits, and float64 holds."""
  hq, hkv = 32, 2
  t = _case([1, 33, 97, 300, 0, 64], hq, hkv, "bf16", seed=90)
  flat = t["view"]
  rows = flat.size(0)
  if layout == "flat":
    pool = t["pool"]
  elif layout.startswith("page"):
    page = int(layout[4:])
    store = torch.full((rows // page + 2, page, hkv, D), NAN8, dtype=torch.uint8, device="cuda")
    pool = store[1:-1]
    pool.copy_(flat.view(rows // page, page, hkv, D))
  elif layout == "row_padded":
    store = torch.full((rows + 2, hkv * (D + 16)), NAN8, dtype=torch.uint8, device="cuda")
    pool = store[1:-1].view(rows, hkv, D + 16)[..., :D]
    pool.copy_(flat)
    assert pool.stride() == (hkv * 592, 592, 1)
  else:
    store = torch.full((rows + 2, hkv, D + 64), NAN8, dtype=torch.uint8, device="cuda")
    pool = store[1:-1, :, :D]
    pool.copy_(flat)
    assert pool.stride() == (hkv * 640, 640, 1)
  assert all(st % 16 == 0 for st in pool.stride()[:-1])
  fused = torch.full((6, hq + 2, D), float("nan"), dtype=t["q"].dtype, device="cuda")
  fused[:, :hq] = t["q"]
  wide = torch.full((6, t["topk"] + 9), 2 ** 30, dtype=torch.int32, device="cuda")
  wide[:, 5:5 + t["topk"]] = t["idx"]
  buf = torch.full((12,), 2 ** 30, dtype=torch.int32, device="cuda")
  buf[::2] = t["lens"]
  out, lse, plan = _fp8(hip, t, kv_scale=0.37, q=fused[:, :hq], pool=pool.view(F8), idx=wide[:, 5:5 + t["topk"]], lens=buf[::2])
  ref, vstat = _ref(t, 0.37)
  _hold(t, out, lse, ref, vstat, f"layout {layout} -> {plan}")
  plain = _fp8(hip, t, kv_scale=0.37)
  assert _same_bits(out, plain[0]) and _same_bits(lse, plain[1])


# ----------------------------------------------------------------------------- 5. one graph
def test_one_graph_follows_the_steps_tensors_and_pool_bytes_written_in_place(hip):
  """Captured once — a split launch: the merge is in the graph —, then q, indices, topk_lens and pool BYTES are overwritten in place: every replay equals a fresh
  eager call bit for bit, and the float64 reference."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse_fp8, quantize_latent_rows

  t = _case([5, 300, 64, 97], 16, 1, "bf16", seed=120)
  storage = t["storage"].clone()
  storage[(storage & 0x7F) == 0x7F] = 0x30  # (replays move the lists around: every row must hold a number)
  pool = storage[GUARD:-GUARD].view(F8)
  q, idx, lens = t["q"].clone(), t["idx"].clone().clamp_(min=0), t["lens"].clone()
  call = lambda: ffpa_attn_with_kvcache_mla_sparse_fp8(q, pool, DV, idx, kv_scale=0.37, topk_lens=lens, softmax_scale=SCALE, num_splits=3, return_softmax_lse=True)
  with _launches(hip, hip.FLAG_FORCE_SPLITS) as plans:
    call()  # (warm: the library is loaded, the scratch is sized)
  assert len(plans) == 1 and plans[0]["splits"] == 3 and plans[0]["kernel"].startswith(KERNEL) and plans[0]["kernel"].endswith("+ ffpa_varlen_merge_kernel"), plans
  with _launches(hip, hip.FLAG_FORCE_SPLITS, record=False):
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      out_g, lse_g = call()
    gc = torch.Generator().manual_seed(5)
    for step, counts in enumerate(([5, 300, 64, 97], [0, 33, 300, 1], [300, 31, 32, 160])):
      if step:
        q.copy_(torch.randn_like(q))
        idx.copy_(torch.randint(0, pool.size(0), tuple(idx.shape), generator=gc).to(torch.int32))
        rows = torch.randperm(pool.size(0), generator=gc)[:100].cuda()
        pool.view(torch.uint8)[rows] = quantize_latent_rows(torch.randn((100, 1, D), device="cuda"), 0.37).view(torch.uint8)
      lens.copy_(torch.tensor(counts, dtype=torch.int32, device="cuda"))
      graph.replay()
      torch.cuda.synchronize()
      eager = call()
      torch.cuda.synchronize()
      assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1]), counts
      deq = pool.double() * 0.37
      R.check(out_g[:, None], lse_g.t()[:, :, None], SR.reference(q, deq, idx, counts, SCALE, DV), v=SR.visible_values(deq, idx, counts, DV), dtype="bf16",
              name=f"graph replay at {counts}")


# ----------------------------------------------------------------------------- 6. torch.compile
def test_under_torch_compile_fullgraph(hip):
  from ffpa_attn_amd import compact_topk_indices, ffpa_attn_with_kvcache_mla_sparse_fp8

  t = _case([33, 0, 97, 300], 16, 1, "fp16", seed=130)

  def f(q, pool, idx):
    slots, counts = compact_topk_indices(idx)  # (rows padded with -1 behind their count: already compact, counted here)
    o, lse = ffpa_attn_with_kvcache_mla_sparse_fp8(q, pool, DV, slots, kv_scale=0.37, topk_lens=counts, softmax_scale=SCALE, return_softmax_lse=True)
    return o * 2, lse

  with _launches(hip) as plans:
    eager = f(t["q"], t["pool"], t["idx"])
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"{KERNEL}<fp16, 576, dv=512"), plans
  compiled = torch.compile(f, fullgraph=True)(t["q"], t["pool"], t["idx"])
  torch.cuda.synchronize()
  assert torch.equal(eager[0], compiled[0]) and torch.equal(eager[1], compiled[1])
  ref, vstat = _ref(t, 0.37)
  R.check((compiled[0].double() / 2).to(torch.float16)[:, None], compiled[1].t()[:, :, None], ref, v=vstat, dtype="fp16", name="torch.compile")
