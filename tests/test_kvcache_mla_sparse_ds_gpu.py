"""``ffpa_attn_with_kvcache_mla_sparse_ds`` and ``store_latent_rows_ds`` on the GPU: the sparse (top-k indexed) latent call over the 656-byte FP8 rows of
DeepSeek-V3.2 (512 e4m3 codes, four float32 scales — one per 128 columns —, 64 bf16 rotary columns) and the kernel that writes such rows by slot.

Two references.  (1) NO TOLERANCE: ``unpack_latent_rows_ds`` is the definition of what the kernel computes on, and nothing is folded into the softmax scale, so O and
LSE are the bits of ``ffpa_attn_with_kvcache_mla_sparse(q, unpack_latent_rows_ds(pool), ...)`` under the same ``num_splits`` and flags.  (2) float64 attention on the
gathered rows of the unpacked pool (tests/kvcache_mla_sparse_ref.py), held to ``kvcache_ref.check`` / ``allowance`` unchanged: the values the kernel multiplies are
bf16 values, as in the 16-bit sparse suite.  The store kernel is held to ``pack_latent_rows_ds`` byte for byte.

D = 576, head_dim_v = 512, scale 1 / sqrt(192), pools of 1024 rows, bf16.  An addressing mistake shows: the four tile scales of a row differ by powers of 7.3 (no
power of two), the rotary columns come from another distribution than the latent ones, and every byte no token selects — rows of the pool, the guard rows around
its view, the padding of padded layouts — is 0xFF: NaN as a code, as a scale and as bf16.  Tiles hold 32 keys: the counts 0, 1, 31, 32, 33, 300 are the empty row,
one key, each side of a tile and a partial last tile; Hq = 128 over one latent head is two row chunks."""

import contextlib

import pytest
import torch

import kvcache_mla_sparse_ref as SR
import kvcache_ref as R
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D, DV, ROW = 576, 512, 656
SCALE = 192 ** -0.5
COUNTS = [0, 1, 31, 32, 33, 300]
HEADS = [(16, 1), (128, 1), (16, 2), (128, 2)]
GUARD = 32  # 0xFF rows in front of and behind the pool's view
KERNEL = "ffpa_fwd_m16_mla_sparse_ds_kernel"
INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1


@contextlib.contextmanager
def _launches(hip, flags=0, record=True):
  """Every sparse launch inside the block — of either pool format: both go through ``hip.mla_sparse_forward`` — carries ``flags`` too, and (``record``) its plan
  is appended to the list the block receives."""
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


def _rows(shape, g):
  """Latent rows [..., 576] (bf16 on the GPU): tile j of the 512 latent columns is randn x a per-row factor in [0.5, 1.5) x 7.3^(j - 1), the rotary columns are
  uniform in [-3, 3).  A tile whose largest magnitude is 1.75 x 2^k as a bf16 — its scale amax / 448 would be a power of two — is stretched by 1.25."""
  nope = torch.randn(shape + (4, 128), generator=g, device="cuda") * (0.5 + torch.rand(shape + (1, 1), generator=g, device="cuda"))
  nope = (nope * torch.tensor([7.3 ** (j - 1) for j in range(4)], device="cuda").view(4, 1)).to(torch.bfloat16)
  pow2 = torch.frexp(nope.float().abs().amax(-1, keepdim=True) / 448)[0] == 0.5
  nope = torch.where(pow2, nope * 1.25, nope)
  rope = (torch.rand(shape + (64,), generator=g, device="cuda") * 6 - 3).to(torch.bfloat16)
  return torch.cat([nope.flatten(-2), rope], dim=-1)


_CASES: dict = {}


def _case(counts, hq, hkv, topk=300, rows=1024, seed=0):
  """q, the flat byte pool (a view of a storage with GUARD rows of 0xFF on either side; 0xFF in every row no token selects), random slots WITH duplicates and -1
  behind every count, the counts, and the unpacked pool: made once per shape and shared (nothing writes to it)."""
  key = (tuple(counts), hq, hkv, topk, rows, seed)
  if key in _CASES:
    return _CASES[key]
  from ffpa_attn_amd import pack_latent_rows_ds, unpack_latent_rows_ds

  g = torch.Generator(device="cuda").manual_seed(7000 + seed)
  gc = torch.Generator().manual_seed(seed)
  T = len(counts)
  q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
  packed = pack_latent_rows_ds(_rows((rows, hkv), g).to(torch.bfloat16))
  live = torch.randperm(rows, generator=gc)[: rows // 2]  # slots are drawn from half of the pool: the other half stays 0xFF
  idx = live[torch.randint(0, live.numel(), (T, topk), generator=gc)]
  seen = torch.zeros(rows, dtype=torch.bool)
  for t, n in enumerate(counts):
    if n >= 2:
      idx[t, n - 1] = idx[t, 0]  # a duplicate in every row that has room for one
    seen[idx[t, :n]] = True
    idx[t, n:] = -1
  packed[~seen.cuda()] = 0xFF
  storage = torch.full((rows + 2 * GUARD, hkv, ROW), 0xFF, dtype=torch.uint8, device="cuda")
  view = storage[GUARD:-GUARD]
  view.copy_(packed)
  s = view[seen.cuda()][..., 512:528].contiguous().view(torch.float32)
  assert ((s[..., 1:] / s[..., :-1]) > 2).all() and (torch.frexp(s)[0] != 0.5).all()  # (the scales of a row differ and none is a power of two)
  t = dict(q=q, pool=view, storage=storage, wide=unpack_latent_rows_ds(view), idx=idx.to(torch.int32).cuda(), lens=torch.tensor(counts, dtype=torch.int32, device="cuda"),
           counts=list(counts), heads=(hq, hkv), topk=topk, refs={})
  _CASES[key] = t
  return t


def _ref(t):
  """float64 attention on the gathered rows of the unpacked pool -> (reference tuple, vstat), once per case."""
  if "f64" not in t["refs"]:
    deq = t["wide"].double()
    t["refs"]["f64"] = (SR.reference(t["q"], deq, t["idx"], t["counts"], SCALE, DV), SR.visible_values(deq, t["idx"], t["counts"], DV))
  return t["refs"]["f64"]


def _ds(hip, t, *, num_splits=0, flags=0, q=None, pool=None, idx=None, lens="case"):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse_ds

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_sparse_ds(t["q"] if q is None else q, t["pool"] if pool is None else pool, DV, t["idx"] if idx is None else idx,
                                                    topk_lens=t["lens"] if isinstance(lens, str) else lens, softmax_scale=SCALE, num_splits=num_splits,
                                                    return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"{KERNEL}<bf16, 576, dv=512"), plans
  return out, lse, plans[0]


def _base(hip, t, *, num_splits=0, flags=0, wide=None, idx=None):
  """The 16-bit sparse call on the unpacked pool."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_sparse(t["q"], t["wide"] if wide is None else wide, DV, t["idx"] if idx is None else idx, topk_lens=t["lens"],
                                                 softmax_scale=SCALE, num_splits=num_splits, return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith("ffpa_fwd_m16_mla_sparse_kernel<bf16, 576, dv=512"), plans
  return out, lse, plans[0]


def _same_bits(a, b):
  return torch.equal(a.view(torch.int16) if a.element_size() == 2 else a.view(torch.int32), b.view(torch.int16) if b.element_size() == 2 else b.view(torch.int32))


def _hold(out, lse, ref, vstat, name):
  T, hq = out.shape[:2]
  assert out.shape == (T, hq, DV) and lse.shape == (hq, T) and lse.dtype == torch.float32
  ratio = R.check(out[:, None], lse.t()[:, :, None], ref, v=vstat, dtype="bf16", name=name)
  print(f"[mla sparse ds] {ratio:.3f} {name}")


# ----------------------------------------------------------------------------- 1. bit identity with the 16-bit sparse kernel on the unpacked pool
@pytest.mark.parametrize("hq, hkv", HEADS)
def test_the_call_returns_the_bits_of_the_16_bit_sparse_call_on_the_unpacked_pool(hip, hq, hkv):
  """Six tokens with the counts 0 ... 300 of topk 300; the library's own launch and three forced KV ranges, the plain build and the NT build, the same choice on
  both arms.  The image the kernel writes is the image the LDS-DMA gather writes from the unpacked pool and nothing behind the image differs: not a bit of O or
  LSE moves, and the NT build equals the plain build."""
  t = _case(COUNTS, hq, hkv, seed=hq + hkv)
  got = {}
  for ns in (0, 3):
    for stream in (hip.FLAG_NO_KV_STREAM, hip.FLAG_KV_STREAM):
      flags = stream | (hip.FLAG_FORCE_SPLITS if ns else 0)
      out, lse, plan = _ds(hip, t, num_splits=ns, flags=flags)
      want, want_lse, want_plan = _base(hip, t, num_splits=ns, flags=flags)
      what = f"heads {(hq, hkv)} splits {ns} -> {plan}"
      assert plan["splits"] == want_plan["splits"] and (ns == 0 or plan["splits"] == ns), what
      assert (", NT>" in plan["kernel"]) == (stream == hip.FLAG_KV_STREAM) == (", NT>" in want_plan["kernel"]), what
      assert plan["kernel"] == want_plan["kernel"].replace("_mla_sparse_kernel", "_mla_sparse_ds_kernel") and plan["workgroups"] == want_plan["workgroups"], what
      assert plan["row_tiles"] == want_plan["row_tiles"] == -(-(hq // hkv) // 64) and plan["block_keys"] == 32, what
      assert out.shape == (len(COUNTS), hq, DV) and (out[0] == 0).all() and torch.isneginf(lse[:, 0]).all(), what
      assert torch.isfinite(out).all() and torch.isfinite(lse[:, 1:]).all(), what  # (no 0xFF row, guard row or tail entry was read)
      assert _same_bits(lse, want_lse), f"LSE: {what}: {int((lse != want_lse).sum())} rows differ"
      assert _same_bits(out, want), f"O: {what}: {int((out != want).sum())} elements differ, max {(out.float() - want.float()).abs().max().item():.3e}"
      got[(ns, stream)] = (out, lse)
    nt, plain = got[(ns, hip.FLAG_KV_STREAM)], got[(ns, hip.FLAG_NO_KV_STREAM)]
    assert _same_bits(nt[0], plain[0]) and _same_bits(nt[1], plain[1]), f"NT build against plain build: heads {(hq, hkv)} splits {ns}"


# ----------------------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize("hq, hkv", HEADS)
def test_against_float64_on_the_unpacked_pool(hip, hq, hkv):
  t = _case(COUNTS, hq, hkv, seed=hq + hkv)
  ref, vstat = _ref(t)
  for kw in ({}, dict(num_splits=3, flags=hip.FLAG_FORCE_SPLITS), dict(flags=hip.FLAG_KV_STREAM)):
    out, lse, plan = _ds(hip, t, **kw)
    _hold(out, lse, ref, vstat, f"float64: heads {(hq, hkv)} {kw} -> {plan}")
    assert (out[0] == 0).all() and torch.isneginf(lse[:, 0]).all()
  full = _case([300, 300, 300], hq, hkv, seed=hq + hkv + 7)  # no counts: every row holds topk valid entries
  ref, vstat = _ref(full)
  out, lse, plan = _ds(hip, full, lens=None)
  _hold(out, lse, ref, vstat, f"topk_lens=None: heads {(hq, hkv)} -> {plan}")


# ----------------------------------------------------------------------------- 3. the index list's edge cases
@pytest.mark.parametrize("ns", [1, 3])
def test_entries_at_and_past_the_count_hold_garbage_and_change_nothing(hip, ns):
  """INT_MIN, INT_MAX, -1 and 2^30 at and past every count — the entry AT the count, the rest of its tile, whole tiles behind it — on the codes' load and on the
  scale's: not a bit moves, and the result is the base call's."""
  t = _case(COUNTS, 16, 1, seed=17)
  flags = hip.FLAG_FORCE_SPLITS
  base = _base(hip, t, num_splits=ns, flags=flags)
  for junk in (INT_MIN, INT_MAX, -1, None):
    idx = t["idx"].clone()
    for i, n in enumerate(t["counts"]):
      idx[i, n:] = junk if junk is not None else torch.tensor([INT_MIN, INT_MAX, -1, 2 ** 30], dtype=torch.int32, device="cuda").repeat(t["topk"])[: t["topk"] - n]
    got = _ds(hip, t, num_splits=ns, flags=flags, idx=idx)
    assert _same_bits(got[0], base[0]) and _same_bits(got[1], base[1]), (junk, ns)
    assert (got[0][0] == 0).all() and torch.isneginf(got[1][:, 0]).all()  # count 0: O = 0, LSE = -inf


def test_entries_in_front_of_the_count_outside_the_pool_are_clamped_not_followed(hip):
  """Negative ids and ids >= num_rows in front of a token's count are clamped into the pool's view (rows 0 and num_rows - 1, made finite here): the result is the
  base call's on the same list, bit for bit, the clamped list's too, and finite — the 0xFF guard rows on either side of the view were not read."""
  from ffpa_attn_amd import pack_latent_rows_ds, unpack_latent_rows_ds

  t = _case([33, 97, 300, 64], 16, 1, seed=150)
  storage = t["storage"].clone()
  view = storage[GUARD:-GUARD]
  ends = pack_latent_rows_ds(_rows((2, 1), torch.Generator(device="cuda").manual_seed(1)).to(torch.bfloat16))
  view[0], view[-1] = ends[0], ends[1]
  wide = unpack_latent_rows_ds(view)
  idx = t["idx"].clone()
  idx[1, 5], idx[1, 40], idx[1, 41], idx[1, 42] = INT_MAX, INT_MIN, -1, view.size(0)
  out, lse, _ = _ds(hip, t, idx=idx, pool=view)
  assert torch.isfinite(out).all() and torch.isfinite(lse).all()
  want = _base(hip, t, idx=idx, wide=wide)
  assert _same_bits(out, want[0]) and _same_bits(lse, want[1])
  clamped = idx.clone()
  clamped[1, 5], clamped[1, 40], clamped[1, 41], clamped[1, 42] = view.size(0) - 1, 0, 0, view.size(0) - 1
  same = _ds(hip, t, idx=clamped, pool=view)
  assert _same_bits(out, same[0]) and _same_bits(lse, same[1])


# ----------------------------------------------------------------------------- 4. pool layouts
@pytest.mark.parametrize("layout", ["flat", "page1", "page16", "page64", "slot_padded", "head_padded", "offset16"])
def test_pool_layouts_and_strided_arguments(hip, layout):
  """The flat 3-D pool, 4-D pools of page size 1 / 16 / 64, a padded slot stride (672 bytes per head row), a padded head stride and a storage offset of 16 bytes —
  two latent heads, every stride a multiple of 16; q as a slice of a fused projection, indices as ``wide[:, 5:5 + topk]`` of a wider tensor (its other columns hold
  ids far outside the pool), topk_lens as ``buf[::2]``.  Everything a storage holds outside the pool's view is 0xFF: the same rows through other strides are the
  same bits, and float64 holds."""
  hq, hkv = 32, 2
  t = _case([1, 33, 97, 300, 0, 64], hq, hkv, seed=90)
  flat = t["pool"]
  rows = flat.size(0)
  if layout == "flat":
    pool = flat
  elif layout.startswith("page"):
    page = int(layout[4:])
    store = torch.full((rows // page + 2, page, hkv, ROW), 0xFF, dtype=torch.uint8, device="cuda")
    pool = store[1:-1]
    pool.copy_(flat.view(rows // page, page, hkv, ROW))
  elif layout == "slot_padded":
    store = torch.full((rows + 2, hkv * (ROW + 16)), 0xFF, dtype=torch.uint8, device="cuda")
    pool = store[1:-1].view(rows, hkv, ROW + 16)[..., :ROW]
    pool.copy_(flat)
    assert pool.stride() == (hkv * 672, 672, 1)
  elif layout == "head_padded":
    store = torch.full((rows + 2, hkv, ROW + 48), 0xFF, dtype=torch.uint8, device="cuda")
    pool = store[1:-1, :, :ROW]
    pool.copy_(flat)
    assert pool.stride() == (hkv * 704, 704, 1)
  else:
    store = torch.full(((rows + 2) * hkv * ROW + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    pool = store[16 + hkv * ROW: 16 + (rows + 1) * hkv * ROW].view(rows, hkv, ROW)
    pool.copy_(flat)
    assert pool.storage_offset() % 16 == 0 and pool.storage_offset() % 32 != 0
  assert all(st % 16 == 0 for st in pool.stride()[:-1])
  fused = torch.full((6, hq + 2, D), float("nan"), dtype=torch.bfloat16, device="cuda")
  fused[:, :hq] = t["q"]
  wide = torch.full((6, t["topk"] + 9), 2 ** 30, dtype=torch.int32, device="cuda")
  wide[:, 5:5 + t["topk"]] = t["idx"]
  buf = torch.full((12,), 2 ** 30, dtype=torch.int32, device="cuda")
  buf[::2] = t["lens"]
  out, lse, plan = _ds(hip, t, q=fused[:, :hq], pool=pool, idx=wide[:, 5:5 + t["topk"]], lens=buf[::2])
  ref, vstat = _ref(t)
  _hold(out, lse, ref, vstat, f"layout {layout} -> {plan}")
  base = _base(hip, t)
  assert _same_bits(out, base[0]) and _same_bits(lse, base[1])


# ----------------------------------------------------------------------------- 5. the store kernel
@pytest.mark.parametrize("hkv, paged", [(1, False), (2, False), (2, True)])
def test_the_store_writes_pack_latent_rows_ds_at_the_named_slots_and_nothing_else(hip, hkv, paged):
  """Rows with inf, NaN, a zero tile, a tile under the scale floor and a tile of the largest bf16 next to ordinary ones, ``kv`` a slice of a wider tensor; slots -1,
  num_rows and INT_MAX write nothing; every other byte of the pool's storage — the padding of its slot stride and the guard rows included — keeps its 0xA5."""
  from ffpa_attn_amd import pack_latent_rows_ds, store_latent_rows_ds

  rows, T = 96, 13
  g = torch.Generator(device="cuda").manual_seed(50 + hkv)
  fused = torch.full((T, hkv + 1, D + 64), float("nan"), dtype=torch.bfloat16, device="cuda")
  kv = fused[:, :hkv, :D]
  kv.copy_(_rows((T, hkv), g))
  kv[0, 0, 3], kv[0, 0, 200], kv[0, 0, 300] = float("inf"), float("-inf"), float("nan")
  kv[0, 0, 301:303] = torch.tensor([0xFFC0 - 0x10000, 0x7FC1], dtype=torch.int16, device="cuda").view(torch.bfloat16)  # (a negative NaN, a NaN with a payload)
  kv[1, 0, 128:256] = 0
  kv[2, 0, 256:384] = 2.0 ** -110
  kv[3, 0, :128] = torch.finfo(torch.bfloat16).max
  kv[4, 0, 384:512] = float("inf")  # (a tile without a finite element: amax 0, the floor)
  kv[5, 0, 520] = float("nan")      # (rotary columns are copied, whatever they hold)
  assert kv.stride() == ((hkv + 1) * (D + 64), D + 64, 1)
  storage = torch.full((rows + 2, hkv, ROW + 16), 0xA5, dtype=torch.uint8, device="cuda")
  pool = storage[1:-1, :, :ROW]
  slots = torch.tensor([7, 0, rows - 1, 31, 32, 33, -1, rows, 64, INT_MAX, 2, INT_MIN, 50], dtype=torch.int32, device="cuda")
  want = storage.clone()
  ok = (slots >= 0) & (slots < rows)
  packed = pack_latent_rows_ds(kv)
  assert torch.equal(packed.cpu(), pack_latent_rows_ds(kv.cpu()))  # (the definition does not depend on the device it runs on)
  want[1:-1, :, :ROW][slots[ok].long()] = packed[ok]
  store_latent_rows_ds(storage[1:-1].view(rows // 16, 16, hkv, ROW + 16)[..., :ROW] if paged else pool, kv, slots)
  torch.cuda.synchronize()
  diff = (storage != want).nonzero()
  assert diff.numel() == 0, f"{diff.size(0)} bytes differ, first at (row, head, byte) = {diff[0].tolist()}: {int(storage[tuple(diff[0])])} != {int(want[tuple(diff[0])])}"
  assert (want[1:-1][slots[ok].long()][..., :ROW] != 0xA5).any()


# ----------------------------------------------------------------------------- 6. store + attend in one graph
def test_store_then_attend_in_one_graph_follows_the_steps_tensors_written_in_place(hip):
  """Captured once — the store, then a split launch with its merge —, then kv, slots, q, indices and topk_lens are overwritten in place: after every replay the
  pool's bytes are a torch-packed shadow pool's, and O / LSE equal the eager call on that shadow bit for bit."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse_ds, pack_latent_rows_ds, store_latent_rows_ds

  rows, T, hq, topk = 1024, 4, 16, 300
  g = torch.Generator(device="cuda").manual_seed(120)
  gc = torch.Generator().manual_seed(5)
  pool = pack_latent_rows_ds(_rows((rows, 1), g).to(torch.bfloat16))
  shadow = pool.clone()
  q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
  kv = _rows((T, 1), g).to(torch.bfloat16)
  slots = torch.tensor([3, 900, -1, 77], dtype=torch.int32, device="cuda")
  idx = torch.randint(0, rows, (T, topk), generator=gc).to(torch.int32).cuda()
  lens = torch.tensor([5, 300, 64, 97], dtype=torch.int32, device="cuda")

  def step(p):
    store_latent_rows_ds(p, kv, slots)
    return ffpa_attn_with_kvcache_mla_sparse_ds(q, p, DV, idx, topk_lens=lens, softmax_scale=SCALE, num_splits=3, return_softmax_lse=True)

  with _launches(hip, hip.FLAG_FORCE_SPLITS) as plans:
    step(pool.clone())  # (warm: the library is loaded, the scratch is sized)
  assert len(plans) == 1 and plans[0]["splits"] == 3 and plans[0]["kernel"].startswith(KERNEL) and plans[0]["kernel"].endswith("+ ffpa_varlen_merge_kernel"), plans
  with _launches(hip, hip.FLAG_FORCE_SPLITS, record=False):
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      out_g, lse_g = step(pool)
    for n, counts in enumerate(([5, 300, 64, 97], [0, 33, 300, 1], [300, 31, 32, 160])):
      if n:
        q.copy_(torch.randn_like(q))
        kv.copy_(_rows((T, 1), g))
        slots.copy_(torch.tensor([[10, 11, 12, rows], [1023, 0, 512, -1]][n - 1], dtype=torch.int32))
        idx.copy_(torch.randint(0, rows, (T, topk), generator=gc).to(torch.int32))
        idx[2, :4] = slots.clamp(0, rows - 1)  # (the step's new rows are among the keys)
      lens.copy_(torch.tensor(counts, dtype=torch.int32))
      ok = (slots >= 0) & (slots < rows)
      shadow[slots[ok].long()] = pack_latent_rows_ds(kv)[ok]
      graph.replay()
      torch.cuda.synchronize()
      assert torch.equal(pool, shadow), counts
      eager = ffpa_attn_with_kvcache_mla_sparse_ds(q, shadow, DV, idx, topk_lens=lens, softmax_scale=SCALE, num_splits=3, return_softmax_lse=True)
      torch.cuda.synchronize()
      assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1]), counts


# ----------------------------------------------------------------------------- 7. torch.compile
def test_store_and_attend_under_torch_compile_fullgraph(hip):
  from ffpa_attn_amd import compact_topk_indices, ffpa_attn_with_kvcache_mla_sparse_ds, store_latent_rows_ds

  t = _case([33, 0, 97, 300], 16, 1, seed=130)
  kv = _rows((2, 1), torch.Generator(device="cuda").manual_seed(9)).to(torch.bfloat16)
  slots = t["idx"][3, :2].contiguous()  # (two rows the 300-key token attends to)

  def f(q, pool, kv, slots, idx):
    store_latent_rows_ds(pool, kv, slots)
    compact, counts = compact_topk_indices(idx)  # (rows padded with -1 behind their count: already compact, counted here)
    o, lse = ffpa_attn_with_kvcache_mla_sparse_ds(q, pool, DV, compact, topk_lens=counts, softmax_scale=SCALE, return_softmax_lse=True)
    return o * 2, lse

  pool_e, pool_c = t["pool"].clone(), t["pool"].clone()
  with _launches(hip) as plans:
    eager = f(t["q"], pool_e, kv, slots, t["idx"])
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"{KERNEL}<bf16, 576, dv=512"), plans
  compiled = torch.compile(f, fullgraph=True)(t["q"], pool_c, kv, slots, t["idx"])
  torch.cuda.synchronize()
  assert torch.equal(pool_e, pool_c) and not torch.equal(pool_e, t["pool"])
  assert torch.equal(eager[0], compiled[0]) and torch.equal(eager[1], compiled[1])
