"""``ffpa_attn_with_kvcache_mla_fp8`` / ``ffpa_attn_varlen_with_kvcache_mla_fp8`` on the GPU: the FP8 build of the MLA latent-cache kernel (a tile of OCP e4m3
codes is staged in registers, widened — exactly — and written to LDS where the 16-bit build's LDS-DMA pieces land) and the quantising appends.

Two references.  (1) NO TOLERANCE: with a power-of-two ``kv_scale`` the call must return the bits of ``ffpa_attn_with_kvcache_mla`` on ``pool8.to(dtype)`` with
``softmax_scale * kv_scale`` and O scaled by ``kv_scale`` — the LSE in both dtypes and bf16 O (fp16 O is checked by (2) only: the last rounding of an fp16 epilogue
is the compiler's choice per build, as in tests/test_kvcache_mla_gpu.py).  (2) float64 attention (tests/kvcache_ref.py ``attend``) on ``pool8.double() * kv_scale``
with ``kv_scale = 0.37``, outputs held to ``kvcache_ref.check`` / ``allowance`` unchanged, LSE to atol 2e-4 / rtol 2e-5 — no new tolerance: the arithmetic on the
dequantised values is the 16-bit kernel's, and the multiply by ``kv_scale`` is one fp32 rounding inside that allowance.  The appends are held to
``quantize_latent_rows`` byte for byte (NaN codes by NaN-ness).

D = 576, head_dim_v = 512, scale 1 / sqrt(192), pages of 64 keys shuffled in a pool that holds the FP8 NaN code in every row no sequence owns.  Tiles: 64 rows x 32
keys: the key lengths 0 ... 97 and 300 cover the empty sequence, the zero-filled tail row and odd and even tile counts (the image toggle); forced KV ranges start
at odd tiles."""

import contextlib

import numpy as np
import pytest
import torch

import kvcache_ref as R
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D, DV, PAGE = 576, 512, 64
SCALE = 192 ** -0.5
LENS = [0, 1, 31, 32, 33, 64, 65, 96, 97, 300]
HEADS = [(1, 1), (16, 1), (128, 1), (32, 2)]
F8 = torch.float8_e4m3fn
NAN8 = 0x7F
EDGES = [0.0, -0.0, 2.0 ** -9, -2.0 ** -9, 2.0 ** -10, -2.0 ** -10, 1.5 * 2.0 ** -9, -2.5 * 2.0 ** -9, 1.0625, -1.1875, 17.0, -19.0, 432.0, 448.0, -448.0, 449.0,
         -449.0, 464.0, -464.0, 1e4, -1e4, float("inf"), -float("inf")]


@contextlib.contextmanager
def _launches(hip, flags=0):
  """Every latent launch inside the block carries ``flags`` too, and its plan (``plan_out``) is appended to the list the block receives."""
  plans, real = [], hip.mla_forward

  def spy(*args, **kw):
    plan = {}
    kw["flags"] = kw.get("flags", 0) | flags
    kw["plan_out"] = plan
    out = real(*args, **kw)
    plans.append(plan)
    return out

  hip.mla_forward = spy
  try:
    yield plans
  finally:
    hip.mla_forward = real


@contextlib.contextmanager
def _forced(hip, flags):
  """Every latent launch inside the block carries ``flags`` too (nothing else: a graph capture runs inside such a block)."""
  real = hip.mla_forward

  def with_flags(*args, **kw):
    kw["flags"] = kw.get("flags", 0) | flags
    return real(*args, **kw)

  hip.mla_forward = with_flags
  try:
    yield
  finally:
    hip.mla_forward = real


_CASES: dict = {}


def _case(lens, hq, hkv, sq, dtype, seed=0, pps=0, contiguous=0, page=PAGE, padded=False):
  """q, the FP8 latent pool (a view of a uint8-backed storage: one page more on either side, or — ``padded`` — a row more per page and 16 columns more per head; the
  NaN code in every byte no sequence owns), the shuffled block table and the lengths: made once per shape and shared (nothing writes to it: the append tests
  clone the storage).  Sequence-owned rows hold ``quantize_latent_rows(randn, 1)``; the LAST owned row of the longest sequence holds +-448 codes, and a
  sequence of length 1 holds a row of zero codes."""
  key = (tuple(lens), hq, hkv, sq, dtype, seed, pps, contiguous, page, padded)
  if key in _CASES:
    return _CASES[key]
  from ffpa_attn_amd import quantize_latent_rows

  g = torch.Generator(device="cuda").manual_seed(3000 + seed)
  tdt = R.TORCH_DTYPE[dtype]
  B = len(lens)
  q = torch.randn((B, sq, hq, D), generator=g, device="cuda", dtype=tdt)
  if contiguous:
    n_pages, page, table, ids = B, contiguous, None, None
    owner = lambda b, j: (b, j)
  else:
    pps = pps or -(-max(max(lens), 1) // page) + 1
    n_pages = B * pps + 3
    ids = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))[: B * pps].to(torch.int32).view(B, pps)
    table = ids.cuda()
    owner = lambda b, j: (int(ids[b, j // page]), j % page)
  codes = quantize_latent_rows(torch.randn((n_pages, page, hkv, D), generator=g, device="cuda", dtype=torch.float32), 1.0).view(torch.uint8)
  seen = torch.zeros((n_pages, page), dtype=torch.bool)
  for b, n in enumerate(lens):
    for j in range(n):
      seen[owner(b, j)] = True
  codes[~seen.cuda()] = NAN8
  longest = max(range(B), key=lambda b: lens[b])
  if lens[longest] > 1:
    codes[owner(longest, lens[longest] - 1)] = torch.tensor([0x7E, 0xFE], dtype=torch.uint8, device="cuda").repeat(D // 2)
  for b, n in enumerate(lens):
    if n == 1:
      codes[owner(b, 0)] = 0
  if padded:
    storage = torch.full((n_pages, page + 1, hkv, D + 16), NAN8, dtype=torch.uint8, device="cuda")
    view = storage[:, :page, :, :D]
  else:
    storage = torch.full((n_pages + 2, page, hkv, D), NAN8, dtype=torch.uint8, device="cuda")
    view = storage[1:-1]
  view.copy_(codes)
  t = dict(q=q, pool=view.view(F8), storage=storage, view=view, table=table, ids=ids, lens=torch.tensor(lens, dtype=torch.int32, device="cuda"), lens_list=list(lens),
           dtype=dtype, sq=sq, heads=(hq, hkv), page=page, capacity=contiguous or pps * page, refs={})
  _CASES[key] = t
  return t


def _pool_of(t, storage):
  """The case's pool view taken of another storage (a clone)."""
  return R.reviewed(t["view"], t["storage"], storage).view(F8)


def _fp8(hip, t, causal=False, *, kv_scale=1.0, num_splits=0, flags=0, lens=None, kv=None, pool=None, q=None, table="case"):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_fp8

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_fp8(t["q"] if q is None else q, t["pool"] if pool is None else pool, DV, kv_scale=kv_scale, kv=kv,
                                              cache_seqlens=t["lens"] if lens is None else lens, block_table=t["table"] if table == "case" else table,
                                              softmax_scale=SCALE, causal=causal, num_splits=num_splits, return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"ffpa_fwd_m16_mla_fp8_kernel<{t['dtype']}, 576, dv=512"), plans
  return out, lse, plans[0]


def _wide(hip, t, causal, kv_scale, *, num_splits=0, flags=0):
  """The 16-bit latent call on the dequantised pool: ``pool8.to(dtype)`` under ``softmax_scale * kv_scale``, O scaled by ``kv_scale``."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  pool16 = t["pool"].to(R.TORCH_DTYPE[t["dtype"]]).contiguous()
  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla(t["q"], pool16, DV, cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE * kv_scale, causal=causal,
                                          num_splits=num_splits, return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"ffpa_fwd_m16_mla_kernel<{t['dtype']}, 576, dv=512"), plans
  return out * kv_scale, lse, plans[0]


def _ref(t, causal, kv_scale, lens=None, pool=None):
  """float64 attention on the dequantised gathered rows with v = k[..., :DV] -> (attend's tuple, vstat of the dequantised visible values)."""
  lens = t["lens_list"] if lens is None else lens
  deq = (t["pool"] if pool is None else pool).double() * kv_scale
  o, lse, pmax, p2sum = R.attend(t["q"], deq, deq, lens, t["table"], causal, SCALE)
  return (o[..., :DV].contiguous(), lse, pmax, p2sum), R.visible_values(deq[..., :DV], lens, t["table"])


def _same_bits(a, b):
  return torch.equal(a.view(torch.int16) if a.element_size() == 2 else a.view(torch.int32), b.view(torch.int16) if b.element_size() == 2 else b.view(torch.int32))


# ----------------------------------------------------------------------------- 1. bit identity with the 16-bit kernel on the dequantised pool
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv", HEADS)
@pytest.mark.parametrize("sq", [1, 3])
def test_power_of_two_scales_return_the_bits_of_the_16_bit_call(hip, dtype, hq, hkv, sq):
  """kv_scale 1, 0.25 and 8; the same forced KV ranges (1, 2, 3, 5: ranges start at odd tiles, some are empty) and the same non-temporal choice, both forced on
  both calls.  The image the FP8 build writes is the image the LDS-DMA writes, and nothing behind the image differs: LSE (both dtypes) and bf16 O are the 16-bit
  call's bits.  The ten lengths are one batch; Sq = 3 runs causal."""
  causal = sq > 1
  t = _case(LENS, hq, hkv, sq, dtype, seed=hq + sq)
  runs = [(1.0, 1, hip.FLAG_NO_KV_STREAM), (1.0, 2, hip.FLAG_KV_STREAM), (0.25, 3, hip.FLAG_NO_KV_STREAM), (0.25, 1, hip.FLAG_KV_STREAM), (8.0, 5, hip.FLAG_KV_STREAM),
          (8.0, 2, hip.FLAG_NO_KV_STREAM)]
  for kv_scale, ns, stream in runs:
    flags = hip.FLAG_FORCE_SPLITS | stream
    out, lse, plan = _fp8(hip, t, causal, kv_scale=kv_scale, num_splits=ns, flags=flags)
    want, want_lse, want_plan = _wide(hip, t, causal, kv_scale, num_splits=ns, flags=flags)
    what = f"{dtype} heads {(hq, hkv)} Sq {sq} kv_scale {kv_scale} splits {ns} -> {plan}"
    assert plan["splits"] == ns == want_plan["splits"] and (", NT>" in plan["kernel"]) == (stream == hip.FLAG_KV_STREAM) == (", NT>" in want_plan["kernel"]), what
    assert plan["kernel"] == want_plan["kernel"].replace("_mla_kernel", "_mla_fp8_kernel") and plan["workgroups"] == want_plan["workgroups"], what
    assert out.shape == (len(LENS), sq, hq, DV) and (out[0] == 0).all() and torch.isneginf(lse[0]).all()
    assert _same_bits(lse, want_lse), f"LSE: {what}: {int((lse != want_lse).sum())} rows differ"
    if dtype == "bf16":
      assert _same_bits(out, want), f"O: {what}: {int((out != want).sum())} elements differ, max {(out.float() - want.float()).abs().max().item():.3e}"


# ----------------------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv", HEADS)
@pytest.mark.parametrize("sq", [1, 3])
def test_a_scale_that_is_no_power_of_two_against_float64(hip, dtype, hq, hkv, sq):
  """kv_scale = 0.37 on the same shapes — the batch holds a row of +-448 codes (the last key of the 300-key sequence) and a sequence whose only row is all zero
  codes — with the library's own split count and with three forced ranges."""
  causal = sq > 1
  t = _case(LENS, hq, hkv, sq, dtype, seed=hq + sq)
  assert ((t["view"][int(t["ids"][9, 299 // PAGE]), 299 % PAGE] & 0x7F) == 0x7E).all() and (t["view"][int(t["ids"][1, 0]), 0] == 0).all()
  ref, vstat = _ref(t, causal, 0.37)
  assert vstat[0] == pytest.approx(448 * 0.37)
  for kw in ({}, dict(num_splits=3, flags=hip.FLAG_FORCE_SPLITS)):
    out, lse, plan = _fp8(hip, t, causal, kv_scale=0.37, **kw)
    name = f"float64: {dtype} heads {(hq, hkv)} Sq {sq} causal={causal} {kw} -> {plan}"
    ratio = R.check(out, lse, ref, v=vstat, dtype=dtype, name=name)
    print(f"[mla fp8] {ratio:.3f} {name}")
  one = dict(t, q=t["q"][1:2], table=t["table"][1:2], lens=t["lens"][1:2], lens_list=[1])  # the zero row alone: p = 1 on a row of zeros
  if not causal:
    o1, l1, _ = _fp8(hip, one, False, kv_scale=0.37)
    assert (o1 == 0).all() and l1.abs().max().item() <= R.LSE_ATOL


# ----------------------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("layout", ["contiguous", "padded", "clamped id", "page 128"])
def test_layouts(hip, dtype, layout):
  """A contiguous cache of capacity 128 (one page per sequence through the identity table), a pool with padded page and row strides, a block table with an id
  past the pool (clamped to its last page) and pages of 128 keys: float64 at kv_scale 0.37 and the 16-bit call's bits at kv_scale 0.25."""
  lens = [1, 97, 128]
  kw = dict(contiguous=dict(contiguous=128), padded=dict(padded=True), **{"clamped id": dict(pps=3), "page 128": dict(page=128)})[layout]
  for sq in (1, 3):
    t = _case(lens, 16, 1, sq, dtype, seed=50 + sq, **kw)
    if layout == "clamped id":
      # sequence 0 (one key) names a page far past the pool in its first slot: the kernel and the reference read the pool's LAST page there
      t = dict(t, table=t["table"].clone(), refs={})
      t["table"][0, 0] = 1 << 20
      last = t["pool"].size(0) - 1
      fixed = t["storage"].clone()
      _pool_of(t, fixed).view(torch.uint8)[last, 0] = 0x38  # 1.0 in every column of the row that key reads
      t["pool"] = _pool_of(t, fixed)
    if layout == "padded":
      assert t["pool"].stride() == (65 * 592, 592, 592, 1)
    if layout == "contiguous":
      assert t["table"] is None and t["pool"].shape == (3, 128, 1, D)
    causal = sq > 1
    ref, vstat = _ref(t, causal, 0.37)
    out, lse, plan = _fp8(hip, t, causal, kv_scale=0.37)
    R.check(out, lse, ref, v=vstat, dtype=dtype, name=f"{layout}: {dtype} Sq {sq} -> {plan}")
    out2, lse2, _ = _fp8(hip, t, causal, kv_scale=0.25, num_splits=2, flags=hip.FLAG_FORCE_SPLITS)
    want, want_lse, _ = _wide(hip, t, causal, 0.25, num_splits=2, flags=hip.FLAG_FORCE_SPLITS)
    assert _same_bits(lse2, want_lse) and (dtype != "bf16" or _same_bits(out2, want)), f"{layout}: {dtype} Sq {sq}"


# ----------------------------------------------------------------------------- 4. the quantising appends
def _new_rows(shape, dtype, seed):
  """New latent rows in q's dtype: random values, the edge-value table at the head of every row, and ONE NaN (the first row's last column)."""
  g = torch.Generator(device="cuda").manual_seed(seed)
  kv = torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) * 3
  kv[..., : len(EDGES)] = torch.tensor(EDGES, device="cuda")
  kv = kv.to(R.TORCH_DTYPE[dtype])
  kv.view(-1, D)[0, D - 1] = float("nan")
  return kv


def _write_rows(t, storage, rows, base_lens, counts, kv_scale):
  """The append, written with torch IN PLACE on the pool view of ``storage``: ``rows [sum(counts), Hkv, D]`` -> the lengths after it."""
  from ffpa_attn_amd import quantize_latent_rows

  view = R.reviewed(t["view"], t["storage"], storage)
  codes = quantize_latent_rows(rows, kv_scale).view(torch.uint8)
  used, r = [], 0
  for b, n in enumerate(counts):
    base = max(base_lens[b], 0)
    used.append(min(base + n, t["capacity"]))
    for i in range(n):
      pos = base + i
      if pos < t["capacity"]:
        slab = (b, pos) if t["ids"] is None else (int(t["ids"][b, pos // t["page"]]), pos % t["page"])
        view[slab] = codes[r + i]
    r += n
  return used


def _same_codes(got, want):
  """Byte equality of two uint8 storages, NaN codes compared by NaN-ness."""
  gn, wn = (got & 0x7F) == 0x7F, (want & 0x7F) == 0x7F
  return torch.equal(gn, wn) and torch.equal(got[~gn], want[~wn])


def _same_out(a, b):
  """Bit equality of two outputs, NaN elements (the rows that read the appended NaN) compared by NaN-ness."""
  an, bn = torch.isnan(a), torch.isnan(b)
  return torch.equal(an, bn) and _same_bits(a.masked_fill(an, 0), b.masked_fill(bn, 0))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("snew", [1, 3])
@pytest.mark.parametrize("paged", [True, False])
@pytest.mark.parametrize("kv_scale", [0.37, 4.0])
def test_the_uniform_append_stores_quantize_latent_rows_and_nothing_else(hip, dtype, snew, paged, kv_scale):
  """``kv=`` at lengths 0, 31, 63 ... 65 (crossing a page) and 126 of 128 (the rows at and past the capacity are dropped): the whole storage equals the one the
  torch helper wrote — the NaN pages around the pool included —, exactly the appended rows changed, and the attention output is the FP8 call's on the pre-filled
  pool, bit for bit."""
  lens = [0, 31, 63, 64, 65, 126]
  t = _case(lens, 16, 1, snew, dtype, seed=40 + snew, pps=2, contiguous=0 if paged else 128)
  kv = _new_rows((len(lens), snew, 1, D), dtype, 77 + snew)
  got, want = t["storage"].clone(), t["storage"].clone()
  used = _write_rows(t, want, kv.reshape(-1, 1, D), lens, [snew] * len(lens), kv_scale)
  assert used == [min(n + snew, 128) for n in lens]
  before = t["lens"].clone()
  out, lse, plan = _fp8(hip, t, True, kv_scale=kv_scale, kv=kv, pool=_pool_of(t, got))
  assert torch.equal(t["lens"], before)  # (cache_seqlens is not advanced)
  assert _same_codes(got, want), "the cache's storage differs from the torch-written reference"
  touched = (want != t["storage"]).any(dim=-1).sum().item()
  assert touched == sum(u - n for u, n in zip(used, lens))  # (NaN rows became data: exactly the appended rows inside the capacity changed)
  again = _fp8(hip, t, True, kv_scale=kv_scale, pool=_pool_of(t, want), lens=torch.tensor(used, dtype=torch.int32, device="cuda"))
  assert _same_out(out, again[0]) and _same_out(lse, again[1])
  assert not torch.isnan(out[1:]).any()  # (the one NaN of kv is a latent row of sequence 0 and of no other)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kv_scale", [0.37, 4.0])
def test_the_ragged_append_stores_quantize_latent_rows_and_nothing_else(hip, dtype, kv_scale):
  """Token counts 0, 1, 3 and 5 at cache lengths 7, 63, 126 (of 128: one row dropped) and 0, with two padding rows behind the batch's last token."""
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache_mla_fp8

  counts, lens = [0, 1, 3, 5], [7, 63, 126, 0]
  t = _case(lens, 16, 1, 1, dtype, seed=60, pps=2)
  T = sum(counts)
  kv = _new_rows((T + 2, 1, D), dtype, 91)
  q = torch.randn((T + 2, 16, D), device="cuda", dtype=R.TORCH_DTYPE[dtype], generator=torch.Generator(device="cuda").manual_seed(92))
  cu = torch.tensor([0, 0, 1, 4, 9], dtype=torch.int32, device="cuda")
  got, want = t["storage"].clone(), t["storage"].clone()
  used = _write_rows(t, want, kv[:T], lens, counts, kv_scale)
  assert used == [7, 64, 128, 5]
  call = lambda pool, cache, rows: ffpa_attn_varlen_with_kvcache_mla_fp8(q, pool, DV, cu, 5, cache, t["table"], kv_scale=kv_scale, kv=rows, softmax_scale=SCALE,
                                                                         causal=True, return_softmax_lse=True)
  with _launches(hip) as plans:
    out, lse = call(_pool_of(t, got), t["lens"], kv)
  assert plans[0]["kernel"].startswith(f"ffpa_fwd_m16_mla_fp8_kernel<{dtype}, 576, dv=512"), plans
  assert _same_codes(got, want)
  assert (want != t["storage"]).any(dim=-1).sum().item() == 8  # (nine token rows, one past the capacity; the padding rows write nothing)
  again = call(_pool_of(t, want), torch.tensor(used, dtype=torch.int32, device="cuda"), None)
  assert _same_out(out[:T], again[0][:T]) and _same_out(lse[:, :T], again[1][:, :T])


# the placement rule of both quantising appends at its edges, in ONE call (tests/test_kvcache_mla_varlen_gpu.py holds the 16-bit appends to the same steps)
EDGE_STEPS = [((-1, 0, 126), (3, 0, 3)), ((-1, 0, 62, 126), (3, 0, 3, 3))]  # (lengths before the step, token rows of the ragged step; a uniform step brings 3 each)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hkv", [1, 2])
@pytest.mark.parametrize("lens, counts", EDGE_STEPS)
@pytest.mark.parametrize("kernel", ["uniform", "ragged"])
def test_both_quantising_appends_place_rows_by_one_rule_at_its_edges(hip, kernel, lens, counts, hkv, dtype):
  """One call of ``ffpa_mla_fp8_append_kernel`` (3 new rows per sequence) and of ``ffpa_mla_fp8_append_varlen_kernel`` (3, 0, 3 rows) at lengths -1 (acts as 0),
  0 and 126 of 128 (the third row is past the capacity) — and, with a fourth sequence, 62 (the rows cross into the next page): the pool's codes are those of
  ``quantize_latent_rows`` written with torch (no NaN among the new rows: the bytes compare as they are), ``used[]`` is written for every sequence, the one
  without a token included, and ``cache_seqlens`` is left alone."""
  from ffpa_attn_amd import quantize_latent_rows

  B, kv_scale = len(lens), 0.37
  counts = (3,) * B if kernel == "uniform" else counts
  g = torch.Generator(device="cuda").manual_seed(13 * hkv + B)
  pool = torch.randint(0, 256, (2 * B + 2, PAGE, hkv, D), device="cuda", generator=g, dtype=torch.uint8)
  ids = torch.randperm(2 * B + 2, device="cuda", generator=g)[:2 * B].to(torch.int32).view(B, 2)
  rows = torch.randn((sum(counts), hkv, D), device="cuda", generator=g).to(R.TORCH_DTYPE[dtype])
  codes = quantize_latent_rows(rows, kv_scale).view(torch.uint8)
  want, used_want, r = pool.clone(), [], 0
  for b, (n, c) in enumerate(zip(lens, counts)):
    base = max(n, 0)
    used_want.append(min(base + c, 2 * PAGE))
    for pos in range(base, min(base + c, 2 * PAGE)):
      want[int(ids[b, pos // PAGE]), pos % PAGE] = codes[r + pos - base]
    r += c
  lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
  cu = torch.tensor(np.concatenate(([0], np.cumsum(counts))), dtype=torch.int32, device="cuda")
  got = pool.clone()
  if kernel == "uniform":
    q = torch.randn((3 * B, 16, D), device="cuda", generator=g).to(rows.dtype)
    used = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.ops.ffpa_attn._mla_fp8_fwd_hip(q, got.view(F8), DV, kv_scale, cu, used, ids, rows.view(B, 3, hkv, D), lens_t, 3, 2 * PAGE, SCALE, 1, 0)
  else:
    used = torch.ops.ffpa_attn._mla_fp8_append_varlen_hip(got.view(F8), rows, kv_scale, cu, lens_t, ids)
  assert used.tolist() == used_want
  assert torch.equal(got, want), "the pool's codes differ from the torch-written ones"
  assert lens_t.tolist() == list(lens)


# ----------------------------------------------------------------------------- 5. the ragged call
RAGGED = [([1, 1, 1, 40], [300, 33, 0, 97]), ([1, 1, 1, 40, 1, 1], [300, 33, 0, 97, 64, 65])]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv", [(128, 1), (32, 2)])
@pytest.mark.parametrize("counts, lens", RAGGED)
def test_each_ragged_sequence_has_the_bits_of_the_uniform_fp8_call_on_it_alone(hip, dtype, hq, hkv, counts, lens):
  """1 + 1 + 1 + 40 tokens over 300, 33, 0 and 97 cached keys — and the same batch with two decodes more —, ``num_splits = 1``: the rows of sequence b are
  ``ffpa_attn_with_kvcache_mla_fp8`` on that sequence alone (Sq = Sq_b, its row of the table, its length), O and LSE bit for bit — and float64 per sequence.
  The grid is the 16-bit latent call's (``hip.mla_compact_slots``): at 128 heads the plan's three-quarter rule leaves the four-sequence batch on the full grid
  (90 slots x 4 > 4 x 80 row tiles) and takes the compact grid on the six-sequence one (96 slots against 480 row tiles)."""
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache_mla_fp8, ffpa_attn_with_kvcache_mla_fp8

  t = _case(lens, hq, hkv, 1, dtype, seed=70 + hq)
  T = sum(counts)
  q = torch.randn((T, hq, D), device="cuda", dtype=R.TORCH_DTYPE[dtype], generator=torch.Generator(device="cuda").manual_seed(71))
  cu = torch.tensor(np.concatenate(([0], np.cumsum(counts))), dtype=torch.int32, device="cuda")
  for causal in (True, False):
    with _launches(hip) as plans:
      out, lse = ffpa_attn_varlen_with_kvcache_mla_fp8(q, t["pool"], DV, cu, 40, t["lens"], t["table"], kv_scale=0.37, softmax_scale=SCALE, causal=causal, num_splits=1,
                                                       return_softmax_lse=True)
    plan = plans[0]
    assert plan["kernel"].startswith(f"ffpa_fwd_m16_mla_fp8_kernel<{dtype}, 576, dv=512") and plan["splits"] == 1, plan
    assert plan["compact_slots"] == hip.mla_compact_slots(hq // hkv, counts) and (plan["compact_slots"] > 0) == ("compact grid" in plan["kernel"]), plan
    assert (plan["compact_slots"] == 96) == (hq == 128 and len(counts) == 6), plan
    assert out.shape == (T, hq, DV) and lse.shape == (hq, T)
    row = 0
    for b, n in enumerate(counts):
      one, one_lse = ffpa_attn_with_kvcache_mla_fp8(q[row:row + n][None], t["pool"], DV, kv_scale=0.37, cache_seqlens=t["lens"][b:b + 1], block_table=t["table"][b:b + 1],
                                                    softmax_scale=SCALE, causal=causal, num_splits=1, return_softmax_lse=True)
      assert _same_bits(out[row:row + n], one[0]) and _same_bits(lse[:, row:row + n], one_lse[0]), f"sequence {b} ({n} tokens over {lens[b]} keys, causal={causal})"
      if lens[b] == 0:
        assert (one == 0).all() and torch.isneginf(one_lse).all()
      else:
        deq = t["pool"].double() * 0.37
        o, l, pmax, p2sum = R.attend(q[row:row + n][None], deq, deq, [lens[b]], t["table"][b:b + 1], causal, SCALE)
        R.check(one, one_lse, (o[..., :DV].contiguous(), l, pmax, p2sum), v=R.visible_values(deq[..., :DV], [lens[b]], t["table"][b:b + 1]), dtype=dtype,
                name=f"ragged: sequence {b} causal={causal}")
      row += n


# ----------------------------------------------------------------------------- 6. graph capture
def test_one_graph_follows_lengths_table_and_new_rows_written_in_place(hip):
  """Quantising append + attention + merge (three forced ranges ride in the captured plan) captured once; replays after cache_seqlens, block_table and kv were
  rewritten in place: each equals the eager call on the same state, storage included."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_fp8

  lens0 = [5, 31, 64, 200]
  t = _case(lens0, 16, 1, 1, "bf16", seed=9, pps=5)
  storage = t["storage"].clone()
  storage[(storage & 0x7F) == 0x7F] = 0x30  # (replays move lengths and pages around: every row must hold a number)
  pool = _pool_of(t, storage)
  lens, table = t["lens"].clone(), t["table"].clone()
  kv = torch.randn((4, 1, 1, D), device="cuda", dtype=torch.bfloat16)
  call = lambda p: ffpa_attn_with_kvcache_mla_fp8(t["q"], p, DV, kv_scale=0.37, kv=kv, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, causal=True,
                                                  num_splits=3, return_softmax_lse=True)
  with _launches(hip, hip.FLAG_FORCE_SPLITS) as plans:
    call(pool.clone())  # (warm: the library is loaded, the scratch is sized)
  assert len(plans) == 1 and "ffpa_varlen_merge_kernel" in plans[0]["kernel"] and plans[0]["splits"] == 3, plans
  with _forced(hip, hip.FLAG_FORCE_SPLITS):
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      out_g, lse_g = call(pool)
    states = [(lens0, table.clone(), kv.clone()), ([0, 63, 65, 97], table.flip(0).contiguous(), torch.randn_like(kv)),
              ([33, 1, 129, 300], table.roll(1, 0).contiguous(), torch.randn_like(kv))]
    for n, tb, rows in states:
      lens.copy_(torch.tensor(n, dtype=torch.int32, device="cuda"))
      table.copy_(tb)
      kv.copy_(rows)
      snapshot = storage.clone()
      graph.replay()
      torch.cuda.synchronize()
      after = storage.clone()
      storage.copy_(snapshot)
      eager = call(pool)
      torch.cuda.synchronize()
      assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1]), n
      assert torch.equal(after, storage) and not torch.equal(after, snapshot), n
      tt = dict(t, table=table)
      ref, vstat = _ref(tt, True, 0.37, lens=[x + 1 for x in n], pool=pool)
      R.check(out_g, lse_g, ref, v=vstat, dtype="bf16", name=f"graph replay at {n}")


# ----------------------------------------------------------------------------- 7. torch.compile
def test_the_uniform_call_under_torch_compile_fullgraph(hip):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_fp8

  lens = [70, 0, 129]
  t = _case(lens, 16, 1, 3, "fp16", seed=88, pps=4)
  kv = _new_rows((3, 3, 1, D), "fp16", 89)
  kv.nan_to_num_(nan=0.5)

  def f(q, pool, rows, cache, table):
    o, lse = ffpa_attn_with_kvcache_mla_fp8(q, pool, DV, kv_scale=0.37, kv=rows, cache_seqlens=cache, block_table=table, softmax_scale=SCALE, causal=True,
                                            return_softmax_lse=True)
    return o * 2, lse

  s_eager, s_compiled = t["storage"].clone(), t["storage"].clone()
  with _launches(hip) as plans:
    eager = f(t["q"], _pool_of(t, s_eager), kv, t["lens"], t["table"])
  assert len(plans) == 1 and plans[0]["kernel"].startswith("ffpa_fwd_m16_mla_fp8_kernel<fp16, 576, dv=512"), plans
  compiled = torch.compile(f, fullgraph=True)(t["q"], _pool_of(t, s_compiled), kv, t["lens"], t["table"])
  torch.cuda.synchronize()
  assert torch.equal(eager[0], compiled[0]) and torch.equal(eager[1], compiled[1])
  assert torch.equal(s_eager, s_compiled) and not torch.equal(s_eager, t["storage"])
  want = t["storage"].clone()
  used = _write_rows(t, want, kv.reshape(-1, 1, D), lens, [3, 3, 3], 0.37)
  assert torch.equal(s_compiled, want)
  ref, vstat = _ref(t, True, 0.37, lens=used, pool=_pool_of(t, want))
  R.check((compiled[0].double() / 2).to(torch.float16), compiled[1], ref, v=vstat, dtype="fp16", name="torch.compile")


# ----------------------------------------------------------------------------- 8. FP8 pools past 2^32 bytes
# tests/test_kvcache_mla_contract_gpu.py section f, for the builds that count the pool in BYTES through strides in two-byte units (k_ps = k_page_stride * 2u): the
# FP8 latent call with and without kv=, the tree call and the cascade.  The pools are ~ 4.3 GB of the NaN code; float64 and the 16-bit twin work on the USED pages
# alone, gathered into a small pool under a remapped table (the twin's pool would be 8.6 GB, a float64 copy 34 GB).
HIGH_LENS = [700, 1500, 1027]


def _high_pool(page):
  """``[num_pages, page, 1, 576]`` uint8, every byte the NaN code, whose used pages — the highest ids, shuffled — all START past byte 2^32; sequence b holds
  ``HIGH_LENS[b]`` rows of codes.  -> the storage, the table, the table of the cascade (every sequence reads its first page through sequence 0's id)."""
  from ffpa_attn_amd import quantize_latent_rows

  B, pps = len(HIGH_LENS), -(-(max(HIGH_LENS) + 2) // page) + 1
  n_pages = -(-(2 ** 32) // (page * D)) + B * pps
  storage = torch.full((n_pages, page, 1, D), 0xFF, dtype=torch.uint8, device="cuda")
  ids = (n_pages - 1 - torch.randperm(B * pps, generator=torch.Generator().manual_seed(page))).to(torch.int32).view(B, pps)
  assert int(ids.min()) * storage.stride(0) >= 2 ** 32, "the used pages must start past byte 2^32"
  g = torch.Generator(device="cuda").manual_seed(page)
  for b, n in enumerate(HIGH_LENS):
    j = torch.arange(n)
    storage[ids[b].long()[j // page].cuda(), (j % page).cuda()] = quantize_latent_rows(torch.randn((n, 1, D), device="cuda", generator=g), 1.0).view(torch.uint8)
  shared = ids.clone()
  shared[:, 0] = ids[0, 0]
  return storage, ids, shared


def _gathered(storage, ids):
  """The pages ``ids`` names, gathered into a small pool, and ``ids`` remapped to it."""
  flat = ids.flatten().long()
  return storage[flat.cuda()].contiguous(), torch.arange(flat.numel(), dtype=torch.int32, device="cuda").view(ids.shape)


def _float64_on(small, table, q, lens, kv_scale, causal=True, mask=None):
  import tree_ref

  deq = small.view(F8).double() * kv_scale
  if mask is not None:
    o, lse, pmax, p2sum = tree_ref.attend_tree(q, deq, deq, lens, table, mask, SCALE)
  else:
    o, lse, pmax, p2sum = R.attend(q, deq, deq, lens, table, causal, SCALE)
  return (o[..., :DV].contiguous(), lse, pmax, p2sum), R.visible_values(deq[..., :DV], lens, table)


@pytest.mark.parametrize("page", [64, 256])
def test_fp8_pool_pages_past_2_32_bytes(hip, page):
  """The FP8 latent call (non-temporal and plain, unsplit and three forced ranges), the tree call and the cascade against float64 at kv_scale 0.37; the 16-bit
  call's bits at 0.25 on the dequantised used pages; then ``kv=``: the used pages hold ``quantize_latent_rows`` of the new rows, every other byte its 0xFF."""
  import tree_ref
  from ffpa_attn_amd import (ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_cascade_fp8, ffpa_attn_with_kvcache_mla_tree_fp8, quantize_latent_rows)

  storage, ids, shared = _high_pool(page)
  low, B, sq, lens = int(ids.min()), len(HIGH_LENS), 2, HIGH_LENS
  g = torch.Generator(device="cuda").manual_seed(11)
  q = torch.randn((B, sq, 16, D), device="cuda", generator=g).bfloat16()
  t = dict(q=q, pool=storage.view(F8), table=ids.cuda(), lens=torch.tensor(lens, dtype=torch.int32, device="cuda"), dtype="bf16")
  small, remap = _gathered(storage, ids)
  ref, vstat = _float64_on(small, remap, q, lens, 0.37)
  for flag in (hip.FLAG_KV_STREAM, hip.FLAG_NO_KV_STREAM):
    for ns in (1, 3):
      out, lse, plan = _fp8(hip, t, True, kv_scale=0.37, num_splits=ns, flags=flag | (hip.FLAG_FORCE_SPLITS if ns > 1 else 0))
      assert plan["splits"] == ns and ((", NT>" in plan["kernel"]) == (flag == hip.FLAG_KV_STREAM)), plan
      print(f"[mla fp8 > 2^32 bytes] page {page} {R.check(out, lse, ref, v=vstat, dtype='bf16', name=f'page {page} past 2^32 bytes {plan}'):.3f} {plan}")
  # the 16-bit call's bits at a power-of-two scale, on the used pages dequantised
  flags = hip.FLAG_FORCE_SPLITS | hip.FLAG_NO_KV_STREAM
  out, lse, plan = _fp8(hip, t, True, kv_scale=0.25, num_splits=3, flags=flags)
  with _launches(hip, flags) as plans:
    want, want_lse = ffpa_attn_with_kvcache_mla(q, small.view(F8).to(torch.bfloat16), DV, cache_seqlens=t["lens"], block_table=remap, softmax_scale=SCALE * 0.25,
                                                causal=True, num_splits=3, return_softmax_lse=True)
  assert plans[0]["splits"] == plan["splits"] == 3 and plans[0]["kernel"] == plan["kernel"].replace("_mla_fp8_kernel", "_mla_kernel"), (plan, plans)
  assert _same_bits(lse, want_lse) and _same_bits(out, want * 0.25)
  # the tree call
  mask = tree_ref.tree_mask_from_parents([-1, 0]).cuda()
  with _launches(hip) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_tree_fp8(q, t["pool"], DV, kv_scale=0.37, tree_mask=mask, cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE,
                                                   return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith("ffpa_fwd_m16_mla_tree_fp8_kernel<bf16"), plans
  tref, tstat = _float64_on(small, remap, q, lens, 0.37, mask=mask)
  print(f"[mla tree fp8 > 2^32 bytes] page {page} {R.check(out, lse, tref, v=tstat, dtype='bf16', name=f'tree, page {page} past 2^32 bytes'):.3f}")
  # the cascade: every sequence reads its first page through sequence 0's row — the prefix pass and the shifted table rows of the suffix pass
  with _launches(hip) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_cascade_fp8(q, t["pool"], DV, shared_prefix_len=page, kv_scale=0.37, cache_seqlens=t["lens"], block_table=shared.cuda(),
                                                      softmax_scale=SCALE, causal=True, return_softmax_lse=True, cascade=True)
  assert len(plans) == 2 and all(p["kernel"].startswith("ffpa_fwd_m16_mla_fp8_kernel<bf16") for p in plans), plans
  csmall, cremap = _gathered(storage, shared)
  cref, cstat = _float64_on(csmall, cremap, q, lens, 0.37)
  print(f"[mla cascade fp8 > 2^32 bytes] page {page} {R.check(out, lse, cref, v=cstat, dtype='bf16', name=f'cascade, page {page} past 2^32 bytes'):.3f}")
  # kv=: two rows per sequence
  kv = torch.randn((B, sq, 1, D), device="cuda", generator=g).bfloat16()
  want = storage.clone()
  codes = quantize_latent_rows(kv, 0.37).view(torch.uint8)
  for b, n in enumerate(lens):
    for i in range(sq):
      want[int(ids[b, (n + i) // page]), (n + i) % page] = codes[b, i]
  out, lse, plan = _fp8(hip, t, True, kv_scale=0.37, kv=kv)
  assert torch.equal(storage, want) and (storage[:low] == 0xFF).all() and int((want != 0xFF).any(dim=-1).sum()) == sum(lens) + B * sq
  used = [n + sq for n in lens]
  small, remap = _gathered(want, ids)
  ref, vstat = _float64_on(small, remap, q, used, 0.37)
  print(f"[mla fp8 append > 2^32 bytes] page {page} {R.check(out, lse, ref, v=vstat, dtype='bf16', name=f'append, page {page} past 2^32 bytes {plan}'):.3f}")
  del storage, want, t
  torch.cuda.empty_cache()


def test_fp8_contiguous_cache_whose_last_slabs_start_past_2_32_bytes(hip):
  """A contiguous FP8 cache [913, 8192, 1, 576] (4.3 GB) in which only the last two slabs hold keys: the FP8 call and the tree call, then ``kv=`` — every sequence
  appends, so the NaN slabs receive rows 0 and 1 and nothing else."""
  import tree_ref
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_tree_fp8, quantize_latent_rows

  B, cap, sq = 913, 8192, 2
  g = torch.Generator(device="cuda").manual_seed(12)
  storage = torch.full((B, cap, 1, D), 0xFF, dtype=torch.uint8, device="cuda")
  lens = [0] * (B - 2) + [1500, 700]
  assert (B - 2) * storage.stride(0) >= 2 ** 32, "the last two slabs must start past byte 2^32"
  for b in (B - 2, B - 1):
    storage[b, :lens[b]] = quantize_latent_rows(torch.randn((lens[b], 1, D), device="cuda", generator=g), 1.0).view(torch.uint8)
  q = torch.randn((B, sq, 16, D), device="cuda", generator=g).bfloat16()
  t = dict(q=q, pool=storage.view(F8), table=None, lens=torch.tensor(lens, dtype=torch.int32, device="cuda"), dtype="bf16")
  ref, vstat = _float64_on(storage[B - 2:], None, q[B - 2:], lens[B - 2:], 0.37)
  for ns, flag in ((1, hip.FLAG_KV_STREAM), (3, hip.FLAG_NO_KV_STREAM | hip.FLAG_FORCE_SPLITS)):
    out, lse, plan = _fp8(hip, t, True, kv_scale=0.37, num_splits=ns, flags=flag)
    assert plan["splits"] == ns and (out[:B - 2] == 0).all() and torch.isneginf(lse[:B - 2]).all(), plan
    print(f"[mla fp8 contiguous > 2^32 bytes] {R.check(out[B - 2:], lse[B - 2:], ref, v=vstat, dtype='bf16', name=f'contiguous past 2^32 bytes {plan}'):.3f} {plan}")
  mask = tree_ref.tree_mask_from_parents([-1, 0]).cuda()
  out, lse = ffpa_attn_with_kvcache_mla_tree_fp8(q, t["pool"], DV, kv_scale=0.37, tree_mask=mask, cache_seqlens=t["lens"], softmax_scale=SCALE, return_softmax_lse=True)
  tref, tstat = _float64_on(storage[B - 2:], None, q[B - 2:], lens[B - 2:], 0.37, mask=mask)
  assert (out[:B - 2] == 0).all() and torch.isneginf(lse[:B - 2]).all()
  print(f"[mla tree fp8 contiguous > 2^32 bytes] {R.check(out[B - 2:], lse[B - 2:], tref, v=tstat, dtype='bf16', name='tree, contiguous past 2^32 bytes'):.3f}")
  kv = torch.randn((B, sq, 1, D), device="cuda", generator=g).bfloat16()
  want = storage.clone()
  codes = quantize_latent_rows(kv, 0.37).view(torch.uint8)
  for b in range(B):
    want[b, lens[b]:lens[b] + sq] = codes[b]
  out, lse, plan = _fp8(hip, t, True, kv_scale=0.37, kv=kv)
  assert torch.equal(storage, want) and (storage[:B - 2, sq:] == 0xFF).all() and not (storage[:B - 2, :sq] == 0xFF).all(dim=-1).any()
  head, hstat = _float64_on(want[:B - 2, :64], None, q[:B - 2], [sq] * (B - 2), 0.37)  # (the first rows of the slabs that held nothing: the two new rows)
  tail, tstat = _float64_on(want[B - 2:], None, q[B - 2:], [n + sq for n in lens[B - 2:]], 0.37)
  print(f"[mla fp8 append contiguous > 2^32 bytes] {R.check(out[:B - 2], lse[:B - 2], head, v=hstat, dtype='bf16', name='append into the empty slabs'):.3f} "
        f"{R.check(out[B - 2:], lse[B - 2:], tail, v=tstat, dtype='bf16', name='append into the last two slabs'):.3f}")
  del storage, want, t
  torch.cuda.empty_cache()
