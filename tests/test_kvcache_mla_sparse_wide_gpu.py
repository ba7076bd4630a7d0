"""``wide_pool=True`` on the three sparse latent calls, on the GPU: the builds whose lanes form 64-bit global addresses (no descriptor; a key past a token's count
reads the library's zero row).  Every comparison is EXACT — the wide build against the narrow build, bit for bit — or the sparse suite's float64 allowance
(tests/kvcache_mla_sparse_ref.py / ``kvcache_ref.check``, unchanged).  D = 576, head_dim_v = 512, scale 1 / sqrt(192); tiles hold 32 keys.

1. a pool inside the narrow reach: the bits of ``wide_pool=False``, with the entries past the counts holding -1, 2^31 - 1 and the id of a NaN row;
2. a pool of rows ~9 MB apart, spanning more than 2^33 bytes and never filled: the bits of the narrow call on a compacted copy of the selected rows — the rows
   lie on both sides of byte 2^31, 2^32 (what catches a 32-bit product) and 2^33; head-major with two latent heads, the second head's base lies past 2^32 too;
3. one HIP graph of the wide call follows indices, counts and pool rows rewritten in place."""

import pytest
import torch

import kvcache_mla_sparse_ref as SR
import kvcache_ref as R
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D, DV = 576, 512
SCALE = 192 ** -0.5
KV_SCALE = 0.5
KINDS = [("16bit", torch.bfloat16), ("16bit", torch.float16), ("fp8", torch.bfloat16), ("fp8", torch.float16), ("ds", torch.bfloat16)]
IDS = [f"{k}-{str(d)[6:]}" for k, d in KINDS]
STRIDE_BYTES = 9_000_000  # between two rows of the far pool: a multiple of 16, below 2^24 elements in every pool format
_FAR = {}


def _pack(kind, dtype, rows):
  """Latent rows ``[..., 576]`` (float32) in the pool format of the kind."""
  from ffpa_attn_amd import pack_latent_rows_ds

  if kind == "ds":
    return pack_latent_rows_ds(rows.to(torch.bfloat16))
  return (rows / KV_SCALE).to(torch.float8_e4m3fn) if kind == "fp8" else rows.to(dtype)


def _values(kind, pool):
  """What the kernel computes on, float64."""
  from ffpa_attn_amd import unpack_latent_rows_ds

  return unpack_latent_rows_ds(pool).double() if kind == "ds" else pool.float().double() * (KV_SCALE if kind == "fp8" else 1.0)


def _raw(t):
  """The tensor's bytes as integers (indexing and copies that no dtype rule can refuse)."""
  return t.view(torch.uint8 if t.element_size() == 1 else torch.int16)


def _call(kind, q, pool, idx, lens, wide, num_splits=0):
  import ffpa_attn_amd as F

  fn, kw = {"16bit": (F.ffpa_attn_with_kvcache_mla_sparse, {}), "fp8": (F.ffpa_attn_with_kvcache_mla_sparse_fp8, dict(kv_scale=KV_SCALE)),
            "ds": (F.ffpa_attn_with_kvcache_mla_sparse_ds, {})}[kind]
  return fn(q, pool, DV, idx, topk_lens=lens, softmax_scale=SCALE, num_splits=num_splits, return_softmax_lse=True, wide_pool=wide, **kw)


def _same_bits(a, b, what):
  assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), what


@pytest.mark.parametrize("hq", [16, 128])
@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_inside_the_narrow_reach_the_wide_build_returns_the_narrow_build_s_bits(hip, kind, dtype, hq):
  """topk = 96 is three tiles (the ids loaded a tile ahead run past one step); the counts are 0, 1, inside a tile, a tile border and topk."""
  g = torch.Generator(device="cuda").manual_seed(11)
  rows, topk, counts = 3000, 96, [0, 1, 20, 64, 96]
  nan_row = 1234
  pool = _pack(kind, dtype, torch.randn((rows, 1, D), generator=g, device="cuda"))
  _raw(pool)[nan_row] = -1  # (every bit set: NaN as bf16, as fp16, as an e4m3 code and as a scale)
  q = torch.randn((len(counts), hq, D), generator=g, device="cuda").to(dtype)
  idx = torch.randint(0, rows, (len(counts), topk), generator=g, device="cuda", dtype=torch.int32)
  idx[idx == nan_row] = 0
  for t, n in enumerate(counts):
    idx[t, n:] = torch.tensor([-1, 2 ** 31 - 1, nan_row], dtype=torch.int32, device="cuda").repeat(topk)[: topk - n]
  lens = torch.tensor(counts, dtype=torch.int32, device="cuda")
  for num_splits in (1, 3):
    narrow, wide = _call(kind, q, pool, idx, lens, False, num_splits), _call(kind, q, pool, idx, lens, True, num_splits)
    _same_bits(wide, narrow, f"num_splits={num_splits}")
    assert not wide[0].isnan().any() and (wide[0][0] == 0).all() and wide[1][:, 0].isneginf().all()


def _far_pool(kind, dtype, rows, hkv):
  """``[rows, hkv, row]`` over ONE uninitialised buffer shared by every case (never filled): rows STRIDE_BYTES apart, heads ``rows`` rows apart (head-major)."""
  nbytes = 1000 * STRIDE_BYTES
  assert rows * hkv * STRIDE_BYTES <= nbytes
  if "buf" not in _FAR:
    _FAR["buf"] = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
  pdt = torch.uint8 if kind == "ds" else torch.float8_e4m3fn if kind == "fp8" else dtype
  row = STRIDE_BYTES // pdt.itemsize
  return _FAR["buf"].view(pdt).as_strided((rows, hkv, 656 if kind == "ds" else D), (row, rows * row, 1))


@pytest.mark.parametrize("rows,hkv", [(1000, 1), (500, 2)], ids=["flat", "two-heads-head-major"])
@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_a_pool_past_2_33_bytes_returns_the_bits_of_the_narrow_call_on_the_compacted_rows(hip, kind, dtype, rows, hkv):
  g = torch.Generator(device="cuda").manual_seed(12)
  pool = _far_pool(kind, dtype, rows, hkv)
  assert (rows * hkv - 1) * STRIDE_BYTES > 2 ** 33 and (hkv == 1 or rows * STRIDE_BYTES > 2 ** 32)
  edges = [r for e in (31, 32, 33) for r in (2 ** e // STRIDE_BYTES, 2 ** e // STRIDE_BYTES + 1) if r < rows]
  # (48+ distinct rows and lists WITHOUT duplicates: a row listed k times carries k equal weights whose bf16 roundings add up in phase, which the allowance's
  #  per-key statistics do not model — measured on lists of 40 entries over 10 rows: one row weighed 0.64 under a largest per-key weight of 0.11)
  must = sorted({0, rows - 1, *edges})
  sel = torch.tensor(must + sorted(set(range(3, rows, rows // 41)) - set(must)), device="cuda")
  assert len(edges) == (6 if hkv == 1 else 4) and len(sel) >= 48
  with pytest.raises(ValueError, match=r"2\^31"):
    _call(kind, torch.empty((1, 16 * hkv, D), dtype=dtype, device="cuda"), pool, torch.zeros((1, 1), dtype=torch.int32, device="cuda"), None, False)
  _raw(pool)[sel] = _raw(_pack(kind, dtype, torch.randn((len(sel), hkv, D), generator=g, device="cuda")))  # (only the rows the tokens select are ever written)
  compact = _raw(pool)[sel].contiguous().view(pool.dtype)
  topk, counts = 40, [40, 33, 9]
  where = torch.stack([torch.randperm(len(sel), generator=g, device="cuda")[:topk] for _ in counts])
  where[0] = torch.arange(topk, device="cuda")  # (token 0 reads row 0, the last row and every row next to 2^31, 2^32 and 2^33)
  idx, idx_c = sel[where].to(torch.int32), where.to(torch.int32)
  for t, n in enumerate(counts):
    idx[t, n:] = idx_c[t, n:] = -1
  lens = torch.tensor(counts, dtype=torch.int32, device="cuda")
  q = torch.randn((len(counts), 16 * hkv, D), generator=g, device="cuda").to(dtype)
  for num_splits in (1, 2):
    wide = _call(kind, q, pool, idx, lens, True, num_splits)
    _same_bits(wide, _call(kind, q, compact, idx_c, lens, False, num_splits), f"num_splits={num_splits}")
  vals = _values(kind, compact)
  R.check(wide[0][:, None], wide[1].t()[:, :, None], SR.reference(q, vals, idx_c, counts, SCALE, DV), v=SR.visible_values(vals, idx_c, counts, DV),
          dtype="bf16" if dtype == torch.bfloat16 else "fp16", name=f"{kind} far pool")


@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_one_graph_of_the_wide_call_follows_indices_counts_and_rows_written_in_place(hip, kind, dtype):
  g = torch.Generator(device="cuda").manual_seed(13)
  rows, topk = 2048, 96
  pool = _pack(kind, dtype, torch.randn((rows, 1, D), generator=g, device="cuda"))
  q = torch.randn((4, 16, D), generator=g, device="cuda").to(dtype)
  idx = torch.randint(0, rows, (4, topk), generator=g, device="cuda", dtype=torch.int32)
  lens = torch.tensor([96, 5, 64, 33], dtype=torch.int32, device="cuda")
  call = lambda: _call(kind, q, pool, idx, lens, True, 2)
  call()  # (warm: the library is loaded, the scratch is sized)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out_g = call()
  seen = []
  for counts in ([96, 5, 64, 33], [0, 96, 31, 70], [1, 32, 96, 65]):
    if seen:
      idx.copy_(torch.randint(0, rows, (4, topk), generator=g, device="cuda", dtype=torch.int32))
      new = torch.randperm(rows, generator=g, device="cuda")[:300]
      _raw(pool)[new] = _raw(_pack(kind, dtype, torch.randn((300, 1, D), generator=g, device="cuda")))
    lens.copy_(torch.tensor(counts, dtype=torch.int32, device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(out_g, call(), f"replay at {counts}")
    assert all(not torch.equal(out_g[0], o) for o in seen)  # (the replay returns the NEW bits)
    seen.append(out_g[0].clone())
