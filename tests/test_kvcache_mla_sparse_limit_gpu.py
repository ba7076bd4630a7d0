"""The three gather kernels — ``ffpa_attn_with_kvcache_mla_sparse``, ``_sparse_fp8`` and ``_sparse_ds`` — at the reach of their addressing: a latent head's rows
are addressed through ONE buffer descriptor of at most 2^31 bytes with 32-bit lane offsets whose bit 31 means "no row", so the pools here are the largest the host
accepts — dense rows of 1152 / 576 / 656 bytes up to 128 / 128 / 80 bytes short of 2^31, 2048 rows 1 MiB apart, and two heads of the largest span each, the
second ending at the pool's last byte.  A pool is ~ 2 ... 4 GiB of 0xFF (NaN in every format) inside an owning storage with 64 KiB of 0xFF on either side; only
the rows a token selects hold data.  The index lists name row 0, row 1, the last rows, the rows around byte offset 2^30, the 64 rows below the span's end, random
rows of the whole pool, ids outside the pool in front of a count (``INT_MAX`` and ``num_rows`` clamp to the last row, ``INT_MIN`` and -1 to row 0) and, behind
every count, the last row's id, ``INT_MAX``, 2^30 and -1.

Checks: (1) ``kvcache_ref.check``, unchanged, against float64 attention over the rows gathered per token (dequantised); (2) NO TOLERANCE: O and LSE are the bits of
the same call — same ``num_splits``, flags and non-temporal build, the same ``splits`` in its plan — on a COMPACTED pool that holds only the referenced rows, in
shuffled order, under the remapped index list: no arithmetic of these kernels depends on an address; (3) everything finite; (4) the guard bytes around the pool
unchanged; (5) ``store_latent_rows_ds`` into the last row and into row ``2^30 // 656`` of the full-size pool writes ``pack_latent_rows_ds``'s bytes and nothing else."""

import random

import pytest
import torch

import kvcache_ref as R
from kvcache_mla_family_ref import INT_MAX, INT_MIN
from kvcache_mla_sparse_ref import gathered
from test_fwd_gpu import hip  # noqa: F401  (fixture)
from test_kvcache_mla_family_gpu import _launches

pytestmark = pytest.mark.gpu

D, DV = 576, 512
SCALE = 192 ** -0.5
KV_SCALE = 0.37
SPAN = 2 ** 31
GUARD = 64 * 1024
ROW_BYTES = {"16bit": 2 * D, "fp8": D, "ds": 656}
MAX_ROWS = {"16bit": 1864135, "fp8": 3728270, "ds": 3273603}  # (2^31 - row) // row + 1: the span is 128, 128 and 80 bytes short of 2^31
T, TOPK, COUNTS = 4, 300, (0, 33, 300, 300)
KERNEL = {"16bit": "ffpa_fwd_m16_mla_sparse_kernel", "fp8": "ffpa_fwd_m16_mla_sparse_fp8_kernel", "ds": "ffpa_fwd_m16_mla_sparse_ds_kernel"}


def _elem(fmt, dtype):
  return dtype if fmt == "16bit" else torch.uint8


def _pool(fmt, kind, dtype):
  """-> ``(storage: uint8, 0xFF, owning; view: the pool in its element type [rows, Hkv, width]; rows; slot stride in bytes)``."""
  row = ROW_BYTES[fmt]
  es = 2 if fmt == "16bit" else 1
  if kind == "strided":
    rows, stride, heads, body = 2048, 2 ** 20, 1, SPAN
  else:
    rows, stride, heads = MAX_ROWS[fmt], row, 2 if kind == "two_heads" else 1
    body = heads * rows * row
  assert (rows - 1) * stride + row <= SPAN < rows * stride + row and rows == (SPAN - row) // stride + 1
  storage = torch.full((GUARD + body + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
  typed = storage[GUARD:GUARD + body].view(_elem(fmt, dtype))
  if kind == "strided":
    view = typed.as_strided((rows, 1, row // es), (stride // es, row // es, 1))
  elif kind == "two_heads":  # head-major: each head's rows span the largest descriptor, and the second head's last row ends at the pool's last byte
    view = typed.view(2, rows, row // es).transpose(0, 1)
    assert view[rows - 1, 1].data_ptr() + row == storage.data_ptr() + GUARD + body
  else:
    view = typed.view(rows, 1, row // es)
  return storage, view, rows, stride


def _encode(fmt, x, dtype):
  from ffpa_attn_amd import pack_latent_rows_ds, quantize_latent_rows

  if fmt == "ds":
    return pack_latent_rows_ds(x)
  return quantize_latent_rows(x, KV_SCALE).view(torch.uint8) if fmt == "fp8" else x.to(dtype)


def _decode(fmt, stored):
  from ffpa_attn_amd import unpack_latent_rows_ds

  if fmt == "ds":
    return unpack_latent_rows_ds(stored).double()
  return stored.view(torch.float8_e4m3fn).double() * KV_SCALE if fmt == "fp8" else stored.double()


def _index_lists(rows, stride, seed):
  """``[T][TOPK]`` ids (Python ints) as the module's docstring lists them, and the same lists with every entry in front of a count clamped into the pool."""
  rng = random.Random(seed)
  last, mid = rows - 1, 2 ** 30 // stride  # (mid: the first row whose offset has bit 30 set is mid + 1 at the latest; mid - 1 lies below it)
  assert (mid + 1) * stride >= 2 ** 30 > (mid - 1) * stride
  anywhere = lambda n: [rng.randrange(rows) for _ in range(n)]
  behind = lambda t, n: [(last, INT_MAX, 2 ** 30, -1)[(t + j) % 4] for j in range(n)]
  edges = [0, 1, last, last - 1, mid - 1, mid, mid + 1]
  lists = [behind(0, TOPK)]
  lists.append(edges + anywhere(COUNTS[1] - len(edges)) + behind(1, TOPK - COUNTS[1]))
  outside = [INT_MAX, INT_MIN, -1, rows]  # in front of the count: clamped to the last row, row 0, row 0, the last row
  body = edges + outside + list(range(rows - 64, rows)) + anywhere(150)
  lists.append(body + anywhere(TOPK - len(body)))
  body = list(range(rows - 64, rows)) + anywhere(150) + [mid + 1, mid, 0, 0, last]  # (duplicates count twice)
  lists.append(anywhere(TOPK - len(body)) + body)
  assert all(len(l) == TOPK for l in lists)
  clamped = [[min(max(i, 0), last) for i in l[:n]] + l[n:] for l, n in zip(lists, COUNTS)]
  return lists, clamped


def _call(hip, fmt, q, pool, indices, counts, num_splits, flags):
  import ffpa_attn_amd as A

  fn = {"16bit": A.ffpa_attn_with_kvcache_mla_sparse, "fp8": A.ffpa_attn_with_kvcache_mla_sparse_fp8, "ds": A.ffpa_attn_with_kvcache_mla_sparse_ds}[fmt]
  kw = dict(kv_scale=KV_SCALE) if fmt == "fp8" else {}
  with _launches(hip, flags) as plans:
    out, lse = fn(q, pool.view(torch.float8_e4m3fn) if fmt == "fp8" else pool, DV, indices, topk_lens=counts, softmax_scale=SCALE, num_splits=num_splits,
                  return_softmax_lse=True, **kw)
  torch.cuda.synchronize()
  assert len(plans) == 1 and plans[0]["kernel"].startswith(KERNEL[fmt]), plans
  return out, lse, plans[0]


@pytest.mark.parametrize("kind", ["dense", "strided", "two_heads"])
@pytest.mark.parametrize("fmt", ["16bit", "fp8", "ds"])
def test_gather_at_the_reach_of_its_offsets(hip, fmt, kind):
  dtype = torch.float16 if (fmt, kind) in (("16bit", "strided"), ("fp8", "two_heads")) else torch.bfloat16
  storage, pool, rows, stride = _pool(fmt, kind, dtype)
  hkv = pool.size(1)
  lists, clamped = _index_lists(rows, stride, seed=len(fmt) * 7 + len(kind))
  used = sorted({i for l, n in zip(clamped, COUNTS) for i in l[:n]})
  assert {0, 1, rows - 1, rows - 2, 2 ** 30 // stride} <= set(used) and (kind == "strided" or (rows - 1) * stride + ROW_BYTES[fmt] >= SPAN - 128)
  assert sum((i * stride) >> 30 == 1 for i in used) >= 100  # offsets with bit 30 set: the upper half of the span
  g = torch.Generator(device="cuda").manual_seed(rows % 1000)
  data = torch.randn((len(used), hkv, D), generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16 if fmt == "ds" else dtype)
  stored = _encode(fmt, data, dtype)
  ids = torch.tensor(used, device="cuda")
  pool[ids] = stored
  q = torch.randn((T, 16, D), generator=g, device="cuda", dtype=torch.float32).to(dtype)
  indices = torch.tensor(lists, dtype=torch.int32, device="cuda")
  counts = torch.tensor(COUNTS, dtype=torch.int32, device="cuda")
  # (1) float64 over the rows gathered per token: the reference never touches the rest of the pool
  cache, ns = gathered(pool, torch.tensor(clamped, device="cuda").clamp(0, rows - 1), COUNTS)
  deq = _decode(fmt, cache)
  o, lse_ref, pmax, p2sum = R.attend(q[:, None], deq, deq, ns, None, False, SCALE)
  ref = (o[..., :DV].contiguous(), lse_ref, pmax, p2sum)
  vstat = R.visible_values(deq[..., :DV], ns, None)
  # (2) the compacted pool: the referenced rows only, shuffled, under the remapped lists
  order = torch.randperm(len(used), generator=torch.Generator().manual_seed(5)).tolist()
  where = {used[src]: dst for dst, src in enumerate(order)}
  compact = stored[torch.tensor(order, device="cuda")].contiguous()
  remapped = torch.tensor([[where[i] for i in l[:n]] + [-1] * (TOPK - n) for l, n in zip(clamped, COUNTS)], dtype=torch.int32, device="cuda")
  for num_splits, flags in ((0, hip.FLAG_KV_STREAM), (3, hip.FLAG_FORCE_SPLITS | hip.FLAG_NO_KV_STREAM)):
    out, lse, plan = _call(hip, fmt, q, pool, indices, counts, num_splits, flags)
    what = f"{fmt} {kind} rows {rows} splits {num_splits} -> {plan}"
    assert out.shape == (T, 16, DV) and lse.shape == (16, T) and (num_splits == 0 or plan["splits"] == num_splits), what
    assert torch.isfinite(out).all() and (out[0] == 0).all() and torch.isneginf(lse[:, 0]).all() and torch.isfinite(lse[:, 1:]).all(), what  # (3)
    ratio = R.check(out[:, None], lse.t()[:, :, None], ref, v=vstat, dtype=dtype, name=what)
    print(f"\nsparse limit: {fmt} {kind} rows {rows} splits {plan['splits']}: worst error / allowance {ratio:.3f}")
    twin, twin_lse, twin_plan = _call(hip, fmt, q, compact, remapped, counts, num_splits, flags)
    assert twin_plan["splits"] == plan["splits"] and twin_plan["kernel"] == plan["kernel"], (plan, twin_plan)
    assert torch.equal(out.view(torch.int16), twin.view(torch.int16)) and torch.equal(lse.view(torch.int32), twin_lse.view(torch.int32)), what
  # (4) the guard bytes around the pool
  assert (storage[:GUARD] == 0xFF).all() and (storage[-GUARD:] == 0xFF).all()
  assert torch.equal(pool[ids], stored)


def test_store_latent_rows_ds_at_the_reach_of_the_pool(hip):
  """(5): the last row and row 2^30 // 656 of the largest dense pool of 656-byte rows — and two slots that write nothing."""
  from ffpa_attn_amd import pack_latent_rows_ds, store_latent_rows_ds

  storage, pool, rows, stride = _pool("ds", "dense", torch.bfloat16)
  before = storage.clone()
  slots = [rows - 1, -1, 2 ** 30 // 656, rows]
  kv = torch.randn((4, 1, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9)).bfloat16()
  store_latent_rows_ds(pool, kv, torch.tensor(slots, dtype=torch.int32, device="cuda"))
  torch.cuda.synchronize()
  want = before.clone()
  packed = pack_latent_rows_ds(kv)
  for i in (0, 2):
    lo = GUARD + slots[i] * 656
    want[lo:lo + 656] = packed[i, 0]
    a, b = max(lo - 2 ** 19, 0), min(lo + 2 ** 19, storage.numel())  # a 1 MiB window around the row
    assert torch.equal(storage[a:b], want[a:b]) and not torch.equal(storage[lo:lo + 656], before[lo:lo + 656])
  assert torch.equal(storage, want)  # ... and nothing else, guards included
  assert int((storage != before).sum()) <= 2 * 656
