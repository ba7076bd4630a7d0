"""``ffpa_attn_varlen_with_kvcache_mla`` on the GPU: ragged query batches over the MLA latent cache — the per-token append (``ffpa_mla_append_varlen_kernel``), the
latent kernel on sequences of different token counts and its compact grid of packed rows — against float64 attention on the gathered latent rows, PER SEQUENCE
(tests/kvcache_ref.py ``attend`` on (pool, pool) with the value columns ``[:512]``; outputs held to ``kvcache_ref.allowance`` through ``check``, LSE to atol 2e-4 /
rtol 2e-5; no new tolerance), and bit for bit against the uniform call.  D = 576, head_dim_v = 512, scale 1 / sqrt(192), pages of 64 keys shuffled in a pool
that holds NaN wherever no sequence holds a key.  Tiles: 64 rows x 32 keys.

Query lengths per batch: (a) one 40-token verification among short ones at 128 heads (compact grid: 106 slots against 480 row tiles), (b) a 64-token chunk among
decodes at 16 / 32 heads (26 against 128), (c) 1 ... 4 tokens (full grid), (d) one sequence of 70 tokens at one head (unpacked).  Cache lengths before the step
cycle through 0, 1, 31, 33, 64, 97, 300."""

import contextlib

import numpy as np
import pytest
import torch

import kvcache_ref as R
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D, DV, PAGE = 576, 512, 64
SCALE = 192 ** -0.5
NAN = float("nan")
CACHE_LENS = [0, 1, 31, 33, 64, 97, 300]
BATCHES = {"a": [1, 0, 3, 5, 1, 40], "b": [1, 0, 1, 1, 1, 1, 1, 64], "c": [1, 2, 3, 4], "d": [70]}
RUNS = [("a", 128, 1), ("b", 16, 1), ("b", 32, 2), ("c", 16, 1), ("c", 128, 1), ("d", 1, 1)]
COMPACT = {("a", 128): 106, ("b", 16): 26, ("b", 32): 26}  # slots per latent head where the plan takes the compact grid


@contextlib.contextmanager
def _launches(hip, flags=0):
  """Every MLA launch inside the block carries ``flags`` too, and its plan (``plan_out``) is appended to the list the block receives."""
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


_CASES: dict = {}


def _cu(qlens, device="cuda"):
  return torch.tensor(np.concatenate(([0], np.cumsum(qlens))), dtype=torch.int32, device=device)


def _case(qlens, hq, hkv, dtype, seed=0, cache=None, pad=0, room=0, contiguous=0, pages=0):
  """A ragged step, made once per shape and shared (nothing writes to it: every call runs on a clone of the storage): q and the new latent rows ``kv`` (``pad``
  rows of NaN behind the batch's last token), the latent pool (a view of a storage that holds NaN in every row no sequence holds), the shuffled block table, and
  the cache lengths BEFORE the step (``cache``, default: CACHE_LENS cycled; ``pages``: pages per sequence, default: what the step needs + ``room`` keys)."""
  key = (tuple(qlens), hq, hkv, dtype, seed, None if cache is None else tuple(cache), pad, room, contiguous, pages)
  if key in _CASES:
    return _CASES[key]
  g = torch.Generator(device="cuda").manual_seed(2000 + seed)
  tdt = R.TORCH_DTYPE[dtype]
  B, T = len(qlens), sum(qlens)
  cache = [CACHE_LENS[(3 * b + seed) % len(CACHE_LENS)] for b in range(B)] if cache is None else list(cache)
  q = torch.randn((T + pad, hq, D), generator=g, device="cuda", dtype=tdt)
  kv = torch.randn((T + pad, hkv, D), generator=g, device="cuda", dtype=tdt)
  kv[T:] = NAN
  held = [min(max(c, 0), (contiguous or pages * PAGE) or c) for c in cache]  # (keys a sequence holds before the step: its length, inside the capacity)
  if contiguous:
    n_pages, page, table, ids = B, contiguous, None, None
  else:
    pps = pages or -(-(max(h + n for h, n in zip(held, qlens)) + room + 1) // PAGE)
    n_pages, page = B * pps + 3, PAGE
    ids = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))[: B * pps].to(torch.int32).view(B, pps)
    table = ids.cuda()
  kc = torch.randn((n_pages, page, hkv, D), generator=g, device="cuda", dtype=tdt)
  seen = torch.zeros((n_pages, page), dtype=torch.bool)
  for b, n in enumerate(held):
    for j in range(n):
      seen[(int(ids[b, j // PAGE]), j % PAGE) if ids is not None else (b, j)] = True
  kc[~seen.cuda()] = NAN
  pool, _, storage, _ = R.lay_out_cache(kc, kc, "batch_padded", fill=NAN) if not contiguous else (kc, None, kc, None)
  t = dict(q=q, kv=kv, pool=pool, storage=storage, table=table, ids=ids, qlens=list(qlens), cache_list=cache, dtype=dtype, heads=(hq, hkv), T=T,
           cache=torch.tensor(cache, dtype=torch.int32, device="cuda"), cu=_cu(qlens), max_q=max(max(qlens), 1), capacity=R.capacity_of(pool, table), refs={})
  _CASES[key] = t
  return t


def _write_rows(t, pool, qlens=None, cache=None, kv=None, table="case"):
  """The append, written with torch IN PLACE on ``pool`` (a re-view of a cloned storage) -> the lengths after it."""
  qlens = t["qlens"] if qlens is None else qlens
  cache = t["cache_list"] if cache is None else cache
  kv = t["kv"] if kv is None else kv
  ids = t["ids"] if isinstance(table, str) else table
  cap, page, used, row = t["capacity"], pool.size(1), [], 0
  for b, n in enumerate(qlens):
    base = max(int(cache[b]), 0)
    used.append(min(base + n, cap))
    for i in range(n):
      pos = base + i
      if pos < cap:
        slab = (b, pos) if ids is None else (min(max(int(ids[b, pos // page]), 0), pool.size(0) - 1), pos % page)
        pool[slab] = kv[row + i]
    row += n
  return used


def _reference(t, causal, with_kv):
  """Per sequence with a token: float64 ``attend`` of its rows over ITS keys (after the torch-written append when ``with_kv``) -> ``{b: (ref, vstat)}``, the
  reference pool and the lengths.  Made once per (case, causal, with_kv)."""
  key = (causal, with_kv)
  if key in t["refs"]:
    return t["refs"][key]
  want_storage = t["storage"].clone()
  want_pool = R.reviewed(t["pool"], t["storage"], want_storage)
  lens = _write_rows(t, want_pool) if with_kv else [min(max(c, 0), t["capacity"]) for c in t["cache_list"]]
  per_seq, row = {}, 0
  for b, n in enumerate(t["qlens"]):
    if n:
      tb = None if t["table"] is None else t["table"][b:b + 1]
      pb = want_pool if tb is not None else want_pool[b:b + 1]
      o, lse, pmax, p2sum = R.attend(t["q"][row:row + n][None], pb, pb, [lens[b]], tb, causal, SCALE)
      per_seq[b] = ((o[..., :DV].contiguous(), lse, pmax, p2sum), R.visible_values(pb[..., :DV], [lens[b]], tb))
    row += n
  t["refs"][key] = (per_seq, want_pool, want_storage, lens)
  return t["refs"][key]


def _run(hip, t, causal, with_kv, *, num_splits=0, flags=0, pool=None, cu=None, cache=None, kv="case", table="case", max_q=None):
  """The call on a clone of the case's storage (or on ``pool``) -> (out, lse, plan, the storage it wrote)."""
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache_mla

  storage = None
  if pool is None:
    storage = t["storage"].clone()
    pool = R.reviewed(t["pool"], t["storage"], storage)
  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_varlen_with_kvcache_mla(t["q"], pool, DV, t["cu"] if cu is None else cu, t["max_q"] if max_q is None else max_q,
                                                 t["cache"] if cache is None else cache, t["table"] if isinstance(table, str) else table,
                                                 kv=(t["kv"] if isinstance(kv, str) else kv) if with_kv else None, softmax_scale=SCALE, causal=causal,
                                                 num_splits=num_splits, return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"ffpa_fwd_m16_mla_kernel<{t['dtype']}, 576, dv=512"), plans
  assert out.shape == (t["q"].size(0), t["heads"][0], DV) and lse.shape == (t["heads"][0], t["q"].size(0)) and lse.dtype == torch.float32
  return out, lse, plans[0], storage


def _check(t, out, lse, causal, with_kv, what):
  per_seq, _, _, lens = _reference(t, causal, with_kv)
  row, worst = 0, 0.0
  for b, n in enumerate(t["qlens"]):
    if n:
      ref, vstat = per_seq[b]
      name = f"{what}: {t['dtype']} heads {t['heads']} causal={causal} kv={with_kv} sequence {b}: {n} tokens over {lens[b]} keys"
      worst = max(worst, R.check(out[row:row + n][None], lse[:, row:row + n][None], ref, v=vstat, dtype=t["dtype"], name=name))
    row += n
  print(f"[mla varlen] {worst:.3f} {what}: {t['dtype']} heads {t['heads']} causal={causal} kv={with_kv} qlens {t['qlens']} cache {t['cache_list']}")


def _plan_is(plan, t, name, splits=None):
  hq, hkv = t["heads"]
  group, B = hq // hkv, len(t["qlens"])
  nqt = -(-group * t["max_q"] // 64) if group > 1 else -(-t["max_q"] // 64)
  slots = COMPACT.get((name, hq), 0)
  assert plan["block_rows"] == 64 and plan["block_keys"] == 32 and plan["row_tiles"] == nqt, plan
  assert plan["compact_slots"] == slots and ("compact" in plan["kernel"]) == (slots > 0), plan
  assert plan["workgroups"] == (slots if slots else B * nqt) * hkv * plan["splits"], plan
  assert ("packed into rows" in plan["kernel"]) == (group > 1), plan
  if splits is not None:
    assert plan["splits"] == splits, plan


# ----------------------------------------------------------------------------- the ragged batches against float64
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name, hq, hkv", RUNS)
def test_ragged_batches_against_float64(hip, dtype, name, hq, hkv):
  """Causal and not, with the step's rows appended (``kv=``) and over the cache as it is — without ``kv`` the sequences whose cache is shorter than their
  tokens have rows that see no key (O = 0, LSE = -inf).  The plan is the pure rule's: compact on (a) and (b), the full grid on (c) and (d)."""
  t = _case(BATCHES[name], hq, hkv, dtype, seed=hq + len(name))
  for causal in (False, True):
    for with_kv in (True, False):
      out, lse, plan, storage = _run(hip, t, causal, with_kv)
      _plan_is(plan, t, name)
      _check(t, out, lse, causal, with_kv, f"batch ({name})")
      if not with_kv:
        assert torch.equal(storage.view(torch.int16), t["storage"].view(torch.int16))  # (nothing is written without kv=)


# ----------------------------------------------------------------------------- bit identity with the uniform call
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name, hq, hkv", RUNS)
def test_each_sequence_has_the_bits_of_the_uniform_call_on_it_alone(hip, dtype, name, hq, hkv):
  """``num_splits = 1``: the rows of sequence b are ``ffpa_attn_with_kvcache_mla`` on that sequence alone (Sq = Sq_b, its row of the table, its length after the
  append) — the same chunks of the same rows over the same tiles, whatever the grid: O and LSE bit for bit."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  t = _case(BATCHES[name], hq, hkv, dtype, seed=hq + len(name))
  for causal in (True, False):
    out, lse, plan, storage = _run(hip, t, causal, True, num_splits=1)
    _plan_is(plan, t, name, splits=1)
    _, want_pool, _, lens = _reference(t, causal, True)
    row = 0
    for b, n in enumerate(t["qlens"]):
      if n:
        one, one_lse = ffpa_attn_with_kvcache_mla(t["q"][row:row + n][None], want_pool, DV, cache_seqlens=torch.tensor([lens[b]], dtype=torch.int32, device="cuda"),
                                                  block_table=t["table"][b:b + 1], softmax_scale=SCALE, causal=causal, num_splits=1, return_softmax_lse=True)
        assert torch.equal(out[row:row + n], one[0]), f"O of sequence {b} ({n} tokens over {lens[b]} keys, causal={causal})"
        assert torch.equal(lse[:, row:row + n], one_lse[0]), f"LSE of sequence {b} ({n} tokens over {lens[b]} keys, causal={causal})"
      row += n


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", [(16, 1, 1), (16, 1, 3), (128, 1, 3), (32, 2, 4)])
def test_uniform_cu_seqlens_give_the_uniform_call(hip, dtype, hq, hkv, sq):
  """Every sequence with ``sq`` tokens: the ragged call — its append and its attention launch — returns the bits of ``ffpa_attn_with_kvcache_mla`` and writes the
  same storage; the plan is the uniform call's (never compact)."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  t = _case([sq] * 5, hq, hkv, dtype, seed=7 + sq, cache=[0, 31, 63, 64, 300])
  for causal in (True, False):
    out, lse, plan, storage = _run(hip, t, causal, True)
    assert plan["compact_slots"] == 0 and "compact" not in plan["kernel"], plan
    want_storage = t["storage"].clone()
    with _launches(hip) as plans:
      want, want_lse = ffpa_attn_with_kvcache_mla(t["q"].view(5, sq, hq, D), R.reviewed(t["pool"], t["storage"], want_storage), DV, kv=t["kv"].view(5, sq, hkv, D),
                                                  cache_seqlens=t["cache"], block_table=t["table"], softmax_scale=SCALE, causal=causal, return_softmax_lse=True)
    assert {k: plan[k] for k in ("row_tiles", "workgroups", "splits", "kernel")} == {k: plans[0][k] for k in ("row_tiles", "workgroups", "splits", "kernel")}
    assert torch.equal(out.view(5, sq, hq, DV), want) and torch.equal(lse.view(hq, 5, sq).permute(1, 0, 2), want_lse)
    assert torch.equal(storage.view(torch.int16), want_storage.view(torch.int16))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name, hq, hkv", [r for r in RUNS if (r[0], r[1]) in COMPACT])
def test_the_full_grid_returns_the_compact_launch_s_bits(hip, dtype, name, hq, hkv):
  t = _case(BATCHES[name], hq, hkv, dtype, seed=hq + len(name))
  for causal in (True, False):
    for ns in (0, 1):
      out, lse, plan, _ = _run(hip, t, causal, True, num_splits=ns)
      full, full_lse, full_plan, _ = _run(hip, t, causal, True, num_splits=plan["splits"], flags=hip.FLAG_NO_COMPACT_GRID | (hip.FLAG_FORCE_SPLITS if plan["splits"] > 1 else 0))
      assert plan["compact_slots"] == COMPACT[(name, hq)] and full_plan["compact_slots"] == 0 and full_plan["splits"] == plan["splits"], (plan, full_plan)
      assert full_plan["workgroups"] == len(t["qlens"]) * plan["row_tiles"] * hkv * plan["splits"] > plan["workgroups"], (plan, full_plan)
      assert torch.equal(out[: t["T"]], full[: t["T"]]) and torch.equal(lse[:, : t["T"]], full_lse[:, : t["T"]]), (causal, plan, full_plan)


# ----------------------------------------------------------------------------- KV ranges
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_forced_kv_ranges_on_the_compact_grid(hip, dtype):
  """2, 3 and 5 KV ranges forced on (a): every sequence shares out ITS tiles (1 ... 11 of 32 keys, so some ranges are empty), on the compact grid x ranges.
  Splits only change the merge's rounding: each agrees with float64."""
  t = _case(BATCHES["a"], 128, 1, dtype, seed=129)
  for causal in (True, False):
    for ns in (2, 3, 5):
      out, lse, plan, _ = _run(hip, t, causal, True, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS)
      _plan_is(plan, t, "a", splits=ns)
      assert "ffpa_varlen_merge_kernel" in plan["kernel"]
      _check(t, out, lse, causal, True, f"{ns} KV ranges")


# ----------------------------------------------------------------------------- the append
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name, hq, hkv", [("a", 128, 1), ("b", 32, 2), ("c", 16, 1)])
def test_append_writes_each_latent_row_once_and_nothing_else(hip, dtype, name, hq, hkv):
  """The cache's storage after the step — the NaN of every row no sequence holds included — is the integers of a storage written with torch: exactly the step's
  rows changed; ``cache_seqlens`` is not advanced; attending over the written cache without ``kv=`` gives the same bits."""
  t = _case(BATCHES[name], hq, hkv, dtype, seed=hq + len(name))
  _, _, want_storage, lens = _reference(t, True, True)
  before = t["cache"].clone()
  out, lse, plan, storage = _run(hip, t, True, True)
  assert torch.equal(t["cache"], before)
  assert torch.equal(storage.view(torch.int16), want_storage.view(torch.int16)), "the cache's storage differs from the torch-written reference"
  touched = (want_storage.view(torch.int16) != t["storage"].view(torch.int16)).any(dim=-1).sum().item()
  assert touched == t["T"] * hkv  # (NaN rows became data: exactly the appended rows changed)
  again = _run(hip, t, True, False, pool=R.reviewed(t["pool"], t["storage"], storage), cache=torch.tensor(lens, dtype=torch.int32, device="cuda"))
  assert torch.equal(out, again[0]) and torch.equal(lse, again[1])


def test_used_lengths_padding_rows_capacity_and_negative_lengths(hip):
  """``used`` for every sequence, empty ones included and with fewer token rows than sequences; rows behind ``cu_seqlens_q[B]`` (they hold NaN) write nothing;
  positions at or past the capacity are dropped and ``used`` stops there; negative ``cache_seqlens`` act as 0."""
  qlens = [0, 2, 0, 0, 5, 0, 1, 0, 0]
  pps, cap = 2, 128
  cache = [5, 127, -3, 128, 125, 200, -1, 0, 64]
  t = _case(qlens, 16, 1, "bf16", seed=3, cache=cache, pad=3, pages=pps)
  assert t["capacity"] == cap and t["table"].size(1) == pps and t["q"].size(0) == 11
  lens_t = torch.tensor(cache, dtype=torch.int32, device="cuda")
  storage, want_storage = t["storage"].clone(), t["storage"].clone()
  pool, want_pool = R.reviewed(t["pool"], t["storage"], storage), R.reviewed(t["pool"], t["storage"], want_storage)
  want_used = _write_rows(t, want_pool, cache=cache)
  assert want_used == [5, 128, 0, 128, 128, 128, 1, 0, 64]
  used = hip.mla_append_varlen(pool, t["kv"], t["cu"], lens_t, t["table"])
  assert used.dtype == torch.int32 and used.tolist() == want_used
  assert torch.equal(storage.view(torch.int16), want_storage.view(torch.int16))
  written = (want_storage.view(torch.int16) != t["storage"].view(torch.int16)).any(dim=-1).sum().item()
  assert written == 1 + 3 + 1  # (127: one of two rows fits; 125: three of five; -1 -> row 0; the three padding rows: none)
  assert torch.equal(lens_t, torch.tensor(cache, dtype=torch.int32, device="cuda"))
  # no token row at all, and more sequences than a workgroup has lanes: used[] still covers the batch
  B = 300
  cu0 = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
  lens0 = torch.arange(-10, B - 10, dtype=torch.int32, device="cuda")
  table0 = torch.zeros((B, pps), dtype=torch.int32, device="cuda")
  snapshot = storage.clone()
  used0 = hip.mla_append_varlen(pool, t["kv"][:0], cu0, lens0, table0)
  assert torch.equal(used0, lens0.clamp(0, cap)) and torch.equal(storage.view(torch.int16), snapshot.view(torch.int16))
  # ... and through the entry point: the whole step with padding rows, against float64 on the torch-written cache
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache_mla

  storage2 = t["storage"].clone()
  out, lse = ffpa_attn_varlen_with_kvcache_mla(t["q"], R.reviewed(t["pool"], t["storage"], storage2), DV, t["cu"], 5, lens_t, t["table"], kv=t["kv"],
                                               softmax_scale=SCALE, causal=True, return_softmax_lse=True)
  assert torch.equal(storage2.view(torch.int16), want_storage.view(torch.int16))
  row = 0
  for b, n in enumerate(qlens):
    if n:
      ref = R.attend(t["q"][row:row + n][None], want_pool, want_pool, [want_used[b]], t["table"][b:b + 1], True, SCALE)
      ref = (ref[0][..., :DV].contiguous(),) + tuple(ref[1:])
      R.check(out[row:row + n][None], lse[:, row:row + n][None], ref, v=R.visible_values(want_pool[..., :DV], [want_used[b]], t["table"][b:b + 1]), dtype="bf16",
              name=f"sequence {b} at the capacity")
    row += n


# ----------------------------------------------------------------------------- the placement rule of both 16-bit appends at its edges, in ONE call
EDGE_STEPS = [((-1, 0, 126), (3, 0, 3)), ((-1, 0, 62, 126), (3, 0, 3, 3))]  # (lengths before the step, token rows of the ragged step; a uniform step brings 3 each)


def _edge_pool(B, hkv, dtype, seed):
  """A pool of 2 B + 2 pages of 64 rows of random values and a table of 2 shuffled pages per sequence (capacity 128)."""
  g = torch.Generator(device="cuda").manual_seed(seed)
  pool = torch.randn((2 * B + 2, PAGE, hkv, D), device="cuda", generator=g).to(dtype)
  table = torch.randperm(2 * B + 2, device="cuda", generator=g)[:2 * B].to(torch.int32).view(B, 2)
  return pool, table, g


def _placed(pool, table, lens, counts, rows):
  """The torch statement of the latent appends' rule: row i of sequence b goes to position max(lens[b], 0) + i of its pages, dropped at or past the capacity
  -> (the pool after the step, used = min(max(lens, 0) + counts, capacity))."""
  want, ids, cap, used, r = pool.clone(), table.tolist(), table.size(1) * PAGE, [], 0
  for b, (n, c) in enumerate(zip(lens, counts)):
    base = max(n, 0)
    used.append(min(base + c, cap))
    for pos in range(base, min(base + c, cap)):
      want[ids[b][pos // PAGE], pos % PAGE] = rows[r + pos - base]
    r += c
  return want, used


@pytest.mark.parametrize("hkv", [1, 2])
@pytest.mark.parametrize("lens, counts", EDGE_STEPS)
@pytest.mark.parametrize("kernel", ["uniform", "ragged"])
def test_both_appends_place_rows_by_one_rule_at_its_edges(hip, kernel, lens, counts, hkv):
  """One call of ``ffpa_mla_append_kernel`` (3 new rows per sequence) and of ``ffpa_mla_append_varlen_kernel`` (3, 0, 3 rows) at lengths -1 (acts as 0), 0 and
  126 of 128 (the third row is past the capacity) — and, with a fourth sequence, 62 (the rows cross into the next page): the raw pool is the torch-written one,
  ``used[]`` is written for every sequence, the one without a token included, and ``cache_seqlens`` is left alone."""
  B = len(lens)
  counts = (3,) * B if kernel == "uniform" else counts
  pool, table, g = _edge_pool(B, hkv, torch.bfloat16, 11 * hkv + B)
  rows = torch.randn((sum(counts), hkv, D), device="cuda", generator=g).to(torch.bfloat16)
  want, want_used = _placed(pool, table, lens, counts, rows)
  lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
  got = pool.clone()
  if kernel == "uniform":
    q = torch.randn((3 * B, 16, D), device="cuda", generator=g).to(torch.bfloat16)
    used = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.ops.ffpa_attn._mla_fwd_hip(q, got, DV, _cu(counts), used, table, rows.view(B, 3, hkv, D), lens_t, 3, 2 * PAGE, SCALE, 1, 0)
  else:
    used = torch.ops.ffpa_attn._mla_append_varlen_hip(got, rows, _cu(counts), lens_t, table)
  assert used.tolist() == want_used
  assert torch.equal(got.view(torch.int16), want.view(torch.int16)), "the raw pool differs from the torch-written one"
  assert lens_t.tolist() == list(lens)


# ----------------------------------------------------------------------------- the contiguous cache
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_a_contiguous_cache_runs_as_one_page_per_sequence(hip, dtype):
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache_mla

  t = _case(BATCHES["c"], 16, 1, dtype, seed=11, cache=[0, 33, 97, 124], contiguous=128)
  assert t["table"] is None and t["pool"].shape == (4, 128, 1, D)
  for with_kv in (True, False):
    out, lse, plan, storage = _run(hip, t, True, with_kv)
    _check(t, out, lse, True, with_kv, "contiguous")
    if with_kv:
      assert torch.equal(storage.view(torch.int16), _reference(t, True, True)[2].view(torch.int16))
  with pytest.raises(ValueError, match="multiple of 64"):
    ffpa_attn_varlen_with_kvcache_mla(t["q"], t["pool"][:, :100], DV, t["cu"], 4, t["cache"], softmax_scale=SCALE)


# ----------------------------------------------------------------------------- graph capture
def test_one_graph_follows_the_step_s_tensors_written_in_place(hip):
  """Append + attention (+ merge, if the plan splits) of (a) captured once; replays after cache_seqlens, cu_seqlens_q (same T, same bound), block_table and kv
  were rewritten in place: each equals the eager call on the same state bit for bit, outputs and storage."""
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache_mla

  t = _case(BATCHES["a"], 128, 1, "bf16", seed=129, room=64)
  storage = t["storage"].clone()
  pool = R.reviewed(t["pool"], t["storage"], storage)
  pool.nan_to_num_(nan=0.25)  # (replays move lengths and pages around: every row must hold a number)
  lens, cu, table, kv = t["cache"].clone(), t["cu"].clone(), t["table"].clone(), t["kv"].clone()
  call = lambda p: ffpa_attn_varlen_with_kvcache_mla(t["q"], p, DV, cu, 40, lens, table, kv=kv, softmax_scale=SCALE, causal=True, return_softmax_lse=True)
  call(pool.clone())  # (warm: the library is loaded, the scratch is sized)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out_g, lse_g = call(pool)
  states = [(t["cache_list"], t["qlens"], table.clone(), kv.clone()),
            ([33, 0, 300, 64, 1, 97], [5, 1, 0, 3, 40, 1], table.flip(0).contiguous(), torch.randn_like(kv)),
            ([64, 31, 0, 1, 200, 33], [10, 10, 10, 10, 5, 5], table.roll(1, 0).contiguous(), torch.randn_like(kv))]
  for n, ql, tb, rows in states:
    assert sum(ql) == t["T"] and max(ql) <= 40
    lens.copy_(torch.tensor(n, dtype=torch.int32, device="cuda"))
    cu.copy_(_cu(ql))
    table.copy_(tb)
    kv.copy_(rows)
    snapshot = storage.clone()
    graph.replay()
    torch.cuda.synchronize()
    after = storage.clone()
    storage.copy_(snapshot)
    eager = call(pool)
    torch.cuda.synchronize()
    assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1]), (n, ql)
    assert torch.equal(after.view(torch.int16), storage.view(torch.int16)), (n, ql)
    want_storage = snapshot.clone()
    used = _write_rows(t, R.reviewed(t["pool"], t["storage"], want_storage), qlens=ql, cache=n, kv=kv, table=tb.cpu())
    assert torch.equal(after.view(torch.int16), want_storage.view(torch.int16)), (n, ql)
    row = 0
    for b, m in enumerate(ql):
      if m:
        ref = R.attend(t["q"][row:row + m][None], pool, pool, [used[b]], table[b:b + 1], True, SCALE)
        ref = (ref[0][..., :DV].contiguous(),) + tuple(ref[1:])
        R.check(out_g[row:row + m][None], lse_g[:, row:row + m][None], ref, v=R.visible_values(pool[..., :DV], [used[b]], table[b:b + 1]), dtype="bf16",
                name=f"graph replay at {n} / {ql}, sequence {b}")
      row += m
