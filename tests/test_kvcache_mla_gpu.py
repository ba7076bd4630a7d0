"""``ffpa_attn_with_kvcache_mla`` on the GPU: the MLA latent-cache kernel — ONE LDS image per latent tile, the two images of the tile alternating by the tile's
parity — against float64 attention on the gathered latent rows (tests/kvcache_ref.py ``gather`` / ``attend`` on (kv, kv), value columns ``[:head_dim_v]``; outputs
held to ``kvcache_ref.allowance`` through ``check``, LSE to atol 2e-4 / rtol 2e-5; no new tolerance).  D = 576, head_dim_v = 512, scale 1 / sqrt(192), pages of
64 keys shuffled in a pool that holds NaN wherever no visible key lives.  Tiles: 64 rows x 32 keys, so the key lengths 0 ... 97 and 300 cover the empty sequence,
the zero-filled tail row and odd and even tile counts (the image toggle), and forced KV ranges start at odd tiles."""

import contextlib
import math

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
NAN = float("nan")


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


def _case(lens, hq, hkv, sq, dtype, seed=0, room=0, contiguous=0):
  """q, the latent pool (a view of a storage with two NaN pages more; NaN in every row no sequence holds), the shuffled block table, the lengths and the float64
  reference for both causal flags: made once per shape and shared (nothing writes to it: the append tests clone the storage)."""
  key = (tuple(lens), hq, hkv, sq, dtype, seed, room, contiguous)
  if key in _CASES:
    return _CASES[key]
  g = torch.Generator(device="cuda").manual_seed(1000 + seed)
  tdt = R.TORCH_DTYPE[dtype]
  B = len(lens)
  q = torch.randn((B, sq, hq, D), generator=g, device="cuda", dtype=tdt)
  if contiguous:
    n_pages, page, table = B, contiguous, None
    owner = lambda b, j: (b, j)
  else:
    pps = -(-(max(max(lens), 1) + room) // PAGE) + 1
    n_pages, page = B * pps + 3, PAGE
    ids = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))[: B * pps].to(torch.int32).view(B, pps)
    table = ids.cuda()
    owner = lambda b, j: (int(ids[b, j // PAGE]), j % PAGE)
  kc = torch.randn((n_pages, page, hkv, D), generator=g, device="cuda", dtype=tdt)
  seen = torch.zeros((n_pages, page), dtype=torch.bool)
  for b, n in enumerate(lens):
    for j in range(n):
      seen[owner(b, j)] = True
  kc[~seen.cuda()] = NAN
  pool, _, storage, _ = R.lay_out_cache(kc, kc, "batch_padded", fill=NAN) if not contiguous else (kc, None, kc, None)
  t = dict(q=q, pool=pool, storage=storage, table=table, lens=torch.tensor(lens, dtype=torch.int32, device="cuda"), lens_list=list(lens), dtype=dtype, sq=sq,
           heads=(hq, hkv))
  t["vstat"] = R.visible_values(pool[..., :DV], lens, table)
  _CASES[key] = t
  return t


def _ref(t, causal, lens=None, pool=None):
  """float64 attention on the gathered latent rows with v = k[..., :DV] (``attend`` on (kv, kv): the value columns are the first DV of its output)."""
  pool = t["pool"] if pool is None else pool
  o, lse, pmax, p2sum = R.attend(t["q"], pool, pool, t["lens_list"] if lens is None else lens, t["table"], causal, SCALE)
  return o[..., :DV].contiguous(), lse, pmax, p2sum


def _mla(hip, t, causal=False, *, num_splits=0, flags=0, lens=None, kv=None, pool=None, q=None, table="case"):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla(t["q"] if q is None else q, t["pool"] if pool is None else pool, DV, kv=kv, cache_seqlens=t["lens"] if lens is None else lens,
                                          block_table=t["table"] if table == "case" else table, softmax_scale=SCALE, causal=causal, num_splits=num_splits,
                                          return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"ffpa_fwd_m16_mla_kernel<{t['dtype']}, 576, dv=512"), plans
  return out, lse, plans[0]


def _check(hip, t, causal, what, **kw):
  ref = _ref(t, causal)
  out, lse, plan = _mla(hip, t, causal, **kw)
  name = f"{what}: {t['dtype']} heads {t['heads']} Sq {t['sq']} causal={causal} lens {t['lens_list']} {kw} -> {plan}"
  assert out.shape == (len(t["lens_list"]), t["sq"], t["heads"][0], DV)
  ratio = R.check(out, lse, ref, v=t["vstat"], dtype=t["dtype"], name=name)
  print(f"[mla] {ratio:.3f} {name}")
  return out, lse, plan, ref


# ----------------------------------------------------------------------------- key lengths x heads x tokens
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv", HEADS)
@pytest.mark.parametrize("sq", [1, 3])
def test_key_lengths_heads_and_tokens(hip, dtype, hq, hkv, sq):
  """The ten lengths as ONE batch (Sq = 3: causal — the last three keys are the queries' own, so lengths 0 and 1 leave empty rows), then 33 and 97 one length per
  call.  The group's heads x tokens are the rows of ceil(group x Sq / 64) chunks: 128 heads x 3 tokens span six, and a chunk boundary falls inside a head."""
  causal = sq > 1
  t = _case(LENS, hq, hkv, sq, dtype, seed=hq + sq)
  out, lse, plan, ref = _check(hip, t, causal, "batch")
  group = hq // hkv
  assert plan["block_rows"] == 64 and plan["block_keys"] == 32
  assert plan["row_tiles"] == (math.ceil(group * sq / 64) if group > 1 else 1), plan
  assert plan["workgroups"] == len(LENS) * hkv * plan["row_tiles"] * plan["splits"], plan
  assert ("packed into rows" in plan["kernel"]) == (group > 1) and ("chunked" in plan["kernel"]) == (group * sq > 64 and group > 1), plan
  assert (out[0] == 0).all() and torch.isneginf(lse[0]).all()
  for i, n in ((4, 33), (8, 97)):
    one = dict(t, q=t["q"][i:i + 1], table=t["table"][i:i + 1], lens=t["lens"][i:i + 1], lens_list=[n])
    o1, l1, p1, _ = _check(hip, one, causal, "one length per call", num_splits=1)


# ----------------------------------------------------------------------------- KV ranges
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", [(16, 1, 1), (128, 1, 3), (32, 2, 3)])
def test_forced_kv_ranges_start_at_odd_tiles(hip, dtype, hq, hkv, sq):
  """num_splits 1, 2, 3 and 5 forced on the batch: every sequence shares out ITS tiles (1 ... 10 of 32 keys), so ranges start at odd tiles — the image parity
  must follow the tile index in the prologue, the loop and the page lookahead — and with five ranges over two or three tiles some ranges are empty (weight 0 in
  the merge).  Every count agrees with float64 and with the unsplit launch to the merge's rounding (two allowances); num_splits = 0 is one of them, bit for bit."""
  causal = sq > 1
  t = _case(LENS, hq, hkv, sq, dtype, seed=hq + sq)
  outs = {}
  for ns in (1, 2, 3, 5):
    out, lse, plan, ref = _check(hip, t, causal, "KV ranges", num_splits=ns, flags=hip.FLAG_FORCE_SPLITS)
    assert plan["splits"] == ns, plan
    assert ("ffpa_varlen_merge_kernel" in plan["kernel"]) == (ns > 1)
    outs[ns] = (out, lse)
  o_ref, lse_ref, pmax, p2sum = (x.cpu().numpy() for x in ref)
  stat = lambda x: np.transpose(x, (0, 2, 1))
  half_ulp, flip = R.allowance(o_ref, stat(pmax), stat(p2sum), t["vstat"], dtype, noise=True)
  for ns in (2, 3, 5):
    err = (outs[ns][0].double() - outs[1][0].double()).abs().cpu().numpy()
    assert (err <= 2 * (half_ulp + flip)).all(), f"num_splits {ns} vs 1: {err.max():.3e}"
    torch.testing.assert_close(outs[ns][1], outs[1][1], atol=2 * R.LSE_ATOL, rtol=2 * R.LSE_RTOL)
  out0, lse0, plan0, _ = _check(hip, t, causal, "library's own count")
  same = [ns for ns in outs if torch.equal(out0, outs[ns][0]) and torch.equal(lse0, outs[ns][1])]
  forced = None
  if not same:  # (the heuristic's own count, forced)
    forced = _mla(hip, t, causal, num_splits=plan0["splits"], flags=hip.FLAG_FORCE_SPLITS)
    same = [plan0["splits"]] if torch.equal(out0, forced[0]) and torch.equal(lse0, forced[1]) else []
  assert same, (plan0, forced[2] if forced else None)


# ----------------------------------------------------------------------------- the same arithmetic as the aliased call
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("sq", [1, 3])
def test_same_arithmetic_as_the_two_cache_call_on_the_aliased_pool(hip, dtype, sq):
  """``ffpa_attn_with_kvcache(q, kv, kv)[..., :512]`` packs the 16 heads x Sq tokens into the rows of one tile as this call does, reads the same K fragments,
  makes the same P^T and multiplies the same V^T values in the same order: bf16 O and the LSE are the same bits; fp16 O to rounding (one output ulp)."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  causal = sq > 1
  t = _case(LENS, 16, 1, sq, dtype, seed=16 + sq)
  out, lse, plan = _mla(hip, t, causal, num_splits=1)
  want, want_lse = ffpa_attn_with_kvcache(t["q"], t["pool"], t["pool"], cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE, causal=causal,
                                          num_splits=1, return_softmax_lse=True)
  want = want[..., :DV]
  assert torch.equal(lse, want_lse)
  if dtype == "bf16":
    assert torch.equal(out, want), f"{int((out != want).sum())} elements differ, max {(out.float() - want.float()).abs().max().item():.3e}"
  else:
    ulp = R.ulp_of(want.double(), dtype)
    assert ((out.double() - want.double()).abs() <= ulp).all()


# ----------------------------------------------------------------------------- the contiguous cache
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_a_contiguous_cache_runs_as_one_page_per_sequence(hip, dtype):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  t = _case([1, 97, 128], 16, 1, 1, dtype, seed=5, contiguous=128)
  assert t["table"] is None and t["pool"].shape == (3, 128, 1, D)
  _check(hip, t, False, "contiguous")
  t3 = _case([1, 97, 128], 16, 1, 3, dtype, seed=6, contiguous=128)
  _check(hip, t3, True, "contiguous, three tokens")
  with pytest.raises(ValueError, match="multiple of 64"):
    ffpa_attn_with_kvcache_mla(t["q"], t["pool"][:, :100], DV, cache_seqlens=t["lens"], softmax_scale=SCALE)


# ----------------------------------------------------------------------------- the append
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("snew", [1, 3])
@pytest.mark.parametrize("paged", [True, False])
def test_append_writes_each_latent_row_once_and_nothing_else(hip, dtype, snew, paged):
  """``kv=`` at lengths 0, 31 and 63 ... 65 (crossing a page) equals writing the rows with torch and then attending; the storage — NaNs included — is the same
  integers as the reference's everywhere."""
  lens = [0, 31, 63, 64, 65]
  t = _case(lens, 16, 1, snew, dtype, seed=40 + snew, room=4, contiguous=0 if paged else 128)
  g = torch.Generator(device="cuda").manual_seed(77 + snew)
  kv = torch.randn((len(lens), snew, 1, D), generator=g, device="cuda", dtype=R.TORCH_DTYPE[dtype])
  got_storage, want_storage = t["storage"].clone(), t["storage"].clone()
  got_pool, want_pool = R.reviewed(t["pool"], t["storage"], got_storage), R.reviewed(t["pool"], t["storage"], want_storage)
  _, used, _ = R.append(want_pool, want_pool, kv, kv, lens, t["table"])
  assert used == [n + snew for n in lens]
  before = t["lens"].clone()
  out, lse, plan = _mla(hip, t, True, kv=kv, pool=got_pool)
  assert torch.equal(t["lens"], before)  # (cache_seqlens is not advanced)
  assert torch.equal(got_storage.view(torch.int16), want_storage.view(torch.int16)), "the cache's storage differs from the torch-written reference"
  touched = (want_storage.view(torch.int16) != t["storage"].view(torch.int16)).any(dim=-1).sum().item()
  assert touched == len(lens) * snew  # (NaN rows became data: exactly the appended rows changed)
  ref = _ref(t, True, lens=used, pool=want_pool)
  vstat = R.visible_values(want_pool[..., :DV], used, t["table"])
  R.check(out, lse, ref, v=vstat, dtype=dtype, name=f"append Snew {snew} paged {paged}")
  # ... and attending over the written cache without kv= gives the same bits
  again = _mla(hip, t, True, pool=got_pool, lens=torch.tensor(used, dtype=torch.int32, device="cuda"))
  assert torch.equal(out, again[0]) and torch.equal(lse, again[1])


# ----------------------------------------------------------------------------- graph capture
def test_one_graph_follows_lengths_table_and_new_rows_written_in_place(hip):
  """Append + attention (+ merge, if the plan splits) captured once; two replays after cache_seqlens, block_table and kv were rewritten in place: each equals
  the eager call on the same state."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  lens0 = [5, 31, 64, 200]
  t = _case(lens0, 16, 1, 1, "bf16", seed=9, room=8)
  storage = t["storage"].clone()
  pool = R.reviewed(t["pool"], t["storage"], storage)
  pool.nan_to_num_(nan=0.25)  # (replays move lengths and pages around: every row must hold a number)
  lens = t["lens"].clone()
  table = t["table"].clone()
  kv = torch.randn((4, 1, 1, D), device="cuda", dtype=torch.bfloat16)
  call = lambda p: ffpa_attn_with_kvcache_mla(t["q"], p, DV, kv=kv, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, causal=True,
                                              return_softmax_lse=True)
  call(pool.clone())  # (warm: the library is loaded, the scratch is sized)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out_g, lse_g = call(pool)
  states = [(lens0, table.clone(), kv.clone()),
            ([0, 63, 65, 97], table.flip(0).contiguous(), torch.randn_like(kv)),
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
    assert torch.equal(after.view(torch.int16), storage.view(torch.int16)), n
    tt = dict(t, table=table)
    R.check(out_g, lse_g, _ref(tt, True, lens=[x + 1 for x in n], pool=pool), v=R.visible_values(pool[..., :DV], [x + 1 for x in n], table), dtype="bf16",
            name=f"graph replay at {n}")
