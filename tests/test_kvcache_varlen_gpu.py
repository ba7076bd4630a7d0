"""``ffpa_attn_varlen_with_kvcache`` on the GPU: a ragged step (token rows packed by ``cu_seqlens_q``) over a paged or contiguous cache, with the per-token append.

Outputs and LSE are held to ``kvcache_ref.check`` — the suite's allowance against the float64 restatement (tests/kvcache_varlen_ref.py), recomputed from the
reference of every case — and the caches to ``kvcache_ref.check_cache``: the whole storage bit-identical to the reference's but for the rotated dims of the
appended K rows (one ulp of the once-rounded float64 rotation).  Pools and slabs hold NaN wherever no key lives, so a read past a length or a write to a row
nobody owns shows.  On a uniform batch the call must equal ``ffpa_attn_with_kvcache`` / ``_window`` / ``_softcap`` to the bit.

Tiles: 128 rows x 64 keys at D <= 512, 64 rows x 32 keys above; pages of 64; Hq / Hkv = 8 / 2 unless said otherwise (GQA rows are packed into a tile when
``group x max_seqlen_q`` fits one).  The shapes are the smallest that cross each edge; every case builds its tensors on the CPU, where the reference runs."""

import pytest
import torch

import kvcache_ref as R
import kvcache_varlen_ref as V
from test_fwd_gpu import hip  # noqa: F401  (fixture)
from test_kvcache_serving_gpu import _launches

pytestmark = pytest.mark.gpu

PACKED = "(GQA heads packed into rows)"


def _dev(t: dict) -> dict:
  """A case's tensors on the GPU (fresh copies: the call writes the caches)."""
  return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in t.items()}


def _run(hip, d, *, max_seqlen_q=None, append_kv=True, rotary=True, positions=None, flags=0, **kw):
  """The public call on a case's device tensors -> (out, lse, the plan of its attention launch)."""
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache

  rot = dict(rotary_cos=d["cos"], rotary_sin=d["sin"]) if (append_kv and rotary) else {}
  kv = dict(k=d["k"], v=d["v"]) if append_kv else {}
  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_varlen_with_kvcache(d["q"], d["k_cache"], d["v_cache"], d["cu"], max(d["seqs"]) if max_seqlen_q is None else max_seqlen_q, d["lens"],
                                             d["table"], positions=positions, return_softmax_lse=True, **kv, **rot, **kw)
  torch.cuda.synchronize()
  assert len(plans) == 1, plans
  return out, lse, plans[0]


def _check(t, d, out, lse, ref, name, rotary_dim, extra=None):
  """Outputs over the real rows against the float64 reference (allowance from the reference's own rows and the V it reads), then both caches."""
  (o_ref, kc, vc, rotated, eff) = ref
  n = int(t["cu"][-1])
  vstat = R.visible_values(vc, eff, t["table"])
  ratio = R.check(out[None, :n], lse[None, :, :n], o_ref, v=vstat, dtype=t["dtype"], name=name, extra=extra)
  gk, gv = d["k_cache"].cpu(), d["v_cache"].cpu()
  R.check_cache(gk, kc, gk, kc, rotated, rotary_dim, name=name + " K")
  R.check_cache(gv, vc, gv, vc, [], 0, name=name + " V")
  print(f"[varlen kvcache] {ratio:.3f} {name}")
  return ratio


# ----------------------------------------------------------------------------- 1. a uniform batch is the existing calls, to the bit
@pytest.mark.parametrize("page", [64, 0])
@pytest.mark.parametrize("D, dtype", [(512, "bf16"), (512, "fp16"), (1024, "bf16")])
def test_uniform_batch_equals_the_existing_calls_bit_for_bit(hip, D, dtype, page):
  from ffpa_attn_amd import ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_softcap, ffpa_attn_with_kvcache_window

  B, Sq = 3, 4
  t = V.make_case([Sq] * B, [70, 0, 129], D=D, dtype=dtype, page=page, seed=D + page, rotary_dim=128)
  for what, interleaved, causal, kw in (("plain", True, False, {}), ("plain", False, True, {}), ("window", True, False, dict(window_size=(40, 0))),
                                        ("softcap", False, True, dict(softcap=30.0))):
    d, u = _dev(t), _dev(t)
    out, lse, _ = _run(hip, d, causal=causal, rotary_interleaved=interleaved, **kw)
    fn = {"plain": ffpa_attn_with_kvcache, "window": ffpa_attn_with_kvcache_window, "softcap": ffpa_attn_with_kvcache_softcap}[what]
    shape4 = lambda x: x.view(B, Sq, x.size(1), D)
    o_u, lse_u = fn(shape4(u["q"]), u["k_cache"], u["v_cache"], shape4(u["k"]), shape4(u["v"]), u["cos"], u["sin"], cache_seqlens=u["lens"], block_table=u["table"],
                    causal=causal, rotary_interleaved=interleaved, return_softmax_lse=True, **kw)
    torch.cuda.synchronize()
    name = f"{what} D{D} {dtype} page{page} interleaved={interleaved} causal={causal}"
    assert torch.equal(out.view(torch.int16), o_u.reshape(B * Sq, -1, D).view(torch.int16)), name
    assert torch.equal(lse.view(-1, B, Sq).permute(1, 0, 2), lse_u), name
    assert torch.equal(d["k_cache"].view(torch.int16), u["k_cache"].view(torch.int16)) and torch.equal(d["v_cache"].view(torch.int16), u["v_cache"].view(torch.int16)), name
    assert torch.isfinite(out.float()).all()


# ----------------------------------------------------------------------------- 2. ragged, rows not packed
@pytest.mark.parametrize("page", [64, 0])
@pytest.mark.parametrize("D", [512, 1024])
def test_ragged_unpacked(hip, D, page):
  """A 130-token chunk (two row tiles at D = 512, three at D = 1024), a decode, an empty sequence, a 3-token verification and a 64-token chunk in one call; causal
  and not, with append + rotary and against a pre-filled cache.  Shuffled pages; rows nobody appends to keep their NaN."""
  seqs, lens = [130, 1, 0, 3, 64], [0, 200, 50, 61, 64]
  t = V.make_case(seqs, lens, D=D, page=page, seed=D + page + 1, rotary_dim=64, bad_unused_ids=True)
  for causal in (True, False):
    for append_kv in (True, False):
      d = _dev(t)
      out, lse, plan = _run(hip, d, max_seqlen_q=130, append_kv=append_kv, causal=causal, rotary_interleaved=False)
      assert PACKED not in plan["kernel"], plan
      ref = V.reference(t, append_kv=append_kv, interleaved=False, causal=causal)
      _check(t, d, out, lse, ref, f"ragged D{D} page{page} causal={causal} append={append_kv} -> {plan['kernel']}", 64 if append_kv else 0)
      if not append_kv and causal:
        assert torch.isneginf(lse[:, :130]).all() and (out[:130] == 0).all()  # (the chunk's sequence holds no key: O = 0, LSE = -inf)


# ----------------------------------------------------------------------------- 3. ragged, (head, token) rows packed under a per-sequence token count
SEQS3, LENS3 = [1, 3, 0, 4, 2], [63, 64, 10, 127, 1]


@pytest.mark.parametrize("D, dtype", [(512, "bf16"), (512, "fp16"), (320, "bf16")])
@pytest.mark.parametrize("kw", [dict(), dict(window_size=(5, 0)), dict(softcap=50.0)], ids=["plain", "window", "softcap"])
def test_ragged_packed_rows(hip, D, dtype, kw):
  """Group 4 x max_seqlen_q 4 fits a tile: rows are (head, token) with every sequence's own token count; lengths straddle a page and a tile edge."""
  t = V.make_case(SEQS3, LENS3, D=D, dtype=dtype, seed=D + 3, rotary_dim=32)
  extra = None
  if "softcap" in kw:
    t["q"] = t["q"] * 64.0  # (exact in 16 bits; scaled scores of deviation ~ 64 sit deep in the tanh's bend: tests/test_kvcache_softcap_gpu.py)
  d = _dev(t)
  out, lse, plan = _run(hip, d, max_seqlen_q=4, causal=True, **kw)
  assert PACKED in plan["kernel"], plan
  ref = V.reference(t, causal=True, window=kw.get("window_size", (-1, -1)), softcap=kw.get("softcap", 0.0))
  if "softcap" in kw:
    # the kernel's tanh is off by <= 2^-21: a capped score by <= c 2^-21, each softmax weight by a factor <= e^(2 d), O by <= 2 d max|v| (test_kvcache_softcap_gpu.py)
    extra = 2.0 * kw["softcap"] * 2.0 ** -21 * R.visible_values(ref[2], ref[4], t["table"])[0]
    plain = V.reference(t, causal=True)[0][0]
    assert (plain - ref[0][0]).abs().max() > 0.05  # (the cap matters on these inputs)
  _check(t, d, out, lse, ref, f"packed rows D{D} {dtype} {kw} -> {plan['kernel']}", 32, extra)


# ----------------------------------------------------------------------------- 4. KV splits
def test_kv_splits(hip):
  seqs, lens = [1, 2], [2000, 700]
  t = V.make_case(seqs, lens, D=512, seed=44, rotary_dim=64)
  ref = V.reference(t, causal=True)
  got = {}
  for ns, flags in ((0, 0), (4, hip.FLAG_FORCE_SPLITS)):
    d = _dev(t)
    out, lse, plan = _run(hip, d, causal=True, num_splits=ns, flags=flags)
    _check(t, d, out, lse, ref, f"num_splits {ns} -> {plan}", 64)
    got[ns] = (out, lse, plan)
  assert got[4][2]["splits"] == 4, got[4][2]
  # ... and against each other: within one allowance of the float64 rows
  import numpy as np

  o_ref, lse_ref, pmax, p2sum = (x.cpu().numpy() for x in ref[0])
  stat = lambda x: np.transpose(x, (0, 2, 1))
  half_ulp, flip = R.allowance(o_ref, stat(pmax), stat(p2sum), R.visible_values(ref[2], ref[4], t["table"]), "bf16", noise=True)
  diff = (got[0][0].double() - got[4][0].double()).abs().cpu().numpy()[None]
  ratio = float((diff / (half_ulp + flip)).max())
  print(f"[varlen kvcache] split 0 vs 4: {ratio:.3f} of the allowance")
  assert ratio <= 1.0
  assert torch.allclose(got[0][1], got[4][1], atol=R.LSE_ATOL, rtol=R.LSE_RTOL)


# ----------------------------------------------------------------------------- 5. per-token rotary positions
def test_positions_rotate_at_the_depth_and_write_at_the_slot(hip):
  t = V.make_case(SEQS3, LENS3, D=512, seed=55, rotary_dim=128)
  owner = sum(([b] * n for b, n in enumerate(SEQS3)), [])
  pos = torch.tensor([LENS3[b] + dep for b, dep in zip(owner, V.tree_depths(SEQS3))], dtype=torch.int32)
  d = _dev(t)
  out, lse, plan = _run(hip, d, max_seqlen_q=4, causal=True, positions=pos.cuda())
  at_pos, at_slot = V.reference(t, causal=True, positions=pos), V.reference(t, causal=True)
  _check(t, d, out, lse, at_pos, f"positions = depths -> {plan['kernel']}", 128)
  # the reference that rotates at the slot is another result, by more than the allowance — in the outputs and in the cache: the case cannot pass by accident
  vstat = R.visible_values(at_slot[2], at_slot[4], t["table"])
  with pytest.raises(AssertionError):
    R.check(at_pos[0][0].to(torch.bfloat16), None, at_slot[0], v=vstat, dtype="bf16")
  with pytest.raises(AssertionError):
    R.check(out[None], lse[None], at_slot[0], v=vstat, dtype="bf16")
  gk = d["k_cache"].cpu()
  with pytest.raises(AssertionError):
    R.check_cache(gk, at_slot[1], gk, at_slot[1], at_slot[3], 128)
  # positions outside the tables are clamped to [0, seqlen_ro - 1]
  wild = torch.tensor([-7, 10 ** 6] * 5, dtype=torch.int32)
  d = _dev(t)
  out, lse, plan = _run(hip, d, max_seqlen_q=4, causal=True, positions=wild.cuda())
  _check(t, d, out, lse, V.reference(t, causal=True, positions=wild), "positions clamped", 128)


# ----------------------------------------------------------------------------- 6. edges
@pytest.mark.parametrize("page", [64, 0])
def test_capacity_negative_length_and_padding_rows(hip, page):
  """Sequence 0 appends 20 keys at 120 into a capacity of 128 (12 dropped, L = 128); sequence 1's length is -5 (acts as 0); 5 token rows behind cu[B] are padding:
  nothing is written for them.  Table entries past a sequence's last page hold ids far outside the pool: never read."""
  t = V.make_case([20, 3], [120, -5], D=128, page=page, seed=66 + page, rotary_dim=64, pad=5, pages_per_seq=2, capacity=128, bad_unused_ids=True)
  assert t["capacity"] == 128 and t["q"].size(0) == 28
  for causal in (True, False):
    d = _dev(t)
    out, lse, plan = _run(hip, d, max_seqlen_q=20, causal=causal)
    ref = V.reference(t, causal=causal)
    assert ref[4] == [128, 3]
    _check(t, d, out, lse, ref, f"edges page{page} causal={causal}", 64)


def test_a_batch_of_only_empty_sequences(hip):
  t = V.make_case([0, 0, 0], [5, 0, 70], D=128, seed=67, rotary_dim=64, pad=4)
  d = _dev(t)
  out, lse, _ = _run(hip, d, max_seqlen_q=1, causal=True)
  assert out.shape == (4, 8, 128) and lse.shape == (8, 4)
  for name in ("k_cache", "v_cache"):
    assert torch.equal(d[name].cpu().view(torch.int16), t[name].view(torch.int16)), name
  q_rot, used = torch.ops.ffpa_attn._kvcache_append_varlen_hip(d["q"], d["k_cache"], d["v_cache"], d["k"], d["v"], d["cu"], d["lens"], d["table"], d["cos"], d["sin"],
                                                               None, True, True)
  assert used.tolist() == [5, 0, 70]  # (written for sequences without a token too)
  # no token at all: empty tensors, nothing launched
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache

  out, lse = ffpa_attn_varlen_with_kvcache(d["q"][:0], d["k_cache"], d["v_cache"], d["cu"], 0, d["lens"], d["table"], k=d["k"][:0], v=d["v"][:0],
                                           return_softmax_lse=True)
  assert out.shape == (0, 8, 128) and lse.shape == (8, 0)


# ----------------------------------------------------------------------------- 7. one HIP graph, replays follow what is written in place
def test_graph_replay_follows_cu_seqlens_lengths_table_and_data(hip):
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache

  t = _dev(V.make_case([4, 1, 3], [70, 0, 129], D=512, seed=77, rotary_dim=64))
  g = torch.Generator(device="cuda").manual_seed(7)
  # (every page holds finite data: a replay under a permuted table reads pages another sequence owned)
  pristine_k = torch.randn(t["k_cache"].shape, generator=g, device="cuda").to(t["k_cache"].dtype)
  pristine_v = torch.randn(t["v_cache"].shape, generator=g, device="cuda").to(t["v_cache"].dtype)
  q, k, v, cu, lens, table = (t[n] for n in ("q", "k", "v", "cu", "lens", "table"))
  kw = dict(rotary_cos=t["cos"], rotary_sin=t["sin"], causal=True, rotary_interleaved=False, return_softmax_lse=True)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    ffpa_attn_varlen_with_kvcache(q, pristine_k.clone(), pristine_v.clone(), cu, 5, lens, table, k=k, v=v, **kw)  # (warm-up outside the capture)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out, lse = ffpa_attn_varlen_with_kvcache(q, t["k_cache"], t["v_cache"], cu, 5, lens, table, k=k, v=v, **kw)
  for split, new_lens, perm in (([4, 1, 3], [70, 0, 129], [0, 1, 2]), ([2, 5, 1], [64, 127, 3], [2, 0, 1]), ([0, 3, 5], [191, 1, 60], [1, 2, 0])):
    q.copy_(torch.randn(q.shape, generator=g, device="cuda").to(q.dtype))
    k.copy_(torch.randn(k.shape, generator=g, device="cuda").to(k.dtype))
    v.copy_(torch.randn(v.shape, generator=g, device="cuda").to(v.dtype))
    cu.copy_(torch.tensor([0, split[0], split[0] + split[1], 8], dtype=torch.int32))
    lens.copy_(torch.tensor(new_lens, dtype=torch.int32))
    table.copy_(table[perm].clone())
    t["k_cache"].copy_(pristine_k), t["v_cache"].copy_(pristine_v)
    graph.replay()
    kc_e, vc_e = pristine_k.clone(), pristine_v.clone()
    o_e, lse_e = ffpa_attn_varlen_with_kvcache(q.clone(), kc_e, vc_e, cu.clone(), 5, lens.clone(), table.clone(), k=k.clone(), v=v.clone(), **kw)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), o_e.view(torch.int16)) and torch.equal(lse, lse_e), split
    assert torch.equal(t["k_cache"].view(torch.int16), kc_e.view(torch.int16)) and torch.equal(t["v_cache"].view(torch.int16), vc_e.view(torch.int16)), split


# ----------------------------------------------------------------------------- 8. torch.compile
def test_under_torch_compile_fullgraph(hip):
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache

  t = _dev(V.make_case([4, 1, 3], [70, 0, 129], D=512, dtype="fp16", seed=88, rotary_dim=64))
  cos, sin = t["cos"], t["sin"]

  def f(q, kc, vc, cu, lens, table, k, v):
    o, lse = ffpa_attn_varlen_with_kvcache(q, kc, vc, cu, 4, lens, table, k=k, v=v, rotary_cos=cos, rotary_sin=sin, causal=True, return_softmax_lse=True)
    return o * 2, lse

  kc_c, vc_c = t["k_cache"].clone(), t["v_cache"].clone()
  args = (t["q"], t["cu"], t["lens"], t["table"], t["k"], t["v"])
  eager = f(args[0], t["k_cache"], t["v_cache"], *args[1:])
  compiled = torch.compile(f, fullgraph=True)(args[0], kc_c, vc_c, *args[1:])
  torch.cuda.synchronize()
  assert torch.equal(eager[0], compiled[0]) and torch.equal(eager[1], compiled[1])
  assert torch.equal(t["k_cache"].view(torch.int16), kc_c.view(torch.int16)) and torch.equal(t["v_cache"].view(torch.int16), vc_c.view(torch.int16))
