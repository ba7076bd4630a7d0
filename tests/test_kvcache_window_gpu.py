"""``ffpa_attn_with_kvcache_window`` on the GPU: every edge of the window build of the packed / paged kernel against the float64 restatement
(tests/kvcache_window_ref.py, outputs held to ``kvcache_ref.allowance``, LSE to atol 2e-4 / rtol 2e-5), bit identity (bf16) with ``ffpa_attn_with_kvcache`` where
that call can say the same thing, KV splits, skipped tiles filled with NaN, the contiguous route, the append + rotary, empty sequences and graph capture.
Tiles: 128 rows x 64 keys at D <= 512, 64 rows x 32 keys above; the shapes are the smallest that cross each edge."""

import pytest
import torch

import kvcache_ref as R
import kvcache_window_ref as W
from test_fwd_gpu import hip  # noqa: F401  (fixture)
from test_kvcache_serving_gpu import _launches, make_case

pytestmark = pytest.mark.gpu

DECODE_LENS = [1, 63, 321, 1500]


def _window(hip, t, window, *, causal=False, flags=0, num_splits=0, k=None, v=None, cos=None, sin=None, lens=None):
  """The public call on a materialised case -> (out, lse, plan of its attention launch)."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_window

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_window(t["q"], t["k_cache"], t["v_cache"], k, v, cos, sin, cache_seqlens=t["lens"] if lens is None else lens,
                                             block_table=t["table"], window_size=window, causal=causal, num_splits=num_splits, return_softmax_lse=True)
  assert len(plans) == 1 and "_window_kernel<" in plans[0]["kernel"], plans
  return out, lse, plans[0]


def _plain(hip, t, causal, *, flags=0, num_splits=0):
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache(t["q"], t["k_cache"], t["v_cache"], cache_seqlens=t["lens"], block_table=t["table"], causal=causal, num_splits=num_splits,
                                      return_softmax_lse=True)
  return out, lse, plans[0]


_CASES: dict = {}


def _case(**kw):
  """A materialised case, its effective lengths and V statistics: made once per shape and shared (nothing writes to it unless the test clones)."""
  key = tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items()))
  if key not in _CASES:
    c = make_case(**kw)
    t = R.materialize(c, "cuda")
    eff = R.effective_lens(c)
    _CASES[key] = (c, t, eff, R.visible_values(t["v_cache"], eff, t["table"]))
  return _CASES[key]


def _check(hip, c, t, eff, vstat, window, causal=False, num_splits=0, flags=0, what=""):
  ref = W.attend(t["q"], t["k_cache"], t["v_cache"], eff, t["table"], window, causal)
  out, lse, plan = _window(hip, t, window, causal=causal, num_splits=num_splits, flags=flags)
  name = f"{what}: D{c['D']} {c['dtype']} Sq{c['Sq']} page{c['page']} lens{c['lens']} window {window} causal={causal} num_splits {num_splits} -> {plan}"
  ratio = R.check(out, lse, ref, v=vstat, dtype=c["dtype"], name=name)
  print(f"[window] {ratio:.3f} {name}")
  return out, lse, plan, ref


# ----------------------------------------------------------------------------- decode
@pytest.mark.parametrize("d, dtype", [(128, "bf16"), (320, "bf16"), (512, "bf16"), (512, "fp16"), (1024, "bf16")])
def test_decode(hip, d, dtype):
  """One token per sequence, GQA 8 / 2 packed into rows, pages of 64: only self (0), mid-tile (100), tile-aligned (128), wider than every sequence (4000),
  a left bound without the causal edge (100, -1) and a right bound alone (-1, 16)."""
  c, t, eff, vstat = _case(D=d, dtype=dtype, page=64, heads=(8, 2), lens=DECODE_LENS, Sq=1, seed=d)
  for window in ((0, 0), (100, 0), (128, 0), (4000, 0), (100, -1), (-1, 16)):
    out, lse, plan, ref = _check(hip, c, t, eff, vstat, window, what="decode")
    assert "(GQA heads packed into rows)" in plan["kernel"] and plan["block_keys"] == (64 if d <= 512 else 32)
  # causal=True means right = 0 whatever was given
  a = _window(hip, t, (100, 7), causal=True)
  b = _window(hip, t, (100, 0))
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------- packed rows (speculative decode)
@pytest.mark.parametrize("d", [128, 512, 1024])
def test_packed_rows(hip, d):
  """Four tokens per sequence, rows are (head, token); L = 3 < Sq: the first token's position is below key 0 — an empty row."""
  c, t, eff, vstat = _case(D=d, dtype="bf16", page=64, heads=(8, 2), lens=[3, 200, 1000], Sq=4, seed=d + 1)
  for window, causal in (((70, 0), False), ((70, -1), True), ((70, 1), False), ((70, -1), False)):
    out, lse, plan, ref = _check(hip, c, t, eff, vstat, window, causal, what="packed rows")
    assert "(GQA heads packed into rows)" in plan["kernel"]
    if (0 if causal else window[1]) == 0:
      assert torch.isneginf(lse[0, :, 0]).all() and (out[0, 0] == 0).all() and torch.isfinite(lse[0, :, 1:]).all()


# ----------------------------------------------------------------------------- prefill chunk
@pytest.mark.parametrize("d", [512, 1024])
@pytest.mark.parametrize("heads", [(2, 2), (4, 2)])
def test_prefill_chunk(hip, d, heads):
  """Sq 200 over 700 keys: two row tiles at D = 512, four at D = 1024.  left = 48 is less than a key tile: a wave's first tiles are wholly hidden for its later
  rows (a running max of -inf followed by finite values); 130 spans tiles; (48, 16) non-causal has both edges inside a tile; (-1, 16) the right edge alone."""
  c, t, eff, vstat = _case(D=d, dtype="bf16", page=64, heads=heads, lens=[700], Sq=200, seed=d + 2)
  for window in ((48, 0), (130, 0), (48, 16), (-1, 16)):
    out, lse, plan, ref = _check(hip, c, t, eff, vstat, window, what="prefill chunk")
    assert plan["row_tiles"] == (2 if d <= 512 else 4) and "(GQA heads packed into rows)" not in plan["kernel"], plan
    assert torch.isfinite(lse).all()


# ----------------------------------------------------------------------------- forced splits
@pytest.mark.parametrize("d", [512, 1024])
def test_kv_splits(hip, d):
  """left = 128: three windowed 64-key tiles (five of 32) — at five ranges some are empty (weight 0 in the merge); every split count agrees with float64 and with
  the unsplit launch to merge rounding (two allowances)."""
  for kw, window in ((dict(lens=[1500], Sq=1, heads=(8, 2)), (128, 0)), (dict(lens=[700], Sq=200, heads=(2, 2)), (128, 0))):
    c, t, eff, vstat = _case(D=d, dtype="bf16", page=64, seed=d + 3, **kw)
    outs = {}
    for ns in (1, 2, 5):
      out, lse, plan, ref = _check(hip, c, t, eff, vstat, window, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS, what="KV splits")
      outs[ns] = (out, lse, plan)
    assert outs[1][2]["splits"] == 1 and outs[2][2]["splits"] == 2 and 2 <= outs[5][2]["splits"] <= 5, [o[2] for o in outs.values()]
    assert all("ffpa_varlen_merge_kernel" in outs[ns][2]["kernel"] for ns in (2, 5))
    o_ref, lse_ref, pmax, p2sum = (x.cpu().numpy() for x in ref)
    import numpy as np

    stat = lambda x: np.transpose(x, (0, 2, 1))
    half_ulp, flip = R.allowance(o_ref, stat(pmax), stat(p2sum), vstat, "bf16", noise=True)
    for ns in (2, 5):
      err = (outs[ns][0].double() - outs[1][0].double()).abs().cpu().numpy()
      assert (err <= 2 * (half_ulp + flip)).all(), f"num_splits {ns} vs 1: {err.max():.3e}"
      torch.testing.assert_close(outs[ns][1], outs[1][1], atol=2 * R.LSE_ATOL, rtol=2 * R.LSE_RTOL)


# ----------------------------------------------------------------------------- skipped tiles are not walked
@pytest.mark.parametrize("d", [512, 1024])
def test_tiles_outside_the_window_are_not_walked(hip, d):
  """Every key tile that lies wholly outside every row's window holds NaN in K and V: a kernel that walked those tiles and masked them would produce 0 x NaN."""
  c, t0, eff, vstat = _case(D=d, dtype="bf16", page=64, heads=(8, 2), lens=DECODE_LENS, Sq=1, seed=d)
  t = dict(t0, k_cache=t0["k_cache"].clone(), v_cache=t0["v_cache"].clone())
  window, bc = (128, 0), (64 if d <= 512 else 32)
  poisoned = 0
  for b, n in enumerate(eff):
    seen = W.seen_tiles(1, n, window, False, bc)
    for tile in range(-(-n // bc)):
      if tile not in seen:
        page, row = int(t["table"][b, tile * bc // 64]), tile * bc % 64
        t["k_cache"][page, row:row + bc] = float("nan")
        t["v_cache"][page, row:row + bc] = float("nan")
        poisoned += 1
  assert poisoned >= 20  # (the 1500-key sequence alone has 21 such 64-key tiles)
  out, lse, plan, ref = _check(hip, c, t, eff, vstat, window, what="NaN outside the window")
  assert torch.isfinite(out).all() and torch.isfinite(lse).all()
  clean = _window(hip, t0, window)
  assert torch.equal(out, clean[0]) and torch.equal(lse, clean[1])


# ----------------------------------------------------------------------------- identities (bf16)
@pytest.mark.parametrize("d, sq, lens, heads", [(512, 1, DECODE_LENS, (8, 2)), (1024, 1, DECODE_LENS, (8, 2)), (128, 4, [3, 200, 1000], (8, 2)), (512, 200, [700], (2, 2)),
                                                (1024, 200, [700], (4, 2))])
@pytest.mark.parametrize("page", [64, 0])
def test_identities_with_the_plain_call(hip, d, sq, lens, heads, page):
  """No window is the plain call's bits: (-1, -1) the non-causal call; (-1, 0), causal=True and (capacity, 0) the causal call."""
  c, t, eff, vstat = _case(D=d, dtype="bf16", page=page, heads=heads, lens=lens, Sq=sq, seed=d + 4)
  cap = R.capacity_of(t["k_cache"], t["table"])
  for ns in (0, 1):
    o0, l0, p0 = _plain(hip, t, False, num_splits=ns)
    o1, l1, p1 = _plain(hip, t, True, num_splits=ns)
    for window, causal, (o, l, p) in (((-1, -1), False, (o0, l0, p0)), ((-1, 0), False, (o1, l1, p1)), ((-1, -1), True, (o1, l1, p1)), ((cap, 0), False, (o1, l1, p1)),
                                      ((cap, 5), True, (o1, l1, p1))):
      out, lse, plan = _window(hip, t, window, causal=causal, num_splits=ns)
      name = f"D{d} Sq{sq} page{page} window {window} causal={causal} num_splits {ns}: {plan} vs {p}"
      assert plan["kernel"].replace("_window_kernel<", "_kernel<") == p["kernel"] and plan["splits"] == p["splits"], name
      assert torch.equal(out, o) and torch.equal(lse, l), name


def test_fp16_without_a_window_is_held_to_the_allowance(hip):
  c, t, eff, vstat = _case(D=512, dtype="fp16", page=64, heads=(8, 2), lens=DECODE_LENS, Sq=1, seed=9)
  for window, causal in (((-1, -1), False), ((-1, 0), False), ((-1, -1), True)):
    _check(hip, c, t, eff, vstat, window, causal, what="fp16 no window")


# ----------------------------------------------------------------------------- routes
@pytest.mark.parametrize("d", [320, 512, 1024])
def test_contiguous_cache(hip, d):
  """A [B, capacity, Hkv, D] cache through the packed kernel's window build (128-key tiles at D = 320)."""
  for sq, lens in ((1, DECODE_LENS), (200, [700])):
    c, t, eff, vstat = _case(D=d, dtype="bf16", page=0, heads=(8, 2) if sq == 1 else (2, 2), lens=lens, Sq=sq, seed=d + 5)
    for window in ((100, 0), (128, 0), (48, 16)):
      out, lse, plan, ref = _check(hip, c, t, eff, vstat, window, what="contiguous")
      assert "ffpa_fwd_m16_varlen_window_kernel" in plan["kernel"] and plan["block_keys"] == (128 if d == 320 else 64 if d <= 512 else 32)


@pytest.mark.parametrize("page", [64, 0])
def test_append_with_rotary_equals_appending_first(hip, page):
  """k / v appended with rotary (rotary_dim = D) inside the window call == appending through ffpa_attn_with_kvcache and calling the window entry on the longer
  cache, to the bit (bf16) — and both agree with float64."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  d, sq = 128, 4
  c = make_case(D=d, dtype="bf16", page=page, heads=(8, 2), lens=[5, 200, 1000], Sq=sq, Snew=sq, rotary_dim=d, causal=True, seed=77)
  t = R.materialize(c, "cuda")
  ref, kview_w, vview_w, ks_w, vs_w, rotated = R.reference(c, t)  # (the reference's caches after the append; its q rotated)
  clone = lambda: dict(t, k_cache=R.reviewed(t["k_cache"], t["k_storage"], t["k_storage"].clone()), v_cache=R.reviewed(t["v_cache"], t["v_storage"], t["v_storage"].clone()))
  window = (70, 0)
  # (a) the window call appends
  ta = clone()
  out_a, lse_a, _ = _window(hip, ta, window, causal=True, k=t["k"], v=t["v"], cos=t["cos"], sin=t["sin"])
  # (b) the plain call appends (its output is not used), then the window call attends over the longer cache with the rotated q
  tb = clone()
  ffpa_attn_with_kvcache(tb["q"], tb["k_cache"], tb["v_cache"], t["k"], t["v"], t["cos"], t["sin"], cache_seqlens=t["lens"], block_table=t["table"], causal=True)
  assert torch.equal(ta["k_cache"].nan_to_num(7.0), tb["k_cache"].nan_to_num(7.0)) and torch.equal(ta["v_cache"].nan_to_num(7.0), tb["v_cache"].nan_to_num(7.0))
  q_rot, post, _ = R.append(R.reviewed(t["k_cache"], t["k_storage"], t["k_storage"].clone()), R.reviewed(t["v_cache"], t["v_storage"], t["v_storage"].clone()),
                            t["k"], t["v"], c["lens"], t["table"], t["cos"], t["sin"], True, True, q=t["q"])
  from ffpa_attn_amd import hip as hip_mod

  q_dev, _ = hip_mod.kvcache_append(t["q"], clone()["k_cache"], clone()["v_cache"], t["k"], t["v"], t["lens"], t["table"], t["cos"], t["sin"], True, True)
  tb2 = dict(tb, q=q_dev)
  out_b, lse_b, _ = _window(hip, tb2, window, causal=True, lens=torch.tensor(post, dtype=torch.int32, device="cuda"))
  assert torch.equal(out_a, out_b) and torch.equal(lse_a, lse_b)
  want = W.attend(q_rot.to(torch.bfloat16), kview_w, vview_w, post, t["table"], window, True)
  R.check(out_a, lse_a, want, v=R.visible_values(vview_w, post, t["table"]), dtype="bf16", name=f"append + rotary page{page}")


# ----------------------------------------------------------------------------- empty sequences
@pytest.mark.parametrize("d, sq", [(512, 1), (1024, 1), (128, 4)])
def test_an_empty_sequence_in_the_batch(hip, d, sq):
  c, t, eff, vstat = _case(D=d, dtype="bf16", page=64, heads=(8, 2), lens=[300, 0, 70], Sq=sq, seed=d + 6)
  out, lse, plan, ref = _check(hip, c, t, eff, vstat, (100, 0), what="empty sequence")
  assert (out[1] == 0).all() and torch.isneginf(lse[1]).all() and torch.isfinite(lse[0]).all() and torch.isfinite(lse[2, :, -1]).all()
  # the other sequences are what they are without it
  c2, t2, eff2, vstat2 = c, dict(t, lens=torch.tensor([300, 64, 70], dtype=torch.int32, device="cuda")), [300, 64, 70], vstat
  out2, lse2, _ = _window(hip, t2, (100, 0))
  assert torch.equal(out[0], out2[0]) and torch.equal(out[2], out2[2]) and torch.equal(lse[0], lse2[0]) and torch.equal(lse[2], lse2[2])


# ----------------------------------------------------------------------------- graph capture
def test_graph_replay_follows_cache_seqlens_written_in_place(hip):
  """The decode case captured once on short lengths; the lengths written in place grow across tile and page boundaries (100 -> 321, 700 -> 1500), one sequence
  stays inside its tile (30 -> 63), one becomes empty."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_window

  c, t0, eff, vstat = _case(D=512, dtype="bf16", page=64, heads=(8, 2), lens=DECODE_LENS, Sq=1, seed=512)
  first, new = [1, 30, 100, 700], [0, 63, 321, 1500]
  lens = torch.tensor(first, dtype=torch.int32, device="cuda")
  call = lambda: ffpa_attn_with_kvcache_window(t0["q"], t0["k_cache"], t0["v_cache"], cache_seqlens=lens, block_table=t0["table"], window_size=(100, 0),
                                               return_softmax_lse=True)
  call()  # (warm: the library is loaded, the scratch is sized)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out_g, lse_g = call()
  graph.replay()
  torch.cuda.synchronize()
  eager = call()
  assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1])
  R.check(out_g, lse_g, W.attend(t0["q"], t0["k_cache"], t0["v_cache"], first, t0["table"], (100, 0), False), v=vstat, dtype="bf16", name="graph replay")
  lens.copy_(torch.tensor(new, dtype=torch.int32, device="cuda"))
  graph.replay()
  torch.cuda.synchronize()
  eager = call()
  assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1])
  R.check(out_g, lse_g, W.attend(t0["q"], t0["k_cache"], t0["v_cache"], new, t0["table"], (100, 0), False), v=vstat, dtype="bf16", name="graph replay on new lengths")
