"""``ffpa_attn_with_kvcache_softcap`` on the GPU: the soft-capping build of the packed / paged kernel against the float64 restatement
(tests/kvcache_softcap_ref.py), at c = 30 and c = 50, with and without a window.

INPUTS THAT MAKE THE CAP MATTER.  The cases are test_kvcache_window_gpu.py's (``make_case`` draws q, k ~ N(0, 1), so ``softmax_scale * q.k`` ~ N(0, 1)); the
materialised q is multiplied by FACTOR[c] — 32 at c = 30, 64 at c = 50, powers of two, so the 16-bit q stays exact — which gives scaled scores of standard
deviation 32 / 64: |score| passes 2 c on about 6 % / 12 % of the keys and the largest of a row's few hundred scores sits near 3 c, deep in the tanh's bend.  The
factors were chosen on the CPU with the float64 reference (capped against uncapped outputs of these cases, drawn on the CPU; share of the non-empty rows that
differ by more than 10 allowances): with 32 at c = 30 the share is 0.73 ... 1.00 over the decode, packed-row, chunk and split cases, with 64 at c = 50 it is
0.73 ... 1.00 (rows with a single visible key cannot differ: a quarter of the decode rows); 32 at c = 50 gives 0.38 (decode, D 128, window 100) and 0.49 (packed
rows, window 70), 8 at c = 30 gives 0.34 — too small.  Every case asserts the same thing on the data it runs on (``_cap_matters``): a kernel that ignored ``softcap`` could not pass.

ALLOWANCE.  Outputs are held to ``kvcache_ref.check`` (``allowance`` with its noise term) plus ``extra = 2 c 2^-21 max|v|``: the kernel's tanh has absolute error
eps_t <= 2^-21 (tests/test_kvcache_softcap.py), a capped score is off by at most c eps_t, and perturbing every score of a row by at most d moves each softmax weight
by at most a factor e^(2 d), so |dO| <= 2 d max|v| to first order.  LSE is held to the existing LSE_ATOL / LSE_RTOL (c 2^-21 = 2.4e-5 at c = 50).

Tiles: 128 rows x 64 keys at D <= 512, 64 rows x 32 keys above; the shapes are the smallest that cross each edge."""

import numpy as np
import pytest
import torch

import kvcache_ref as R
import kvcache_softcap_ref as S
from test_fwd_gpu import hip  # noqa: F401  (fixture)
from test_kvcache_serving_gpu import _launches, make_case

pytestmark = pytest.mark.gpu

DECODE_LENS = [1, 63, 321, 1500]
CAPS = (30.0, 50.0)
FACTOR = {30.0: 32.0, 50.0: 64.0}


def _softcap(hip, t, cap, window=None, *, causal=False, flags=0, num_splits=0, k=None, v=None, cos=None, sin=None, lens=None, family="_softcap_kernel<"):
  """The public call on a materialised case -> (out, lse, plan of its attention launch)."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_softcap

  kw = {} if window is None else dict(window_size=window)
  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_softcap(t["q"], t["k_cache"], t["v_cache"], k, v, cos, sin, cache_seqlens=t["lens"] if lens is None else lens,
                                              block_table=t["table"], softcap=cap, causal=causal, num_splits=num_splits, return_softmax_lse=True, **kw)
  assert len(plans) == 1 and family in plans[0]["kernel"], plans
  return out, lse, plans[0]


_CASES: dict = {}


def _case(cap, factor=None, **kw):
  """A materialised case with q scaled for ``cap``, its effective lengths and V statistics: made once per (shape, factor) and shared (nothing writes to it)."""
  factor = FACTOR[cap] if factor is None else factor
  key = (factor,) + tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items()))
  if key not in _CASES:
    c = make_case(**kw)
    t = R.materialize(c, "cuda")
    t["q"] = t["q"] * factor
    assert torch.isfinite(t["q"]).all()
    eff = R.effective_lens(c)
    _CASES[key] = (c, t, eff, R.visible_values(t["v_cache"], eff, t["table"]))
  return _CASES[key]


def _extra(cap, vstat) -> float:
  vmax = float(vstat[0]) if isinstance(vstat, tuple) else float(vstat.detach().float().abs().max().item())
  return 2.0 * cap * 2.0 ** -21 * vmax


def _cap_matters(c, ref, t, eff, vstat, window, causal, name):
  """On the float64 side: the capped and the uncapped outputs differ by more than 10 allowances in at least half of the non-empty rows."""
  o_ref, lse_ref, pmax, p2sum = (x.cpu().numpy() for x in ref)
  plain = S.attend(t["q"], t["k_cache"], t["v_cache"], eff, t["table"], window or (-1, -1), causal, softcap=0.0)[0].cpu().numpy()
  stat = lambda x: np.transpose(x, (0, 2, 1))
  half_ulp, flip = R.allowance(o_ref, stat(pmax), stat(p2sum), vstat, c["dtype"], noise=True)
  rows = (np.abs(plain - o_ref) > 10.0 * (half_ulp + flip)).any(axis=-1)  # [B, Sq, Hq]
  live = np.isfinite(stat(lse_ref))
  share = rows[live].mean()
  assert share >= 0.5, f"{name}: the cap moves only {share:.0%} of the non-empty rows by more than 10 allowances"
  return share


def _check(hip, cap, c, t, eff, vstat, window=None, causal=False, num_splits=0, flags=0, what="", matters=True):
  ref = S.attend(t["q"], t["k_cache"], t["v_cache"], eff, t["table"], window or (-1, -1), causal, softcap=cap)
  out, lse, plan = _softcap(hip, t, cap, window, causal=causal, num_splits=num_splits, flags=flags)
  name = f"{what}: c {cap} D{c['D']} {c['dtype']} Sq{c['Sq']} page{c['page']} lens{c['lens']} window {window} causal={causal} num_splits {num_splits} -> {plan}"
  share = _cap_matters(c, ref, t, eff, vstat, window, causal, name) if matters else float("nan")
  ratio = R.check(out, lse, ref, v=vstat, dtype=c["dtype"], name=name, extra=_extra(cap, vstat))
  print(f"[softcap] {ratio:.3f} (cap matters in {share:.0%} of the rows) {name}")
  return out, lse, plan, ref


# ----------------------------------------------------------------------------- decode
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("d, dtype", [(128, "bf16"), (512, "bf16"), (512, "fp16"), (576, "bf16"), (1024, "bf16")])
def test_decode(hip, d, dtype, cap):
  """One token per sequence, GQA 8 / 2 packed into rows, pages of 64, without a window and with (100, 0).  Length 63 and the tile tails leave finite garbage
  behind the last key: a tanh applied after the mask would turn its -inf into -c, a weight that is not 0."""
  c, t, eff, vstat = _case(cap, D=d, dtype=dtype, page=64, heads=(8, 2), lens=DECODE_LENS, Sq=1, seed=d)
  for window in (None, (100, 0)):
    out, lse, plan, ref = _check(hip, cap, c, t, eff, vstat, window, what="decode")
    assert "(GQA heads packed into rows)" in plan["kernel"] and plan["block_keys"] == (64 if d <= 512 else 32)
    assert plan["kernel"].startswith(f"ffpa_fwd_m16_paged_softcap_kernel<{dtype}, {d}")


# ----------------------------------------------------------------------------- packed rows (speculative decode)
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("d", [128, 512, 1024])
def test_packed_rows(hip, d, cap):
  """Four tokens per sequence, rows are (head, token), causal; L = 3 < Sq: the first token's position is below key 0 — an empty row."""
  c, t, eff, vstat = _case(cap, D=d, dtype="bf16", page=64, heads=(8, 2), lens=[3, 200, 1000], Sq=4, seed=d + 1)
  for window in ((70, 0), None):
    out, lse, plan, ref = _check(hip, cap, c, t, eff, vstat, window, True, what="packed rows")
    assert "(GQA heads packed into rows)" in plan["kernel"]
    assert torch.isneginf(lse[0, :, 0]).all() and (out[0, 0] == 0).all() and torch.isfinite(lse[0, :, 1:]).all()


# ----------------------------------------------------------------------------- prefill chunk
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("d", [512, 1024])
@pytest.mark.parametrize("heads", [(2, 2), (4, 2)])
def test_prefill_chunk(hip, d, heads, cap):
  """Sq 200 over 700 keys, causal and (48, 0): two row tiles at D = 512 (the D <= 512 softmax site), four at D = 1024 (the piped split-D site); the running max
  grows over capped scores from tile to tile."""
  c, t, eff, vstat = _case(cap, D=d, dtype="bf16", page=64, heads=heads, lens=[700], Sq=200, seed=d + 2)
  for window, causal in ((None, True), ((48, 0), False)):
    out, lse, plan, ref = _check(hip, cap, c, t, eff, vstat, window, causal, what="prefill chunk")
    assert plan["row_tiles"] == (2 if d <= 512 else 4) and "(GQA heads packed into rows)" not in plan["kernel"], plan
    assert torch.isfinite(lse).all()


# ----------------------------------------------------------------------------- forced splits
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("d", [512, 1024])
def test_kv_splits(hip, d, cap):
  """Every split count agrees with float64 and with the unsplit launch to merge rounding (two allowances): the partials are ordinary (O, LSE) states."""
  for kw, window, causal in ((dict(lens=[1500], Sq=1, heads=(8, 2)), None, False), (dict(lens=[700], Sq=200, heads=(2, 2)), (128, 0), False)):
    c, t, eff, vstat = _case(cap, D=d, dtype="bf16", page=64, seed=d + 3, **kw)
    outs = {}
    for ns in (1, 2, 5):
      out, lse, plan, ref = _check(hip, cap, c, t, eff, vstat, window, causal, num_splits=ns, flags=hip.FLAG_FORCE_SPLITS, what="KV splits")
      outs[ns] = (out, lse, plan)
    assert outs[1][2]["splits"] == 1 and outs[2][2]["splits"] == 2 and 2 <= outs[5][2]["splits"] <= 5, [o[2] for o in outs.values()]
    assert all("ffpa_varlen_merge_kernel" in outs[ns][2]["kernel"] for ns in (2, 5))
    o_ref, lse_ref, pmax, p2sum = (x.cpu().numpy() for x in ref)
    stat = lambda x: np.transpose(x, (0, 2, 1))
    half_ulp, flip = R.allowance(o_ref, stat(pmax), stat(p2sum), vstat, "bf16", noise=True)
    for ns in (2, 5):
      err = (outs[ns][0].double() - outs[1][0].double()).abs().cpu().numpy()
      assert (err <= 2 * (half_ulp + flip)).all(), f"num_splits {ns} vs 1: {err.max():.3e}"
      torch.testing.assert_close(outs[ns][1], outs[1][1], atol=2 * R.LSE_ATOL, rtol=2 * R.LSE_RTOL)


# ----------------------------------------------------------------------------- routes
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("d", [512, 1024])
def test_contiguous_cache(hip, d, cap):
  """A [B, capacity, Hkv, D] cache through the packed kernel's soft-capping build: one decode case and one chunk case."""
  for sq, lens, window, causal in ((1, DECODE_LENS, (100, 0), False), (200, [700], None, True)):
    c, t, eff, vstat = _case(cap, D=d, dtype="bf16", page=0, heads=(8, 2) if sq == 1 else (2, 2), lens=lens, Sq=sq, seed=d + 5)
    out, lse, plan, ref = _check(hip, cap, c, t, eff, vstat, window, causal, what="contiguous")
    assert "ffpa_fwd_m16_varlen_softcap_kernel" in plan["kernel"] and plan["block_keys"] == (64 if d <= 512 else 32)


@pytest.mark.parametrize("page", [64, 0])
def test_append_with_rotary_equals_appending_first(hip, page):
  """k / v appended with rotary (rotary_dim = D) inside the soft-capping call == appending through ffpa_attn_with_kvcache_window and calling the new entry
  without k / v on the longer cache: identical bits, identical caches — and both agree with float64."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_window
  from ffpa_attn_amd import hip as hip_mod

  cap, d, sq = 50.0, 128, 4
  c = make_case(D=d, dtype="bf16", page=page, heads=(8, 2), lens=[5, 200, 1000], Sq=sq, Snew=sq, rotary_dim=d, causal=True, seed=78)
  t = R.materialize(c, "cuda")
  t["q"] = t["q"] * FACTOR[cap]
  ref, kview_w, vview_w, ks_w, vs_w, rotated = R.reference(c, t)  # (the reference's caches after the append)
  clone = lambda: dict(t, k_cache=R.reviewed(t["k_cache"], t["k_storage"], t["k_storage"].clone()), v_cache=R.reviewed(t["v_cache"], t["v_storage"], t["v_storage"].clone()))
  window = (70, 0)
  # (a) the soft-capping call appends
  ta = clone()
  out_a, lse_a, _ = _softcap(hip, ta, cap, window, causal=True, k=t["k"], v=t["v"], cos=t["cos"], sin=t["sin"])
  # (b) the window call appends (its output is not used), then the soft-capping call attends over the longer cache with the rotated q
  tb = clone()
  ffpa_attn_with_kvcache_window(tb["q"], tb["k_cache"], tb["v_cache"], t["k"], t["v"], t["cos"], t["sin"], cache_seqlens=t["lens"], block_table=t["table"],
                                window_size=window, causal=True)
  assert torch.equal(ta["k_cache"].nan_to_num(7.0), tb["k_cache"].nan_to_num(7.0)) and torch.equal(ta["v_cache"].nan_to_num(7.0), tb["v_cache"].nan_to_num(7.0))
  q_rot, post, _ = R.append(R.reviewed(t["k_cache"], t["k_storage"], t["k_storage"].clone()), R.reviewed(t["v_cache"], t["v_storage"], t["v_storage"].clone()),
                            t["k"], t["v"], c["lens"], t["table"], t["cos"], t["sin"], True, True, q=t["q"])
  q_dev, _ = hip_mod.kvcache_append(t["q"], clone()["k_cache"], clone()["v_cache"], t["k"], t["v"], t["lens"], t["table"], t["cos"], t["sin"], True, True)
  tb2 = dict(tb, q=q_dev)
  out_b, lse_b, _ = _softcap(hip, tb2, cap, window, causal=True, lens=torch.tensor(post, dtype=torch.int32, device="cuda"))
  assert torch.equal(out_a, out_b) and torch.equal(lse_a, lse_b)
  vstat = R.visible_values(vview_w, post, t["table"])
  want = S.attend(q_rot.to(torch.bfloat16), kview_w, vview_w, post, t["table"], window, True, softcap=cap)
  R.check(out_a, lse_a, want, v=vstat, dtype="bf16", name=f"append + rotary page{page}", extra=_extra(cap, vstat))


@pytest.mark.parametrize("d, sq, lens, heads", [(512, 1, DECODE_LENS, (8, 2)), (1024, 200, [700], (4, 2))])
def test_softcap_zero_is_the_window_call(hip, d, sq, lens, heads):
  """softcap = 0 forwards to ffpa_attn_with_kvcache_window: a *_window_kernel launch and its bits."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_window

  c, t, eff, vstat = _case(30.0, D=d, dtype="bf16", page=64, heads=heads, lens=lens, Sq=sq, seed=d + 4)
  for window, causal in (((100, 0), False), ((-1, -1), True)):
    want = ffpa_attn_with_kvcache_window(t["q"], t["k_cache"], t["v_cache"], cache_seqlens=t["lens"], block_table=t["table"], window_size=window, causal=causal,
                                         return_softmax_lse=True)
    for zero in (0, 0.0):
      out, lse, plan = _softcap(hip, t, zero, window, causal=causal, family="_window_kernel<")
      assert "_softcap" not in plan["kernel"]
      assert torch.equal(out, want[0]) and torch.equal(lse, want[1])


@pytest.mark.parametrize("cap", CAPS)
def test_very_large_scores_saturate_to_the_cap(hip, cap):
  """q x 1e4 at D = 128: nearly every score sits at +- c exactly (e = inf / e = 0 in the kernel's chain); finite outputs that match float64."""
  for sq, lens, window, causal in ((1, DECODE_LENS, None, False), (4, [3, 200, 1000], (70, 0), True)):
    c, t, eff, vstat = _case(cap, factor=1e4, D=128, dtype="bf16", page=64, heads=(8, 2), lens=lens, Sq=sq, seed=131)
    out, lse, plan, ref = _check(hip, cap, c, t, eff, vstat, window, causal, what="saturated")
    assert torch.isfinite(out).all() and not torch.isnan(lse).any() and not torch.isposinf(lse).any()


# ----------------------------------------------------------------------------- graph capture
def test_graph_replay_follows_cache_seqlens_written_in_place(hip):
  """The decode case captured once on short lengths; the lengths written in place grow across tile and page boundaries, one sequence becomes empty."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_softcap

  cap, window = 50.0, (100, 0)
  c, t0, eff, vstat = _case(cap, D=512, dtype="bf16", page=64, heads=(8, 2), lens=DECODE_LENS, Sq=1, seed=512)
  first, new = [1, 30, 100, 700], [0, 63, 321, 1500]
  lens = torch.tensor(first, dtype=torch.int32, device="cuda")
  call = lambda: ffpa_attn_with_kvcache_softcap(t0["q"], t0["k_cache"], t0["v_cache"], cache_seqlens=lens, block_table=t0["table"], softcap=cap, window_size=window,
                                                return_softmax_lse=True)
  call()  # (warm: the library is loaded, the scratch is sized)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out_g, lse_g = call()
  for now in (first, new):
    lens.copy_(torch.tensor(now, dtype=torch.int32, device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    eager = call()
    assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1])
    R.check(out_g, lse_g, S.attend(t0["q"], t0["k_cache"], t0["v_cache"], now, t0["table"], window, False, softcap=cap), v=vstat, dtype="bf16",
            name=f"graph replay on lengths {now}", extra=_extra(cap, vstat))
