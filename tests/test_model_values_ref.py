"""tests/model_values.py without a GPU: on every case tests/test_fwd_model_values_gpu.py and tests/test_fwd_split_d_gpu.py run (the short-query cases included), (1) the C oracle — the kernels' arithmetic on the CPU, blocked
by the tile the launch plan picks — stays inside ``kvcache_ref.allowance`` of the float64 reference with no element left out, so a failure of a kernel on
the GPU is a finding about the kernel, not about the inputs; (2) every family has the property its docstring promises; (3) the float64 reference is
``torch`` SDPA in float64; (4) ``kvcache_ref.check`` rejects the mistakes these inputs exist to catch; (5) every short-query case has the property it is there for at the first seed that gives it."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kvcache_ref as kr
import model_values as mv
from oracle import ffpa_oracle as fo


@pytest.fixture(scope="module")
def hip():
  from ffpa_attn_amd import hip as h

  h.load_library()
  return h


def _plan(hip, case, bias):
  B, hq, hkv, nq, nkv, d = case["shape"]
  return hip.launch_plan(B, hq, hkv, nq, nkv, d, dtype=case["dtype"], causal=case["causal"], bias_dtype=None if bias is None else bias.dtype)


def _oracle(q, k, v, bias, causal, block_keys, threshold=mv.RESCALE_THRESHOLD):
  """The C oracle's 16-bit output ``[B, Hq, Nq, D]`` and LSE as torch tensors."""
  qb, dt = fo.torch_to_bits(q)
  kb, _ = fo.torch_to_bits(k)
  vb, _ = fo.torch_to_bits(v)
  b = None
  if bias is not None:
    b = bias.float().numpy()  # (a 16-bit mask widens exactly: the kernels read the same values)
    b = np.broadcast_to(b, (b.shape[0], b.shape[1], q.size(2), k.size(2))) if b.shape[2] == 1 else b
  with np.errstate(all="ignore"):
    o, _, lse = fo.oracle_forward(qb, kb, vb, dt, causal=causal, bias=b, block_keys=block_keys, threshold=threshold)
  out = torch.from_numpy(o.view(np.int16).copy()).view(q.dtype)
  return out, torch.from_numpy(lse)


@pytest.mark.parametrize("D", mv.HEAD_DIMS + mv.SMALL_HEAD_DIMS)
@pytest.mark.parametrize("variant", list(mv.VARIANTS))
def test_the_oracle_alone_stays_inside_the_allowance_on_every_case(hip, variant, D):
  worst, worst_masked = 0.0, 0.0
  for case in mv.dense_cases(variant, D):
    probe = mv.build(case)[3]
    plan = _plan(hip, case, probe)
    q, k, v, bias, rows, value = mv.build(case, plan["block_keys"])
    ref = mv.attend(q, k, v, bias, case["causal"], fp32_rows=rows)
    out, lse = _oracle(q, k, v, bias, case["causal"], plan["block_keys"])
    name = f"{variant} {case['shape']} {kr.DTYPE_NAME[case['dtype']]} causal={case['causal']} [{plan['kernel']}]"
    worst = max(worst, mv.check_case(out, lse, ref, case, v=v, value=value, name=name))
    if rows is not None and value >= mv.BIAS_FLOOR:  # what the wholly masked rows need of their margin (profiles/r11_model_values.md)
      worst_masked = max(worst_masked, mv.masked_rows_need(out, ref, case, v=v, value=value))
  print(f"{variant} D={D}: worst error / allowance {worst:.3f}" + (f"; wholly masked rows need {worst_masked:.3f} of their margin" if worst_masked else ""))


@pytest.mark.parametrize("D", mv.SMALL_HEAD_DIMS)
@pytest.mark.parametrize("variant", mv.SPLIT_VARIANTS)
def test_the_oracle_alone_stays_inside_the_allowance_on_every_split_case(hip, variant, D):
  """The (129, 3100) cases the head dims <= 64 run with the KV axis cut into 3 ranges: the oracle in one walk over the plan's tiles."""
  worst = 0.0
  for case in mv.split_cases(variant, D):
    plan = _plan(hip, case, None)
    assert plan["block_keys"] == 128 and -(-case["shape"][4] // 128) // 8 == 3, plan  # (ffpa_capi.hip clamp_splits: at least 8 tiles per range of a prefill launch)
    q, k, v, bias, rows, value = mv.build(case, plan["block_keys"])
    ref = mv.attend(q, k, v, bias, case["causal"])
    out, lse = _oracle(q, k, v, bias, case["causal"], plan["block_keys"])
    name = f"{variant} {case['shape']} {kr.DTYPE_NAME[case['dtype']]} causal={case['causal']} [{plan['kernel']}]"
    worst = max(worst, mv.check_case(out, lse, ref, case, v=v, name=name))
  print(f"3 KV ranges {variant} D={D}: worst error / allowance {worst:.3f}")


@pytest.mark.parametrize("nq", (1, 7))
@pytest.mark.parametrize("D", mv.SHORT_QUERY_HEAD_DIMS)
@pytest.mark.parametrize("variant", mv.SHORT_QUERY_VARIANTS)
def test_the_oracle_alone_stays_inside_the_allowance_on_every_short_query_case(hip, variant, D, nq):
  """The short-query cases: each has the property it is there for (``assert_short_query_property``, at the seed the case carries — the FIRST from its base
  at which it holds), was built for the tile the plan picks, and the C oracle, blocked by that tile in one walk, stays inside the allowance."""
  worst, figs = 0.0, []
  for case in (c for c in mv.short_query_cases(variant, D) if c["shape"][3] == nq):
    plan = _plan(hip, case, None)
    assert plan["variant"] == 1 and plan["block_keys"] == case["block_keys"] == mv.SHORT_QUERY_TILES[D][1], (plan, case)
    q, k, v, bias, _, _ = mv.build(case, plan["block_keys"])
    fig = mv.assert_short_query_property(case, q, k, bias)
    B, hq, hkv, nq, nkv, d = case["shape"]
    base = 77 + nq + hq
    for seed in range(base, case["first_seed"]):  # (a case that does not hold at its base: no earlier seed does either)
      early = dict(case, seed=seed)
      qe, ke = mv.build(early, plan["block_keys"])[:2]
      assert not mv.short_query_property_holds(early, mv.short_query_property(early, qe, ke)), (variant, case["shape"], seed)
    ref = mv.attend_each_batch(q, k, v, bias, case["causal"])
    out, lse = _oracle(q, k, v, bias, case["causal"], plan["block_keys"])
    name = f"{variant} {case['shape']} {kr.DTYPE_NAME[case['dtype']]} seed {case['seed']} [{plan['kernel']}]"
    worst = max(worst, mv.check_case(out, lse, ref, case, v=v, name=name))
    figs.append(f"Nq {nq} heads {hq}/{hkv} {kr.DTYPE_NAME[case['dtype']]} seed {case['seed']}: {fig['sink rows']} sink rows of {fig['rows']}, mean pmax {fig['mean pmax']:.2f}")
  print(f"short query {variant} D={D} Nq={nq}: worst error / allowance {worst:.3f}\n  " + "\n  ".join(figs))


def _mean_pmax(ref, visible=None):
  p = ref[2]
  return float(p.mean()) if visible is None else float(p[visible].mean())


@pytest.mark.parametrize("D", mv.HEAD_DIMS + mv.SMALL_HEAD_DIMS)
def test_families_have_the_properties_they_state(D):
  for nq, nkv in mv.SEQ_SHAPES + mv.BIAS_SEQ_SHAPES:
    for dtype in mv.DTYPES:
      shape = (1, 4, 1, nq, nkv, D)
      scale = D ** -0.5
      # randn, for contrast: flat rows
      flat = _mean_pmax(mv.attend(*mv.plain(shape, dtype, 3)))
      assert flat < 0.08, flat
      # outliers: |v| >= 100 on the outlier channel alone
      q, k, v = mv.outliers(shape, dtype, 3)
      assert v.float().abs().max() >= 100.0 and v.float()[..., mv.V_OUTLIER_CHANNEL].abs().max() == v.float().abs().max()
      assert _mean_pmax(mv.attend(q, k, v)) >= 0.4
      # sink: some rows put their mass on key 0, others never see it; its V row is small
      q, k, v = mv.sink(shape, dtype, 3)
      p0 = torch.softmax(mv.scores(q, k), dim=-1)[..., 0]
      assert float((p0 >= 0.5).double().mean()) >= 0.04, float((p0 >= 0.5).double().mean())
      assert _mean_pmax(mv.attend(q, k, v)) >= 0.4
      assert float((p0 <= 1e-6).double().mean()) >= 0.25  # ... and the rows whose outlier channels point the other way never see it
      assert k[:, :, 0].float().abs().sum() == 2 * mv.SINK_VALUE and v[:, :, 0].float().abs().max() <= 0.05 * 40 * 6
      # peaked
      assert _mean_pmax(mv.attend(*mv.peaked(shape, dtype, 3))) >= 0.5
      # large logits
      q, k, v = mv.large_logits(shape, dtype, 3)
      s = mv.scores(q, k)
      assert 55.0 <= float(s.abs().max()) <= 140.0, float(s.abs().max())
      assert float(mv.attend(q, k, v)[1].abs().max()) >= 40.0  # (the LSE is compared at that magnitude)
      # staircases: the row maximum of consecutive KV tiles differs by the step, in log2 units
      for bc in {40: (64, 128), 64: (64, 128), 128: (64,), 320: (64, 128), 512: (64,), 1024: (32, 64)}[D]:  # (the KV tiles the launches of this head dim use)
        for step in mv.STAIR_STEPS:
          for up in (True, False):
            q, k, v = (mv.staircase_up if up else mv.staircase_down)(shape, dtype, 3, block_keys=bc, step=step)
            s2 = mv.scores(q, k) * mv.LOG2E
            tiles = -(-nkv // bc)
            tmax = torch.stack([s2[..., t * bc:(t + 1) * bc].amax(dim=-1) for t in range(tiles)], dim=-1)
            diff = (tmax[..., 1:] - tmax[..., :-1]) * (1 if up else -1)
            assert float((diff - step).abs().max()) <= 0.25, (bc, step, up, float((diff - step).abs().max()))
            assert bool(((diff > mv.RESCALE_THRESHOLD) == (step > mv.RESCALE_THRESHOLD)).all())
      # alibi
      for bdt in (torch.float32, dtype):
        _, _, _, bias = mv.alibi(shape, dtype, 3, bias_dtype=bdt)
        assert bias.shape == (1, 4, nq, nkv) and bias.dtype == bdt
        i = torch.arange(nq)
        assert bool((bias[0, :, i, i + (nkv - nq)] == 0).all())
        assert float(bias.float().min()) == float(torch.tensor(-(2.0 ** -2.0) * (nkv - 1)).to(bdt).float())
      # hf_mask: rows [0, 5) of batch 1 are the wholly masked ones, and only they
      for kind in mv.MASK_VALUES:
        shape2 = (2,) + shape[1:]
        q, k, v, bias = mv.hf_mask(shape2, dtype, 3, kind=kind)
        value, mdt = mv.mask_value(kind, dtype)
        assert bias.dtype == mdt and bias.shape == (2, 1, nq, nkv)
        whole = (bias.float() == float(torch.tensor(value).to(mdt).float())).all(dim=-1)[:, 0]
        assert torch.equal(whole, mv.wholly_masked_rows(shape2))
        assert bool((bias[1, 0, mv.MASKED_ROWS:, :mv.padded_keys(nkv)].float() == bias[1, 0, 0, 0].float()).all()) and bool((bias[0] == 0).all())
        assert bool((bias[1, 0, mv.MASKED_ROWS:, mv.padded_keys(nkv):] == 0).all())


@pytest.mark.parametrize("variant", ["sink", "peaked", "large_logits", "staircase_down_8.5", "hf_mask_neg_inf", "hf_mask_finfo_min", "hf_mask_finfo_min_fp32",
                                     "hf_mask_minus_1e4", "alibi_fp32", "alibi_16bit"])
def test_the_float64_reference_is_sdpa_in_float64(variant):
  for D in (128, 320):
    for case in mv.dense_cases(variant, D)[:8]:
      q, k, v, bias, rows, value = mv.build(case)
      o, lse, _, _ = mv.attend(q, k, v, bias, case["causal"])  # (no fp32 rows: float64 against float64)
      B, hq, hkv, nq, nkv, d = case["shape"]
      mask = None if bias is None else bias.double()
      if case["causal"]:  # tail aligned: as an explicit mask (SDPA's is_causal is top-left aligned)
        mask = torch.zeros((nq, nkv), dtype=torch.float64).masked_fill(~mv.causal_mask(nq, nkv), float("-inf"))
      g = hq // hkv
      want = F.scaled_dot_product_attention(q.double(), k.double().repeat_interleave(g, dim=1), v.double().repeat_interleave(g, dim=1), attn_mask=mask)
      want = want.transpose(1, 2)
      dead = torch.isneginf(lse).transpose(1, 2)  # rows without a visible key: NaN or 0 in SDPA (its backends differ), 0 here (``kvcache_ref.check``'s contract)
      assert bool((o[dead] == 0).all()) and int(dead.sum()) == (mv.MASKED_ROWS * hq if variant == "hf_mask_neg_inf" else 0)
      if value is not None and np.isfinite(value) and value < mv.BIAS_FLOOR:
        # float64 does not absorb q.k into finfo(float32).min the way fp32 does: the wholly masked rows are compared on the fp32 grid, where SDPA's own
        # float32 math path is the statement of the contract
        want32 = F.scaled_dot_product_attention(q.float(), k.float().repeat_interleave(g, dim=1), v.float().repeat_interleave(g, dim=1), attn_mask=bias.float())
        o32 = mv.attend(q, k, v, bias, False, fp32_rows=mv.wholly_masked_rows(case["shape"]))[0]
        r = mv.wholly_masked_rows(case["shape"])
        torch.testing.assert_close(o32[r], want32.transpose(1, 2).double()[r], atol=2e-6, rtol=1e-5)
        torch.testing.assert_close(o32[r], v.double().mean(dim=2)[1].repeat_interleave(g, dim=0)[None].expand(mv.MASKED_ROWS, -1, -1), atol=1e-12, rtol=0)
      torch.testing.assert_close(o[~dead], want[~dead], atol=1e-12, rtol=1e-10)


def _rejected(out, lse, ref, case, **kw) -> bool:
  try:
    mv.check_case(out, lse, ref, case, **kw)
  except AssertionError:
    return True
  return False


@pytest.mark.parametrize("dtype", mv.DTYPES)
def test_check_rejects_the_mistakes_these_inputs_exist_to_catch(hip, dtype):
  D, nq, nkv = 512, 64, 700
  shape = (1, 2, 2, nq, nkv, D)
  case = {"shape": shape, "dtype": dtype, "causal": False, "family": "sink", "knobs": {}, "seed": 5, "variant": "sink"}
  as_out = lambda ref: ref[0].transpose(1, 2).to(dtype)  # a float64 result as a kernel would hand it over: [B, Hq, Nq, D], 16 bits
  # (0) the honest result passes
  q, k, v = mv.sink(shape, dtype, 5)
  ref = mv.attend(q, k, v)
  assert not _rejected(as_out(ref), ref[1].float(), ref, case, v=v, value=None)
  # (1) the sink key dropped
  wrong = mv.attend(q, k[:, :, 1:], v[:, :, 1:])
  assert _rejected(as_out(wrong), None, ref, case, v=v, value=None)
  # (2) the V outlier channel taken from the neighbouring key
  v2 = v.clone()
  v2[..., mv.V_OUTLIER_CHANNEL] = torch.roll(v[..., mv.V_OUTLIER_CHANNEL], 1, dims=2)
  assert _rejected(as_out(mv.attend(q, k, v2)), None, ref, case, v=v, value=None)
  # (3) the row maximum frozen after the first tile: the C oracle with a threshold that never fires again.  fp16: P outgrows 65504 on the third tile of a
  # rising staircase; bf16 has fp32's exponent range — a frozen maximum is harmless until 2^128, which twelve tiles of 16 log2 units pass
  step = 8.5 if dtype == torch.float16 else 16.0
  bc = _plan(hip, case, None)["block_keys"]
  case_s = dict(case, family="staircase_up", knobs={"step": step})
  q, k, v = mv.staircase_up(shape, dtype, 5, block_keys=bc, step=step)
  ref = mv.attend(q, k, v)
  out, lse = _oracle(q, k, v, None, False, bc)
  assert not _rejected(out, lse, ref, case_s, v=v, value=None)
  out, lse = _oracle(q, k, v, None, False, bc, threshold=3e38)
  assert _rejected(out, lse, ref, case_s, v=v, value=None)
  # (4) finfo.min turned into -inf
  shape2 = (2,) + shape[1:]
  for kind in ("finfo_min", "finfo_min_fp32"):
    case_m = dict(case, shape=shape2, family="hf_mask", knobs={"kind": kind})
    q, k, v, bias, rows, value = mv.build(case_m)
    ref = mv.attend(q, k, v, bias, fp32_rows=rows)
    assert not _rejected(as_out(ref), ref[1].float(), ref, case_m, v=v, value=value)
    hidden = torch.where(bias.float() < -1e4, torch.full_like(bias.float(), float("-inf")), bias.float())
    wrong = mv.attend(q, k, v, hidden)
    nan_rows = mv.wholly_masked_rows(shape2)
    out = as_out(wrong)
    assert _rejected(out, None, ref, case_m, v=v, value=value)      # 0 in the rows the float64 restatement leaves without a key
    out[nan_rows[:, None, :].expand(-1, 2, -1)] = float("nan")      # ... NaN as the kernels leave them
    assert _rejected(out, None, ref, case_m, v=v, value=value)


def _as_out(o, dtype):
  """A float64 result ``[B, Nq, Hq, D]`` as a kernel would hand it over: ``[B, Hq, Nq, D]``, 16 bits."""
  return o.transpose(1, 2).to(dtype)


def _two_range_merge_against_range_0(q, k, v):
  """Float64 attention as a two-range KV split computes it — each range normalised against its OWN row maximum m_i, with row sum l_i, the merge weighing
  range i by l_i exp(m_i - M) — but with range 0's maximum in BOTH weights: l_i exp(m_0 - M), that is, l_i alone.  -> ``[B, Nq, Hq, D]``."""
  outs = []
  for b in range(q.size(0)):
    s = mv.scores(q[b:b + 1], k[b:b + 1])
    vv = v[b:b + 1].double().repeat_interleave(q.size(1) // k.size(1), dim=1)
    half = k.size(2) // 2
    o, w = [], []
    for lo, hi in ((0, half), (half, k.size(2))):
      e = torch.exp(s[..., lo:hi] - s[..., lo:hi].amax(dim=-1, keepdim=True))
      l = e.sum(dim=-1, keepdim=True)
      o.append(torch.matmul(e / l, vv[:, :, lo:hi]))
      w.append(l)
    outs.append(((w[0] * o[0] + w[1] * o[1]) / (w[0] + w[1])).transpose(1, 2))
  return torch.cat(outs)


@pytest.mark.parametrize("nq", (1, 7))
@pytest.mark.parametrize("D", mv.SHORT_QUERY_HEAD_DIMS)
@pytest.mark.parametrize("variant", ("sink", "staircase_up_8.5", "large_logits"))
def test_check_rejects_the_mistakes_the_short_query_cases_exist_to_catch(variant, D, nq):
  """What a KV-split launch can get wrong that one walk cannot, on EVERY short-query case of the variant: (sink) key 0 — the first range's weight — lost;
  (staircase_up_8.5) the last range of a 4-way split — the staircase's top — lost; (large_logits) a merge whose weights never see the second range's
  maximum.  The honest float64 result passes, each mistake is rejected."""
  for case in (c for c in mv.short_query_cases(variant, D) if c["shape"][3] == nq):
    bc = case["block_keys"]
    q, k, v = mv.build(case, bc)[:3]
    ref = mv.attend_each_batch(q, k, v)
    kw = dict(v=v, value=None, name=f"{variant} {case['shape']}")
    assert not _rejected(_as_out(ref[0], case["dtype"]), ref[1].float(), ref, case, **kw)
    if variant == "sink":
      wrong = mv.attend_each_batch(q, k[:, :, 1:], v[:, :, 1:])[0]
    elif variant == "staircase_up_8.5":
      tiles = -(-k.size(2) // bc)
      cut = 3 * -(-tiles // 4) * bc  # (ffpa_capi.hip make_plan: ranges of ceil(tiles / splits) tiles)
      assert 0 < cut < k.size(2)
      wrong = mv.attend_each_batch(q, k[:, :, :cut], v[:, :, :cut])[0]
    else:
      wrong = _two_range_merge_against_range_0(q, k, v)
    assert _rejected(_as_out(wrong, case["dtype"]), None, ref, case, **kw), (variant, case["shape"], case["dtype"])
