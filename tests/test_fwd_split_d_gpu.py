"""Every build of ``ffpa_fwd_split_d_kernel`` (csrc/ffpa_fwd_kernel.h: the 32x32x16 mapping) against float64 on the values models produce (tests/model_values.py):

* the short-query tiles — head dim over 2 or 4 waves x 32 or 64 keys per tile, one head dim for each of the four shapes twice over
  (``model_values.SHORT_QUERY_TILES``) — in the plan's own split count, split into 4 and unsplit, plain and tail-aligned causal, GQA heads packed into rows, the
  merge kernel and the in-launch merge, under padding masks and key bias; every case asserts the property it is there for on the rows it computes
  (``model_values.assert_short_query_property``);
* prefill at head dims <= 64 (``model_values.SMALL_HEAD_DIMS``; 40 runs the 64 build with columns that are not there): the whole grid of variants, the
  LDS-staged 16-bit bias tiles (``BTILE``), key bias, boolean masks, a KV split + merge;
* the keep decisions of the three ``DROP`` builds, whole tensors against ``ffpa_attn_amd.philox``.

Every comparison goes through ``model_values.check_case`` -> ``kvcache_ref.check``: the allowance tests/test_model_values_ref.py shows the C oracle to stay inside on
the same inputs.  The kernel each launch ran is asserted by the name the launch reports."""

import math

import numpy as np
import pytest
import torch

import kvcache_ref as kr
import model_values as mv
from backward_dense_ref import element_index
from test_backward_dense_family_gpu import KEEP_OFFSET, KEEP_SEED
from test_fwd_model_values_gpu import REACHED, _bool_builder, _dense, _family, _key_padding_builder, _short_query_launches

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def hip():
  if not torch.cuda.is_available():
    pytest.fail("these tests need a GPU; run with -m 'not gpu' on CPU boxes")
  from ffpa_attn_amd import hip as h

  h.load_library()  # fail loudly if the extension is missing: there is no fallback
  return h


# ----------------------------------------------------------------------------- short-query tiles
@pytest.mark.parametrize("nq", (1, 7))
@pytest.mark.parametrize("D", mv.SHORT_QUERY_HEAD_DIMS)
@pytest.mark.parametrize("variant", mv.SHORT_QUERY_VARIANTS)
def test_short_query_launches_on_model_values(hip, variant, D, nq):
  """Each case once through ``check_case`` per launch form: the plan's own split count, 4 KV ranges, none; at Nq = 7 tail-aligned causal too.  On the
  staircase the in-launch merge returns the merge kernel's bits."""
  forms = [(0, False), (4, False), (1, False)] + ([(0, True), (4, True), (1, True)] if nq == 7 else [])
  worst = 0.0
  for case in mv.short_query_cases(variant, D):
    if case["shape"][3] != nq:
      continue
    ratio, fig, plans = _short_query_launches(hip, case, forms, equal_in_launch_merge=variant == "staircase_up_8.5")
    worst = max(worst, ratio)
    print(f"short query {variant} D={D} Nq={nq} heads {case['shape'][1]}/{case['shape'][2]} {kr.DTYPE_NAME[case['dtype']]} seed {case['seed']}: "
          f"{fig['sink rows']} sink rows of {fig['rows']}, mean pmax {fig['mean pmax']:.2f}, top |s| {fig['top |s|']:.0f}; error / allowance {ratio:.3f} "
          f"[{plans[1]['kernel']}; splits {[p['splits'] for p in plans]}]")
  print(f"short query {variant} D={D} Nq={nq}: worst error / allowance {worst:.3f}")


def _dense_on(hip, case, family: str, **kw):
  """``_dense`` -> (worst error / allowance, plan), the launch asserted to have run the kernel family ``family`` (as ``_family`` names it)."""
  seen = {}
  ratio = _dense(hip, case, seen=seen, **kw)
  assert family in _family(seen["kernel"]), (family, seen)
  return ratio, seen


@pytest.mark.parametrize("D", (320, 576))
@pytest.mark.parametrize("kind", ("neg_inf", "finfo_min", "finfo_min_fp32", "minus_1e9"))
def test_two_wave_short_query_tiles_under_padding_masks(hip, kind, D):
  """tests/test_fwd_model_values_gpu.py ``test_short_query_split_kv_under_padding_masks`` on the tiles that split the head dim over TWO waves (64 and 32 keys):
  seven query rows against 2000 keys under ``hf_mask`` and under the same values as a key bias, the KV axis split by the plan and into 4."""
  worst = 0.0
  for hq, hkv in mv.HEADS:
    for dtype in mv.DTYPES:
      if float(mv.mask_value(kind, dtype)[0]) >= mv.BIAS_FLOOR:
        continue  # (finfo(fp16).min: not saturated — the rows-masked-wholly tests)
      for splits in (0, 4):
        case = {"variant": f"hf_mask_{kind}", "family": "hf_mask", "knobs": {"kind": kind}, "shape": (2, hq, hkv, 7, 2000, D), "dtype": dtype, "causal": False,
                "seed": 300 + hq}
        for builder in (None,) + ((_key_padding_builder,) if kind != "neg_inf" else ()):
          ratio, plan = _dense_on(hip, case, "ffpa_fwd_split_d_kernel ND=2", builder=builder, num_splits=splits)
          assert plan["block_keys"] == mv.SHORT_QUERY_TILES[D][1] and (splits == 0 or (plan["splits"] > 1 and "ffpa_fwd_merge_kernel" in plan["kernel"])), plan
          worst = max(worst, ratio)
  print(f"short query {kind} D={D}: worst error / allowance {worst:.3f}")


# ----------------------------------------------------------------------------- prefill at head dims <= 64
def _small_family(case) -> str:
  """The build a prefill case of SMALL_HEAD_DIMS must run: ND = 1, with staged bias tiles where a 16-bit bias with a row axis has 16-byte aligned rows."""
  _, _, has_bias = mv.VARIANTS[case["variant"]]
  staged = has_bias and case["shape"][4] % 8 == 0 and mv.build(case)[3].dtype == case["dtype"]
  return "ffpa_fwd_split_d_kernel ND=1" + (" BTILE" if staged else "")


@pytest.mark.parametrize("D", mv.SMALL_HEAD_DIMS)
@pytest.mark.parametrize("variant", list(mv.VARIANTS))
def test_small_head_dim_prefill_on_model_values(hip, variant, D):
  worst, staged = 0.0, 0
  for case in mv.dense_cases(variant, D):
    family = _small_family(case)
    ratio, plan = _dense_on(hip, case, family)
    assert f", 64, ND=1" in plan["kernel"] and plan["splits"] == 1, plan
    staged += family.endswith("BTILE")
    worst = max(worst, ratio)
  if variant == "alibi_16bit":
    assert staged == len(mv.BIAS_SEQ_SHAPES) * len(mv.HEADS) * len(mv.DTYPES)  # (every (129, 520) case, and no other)
  print(f"small head dim {variant} D={D}: worst error / allowance {worst:.3f} ({staged} cases through staged bias tiles)")


@pytest.mark.parametrize("D", mv.HEAD_DIMS)
def test_staged_bias_tiles_of_the_large_head_dims(hip, D):
  """The (129, 520) ALiBi cases in 16 bits at the head dims of the 16x16x32 kernel, whose name carries no tag for the placement of the bias."""
  cases = [c for c in mv.dense_cases("alibi_16bit", D) if (c["shape"][3], c["shape"][4]) in mv.BIAS_SEQ_SHAPES]
  assert len(cases) == len(mv.HEADS) * len(mv.DTYPES)
  print(f"alibi_16bit (129, 520) D={D}: worst error / allowance {max(_dense(hip, c) for c in cases):.3f}")


@pytest.mark.parametrize("D", mv.SMALL_HEAD_DIMS)
def test_small_head_dim_key_bias_bool_masks_and_a_kv_split(hip, D):
  """Head dims <= 64 under a padding mask without a row axis (every finite mask value), under a boolean mask, and — an under-filled launch — with the KV axis
  split into 3 and merged."""
  worst = 0.0
  for kind in mv.MASK_VALUES[1:]:  # (a sequence that is -inf throughout has no key for the launch to walk)
    for case in mv.dense_cases(f"hf_mask_{kind}", D):
      worst = max(worst, _dense_on(hip, case, "ffpa_fwd_split_d_kernel ND=1", builder=_key_padding_builder)[0])
  for case in mv.dense_cases("hf_mask_neg_inf", D):
    worst = max(worst, _dense_on(hip, case, "ffpa_fwd_split_d_kernel ND=1", builder=_bool_builder)[0])
  for variant in mv.SPLIT_VARIANTS:
    for case in mv.split_cases(variant, D):  # (3100 keys: a range of a prefill launch holds at least 8 tiles of 128)
      ratio, plan = _dense_on(hip, case, "ffpa_fwd_split_d_kernel ND=1", num_splits=3)
      assert plan["splits"] == 3 and "ffpa_fwd_merge_kernel" in plan["kernel"], plan
      worst = max(worst, ratio)
  print(f"small head dim key bias / bool / 3 KV ranges D={D}: worst error / allowance {worst:.3f}")


def _small_absorbed_cases():
  """``test_fwd_model_values_gpu._absorbed_cases`` at SMALL_HEAD_DIMS: the mask as given and as a key bias, one id per case."""
  out = []
  for route, builder in (("dense", None), ("keybias", _key_padding_builder)):
    for kind in ("minus_1e4", "finfo_min"):
      for D in mv.SMALL_HEAD_DIMS:
        for case in mv.dense_cases(f"hf_mask_{kind}", D):
          if kind == "minus_1e4" or case["dtype"] == torch.float16:
            _, hq, hkv, nq, nkv, _ = case["shape"]
            cid = f"{route}-{kind}-D{D}-{nq}x{nkv}-h{hq}_{hkv}-{kr.DTYPE_NAME[case['dtype']]}"
            marks = [pytest.mark.xfail(strict=True, reason=SMALL_ABSORBED_MISS)] if cid in SMALL_ABSORBED_MISSES else []
            out.append(pytest.param(case, builder, id=cid, marks=marks))
  return out


SMALL_ABSORBED_MISS = "measured to miss allowance + margin on an MI355X (profiles/r34_split_d_model_values.md)"
SMALL_ABSORBED_MISSES = frozenset(())


@pytest.mark.parametrize("case,builder", _small_absorbed_cases())
def test_small_head_dim_rows_masked_wholly_by_a_large_finite_value(hip, case, builder):
  """``test_rows_masked_wholly_by_a_large_finite_value`` of tests/test_fwd_model_values_gpu.py for the ND = 1 builds: a row whose every key carries -1e4 or
  finfo(fp16).min against the float64 softmax of the fp32-rounded sums, within the allowance + ``model_values.absorbed_margin``."""
  ratio = _dense(hip, case, builder=builder, judge_absorbed_rows=True)
  print(f"absorbed rows: worst error / allowance {ratio:.3f}")


# ----------------------------------------------------------------------------- the keep masks of the DROP builds, exactly
# (D, Nq, Nkv, num_splits (0: the plan's), causal, the ND= tag, keys per tile)
KEEP_CASES = [
  (64, 130, 300, 0, False, 1, None),
  (320, 7, 777, 1, False, 2, 64), (320, 32, 777, 3, False, 2, 64), (320, 7, 777, 3, True, 2, 64),
  (576, 1, 1100, 0, False, 2, 32),
  (512, 7, 777, 1, False, 4, 64), (512, 7, 777, 3, False, 4, 64),
  (1024, 20, 1024, 0, False, 4, 32),
]
KEEP_P = [0.1, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1.0)))]


def _kept_by_the_kernel(hip, D, nq, nkv, splits, causal, nd, bc, p):
  """bool ``[B, Hq, Nq, Nkv]`` at B 2, heads 4 / 2: the elements the launch kept.  q = 0 makes P uniform and positive over the keys a row sees; V is a shifted
  identity — in launch c of ceil(Nkv / D), V[j, j - c D] = 1 for the keys of chunk c and 0 elsewhere — so ``O_c[..., col] != 0`` exactly where the kernel kept
  key c D + col.  Every launch must be the ``ND=nd, DROP`` build on ``bc``-key tiles, split (or not) as asked."""
  B, hq, hkv = KEEP_SHAPE["B"], *KEEP_SHAPE["heads"]
  dtype = torch.bfloat16 if D in (64, 512, 576) else torch.float16
  g = torch.Generator(device="cuda").manual_seed(nkv + D + nq)
  q = torch.zeros(B, hq, nq, D, dtype=dtype, device="cuda")
  k = torch.randn(B, hkv, nkv, D, dtype=torch.float32, device="cuda", generator=g).to(dtype)
  kept = torch.zeros(B, hq, nq, nkv, dtype=torch.bool, device="cuda")
  for c in range(-(-nkv // D)):
    n = min(D, nkv - c * D)
    v = torch.zeros(B, hkv, nkv, D, dtype=dtype, device="cuda")
    v[:, :, c * D:c * D + n, :n] = torch.eye(n, dtype=dtype, device="cuda")
    plan = {}
    o, _ = hip.forward(q, k, v, None, causal, D ** -0.5, dropout_p=p, philox_seed=KEEP_SEED, philox_offset=KEEP_OFFSET, num_splits=splits, plan_out=plan)
    assert f", {D}, ND={nd}, DROP>" in plan["kernel"] and plan["variant"] == (0 if nd == 1 else 1) and not plan["packed"], plan
    assert (bc is None or plan["block_keys"] == bc) and (splits == 0 or (plan["splits"] > 1) == (splits > 1)), plan
    REACHED.update(_family(plan["kernel"]))
    assert o.shape == (B, hq, nq, D) and bool(torch.isfinite(o).all()) and bool((o >= 0).all()) and bool((o[..., n:] == 0).all())
    kept[..., c * D:c * D + n] = o[..., :n] != 0
  return kept, plan


KEEP_SHAPE = {"B": 2, "heads": (4, 2)}


@pytest.mark.parametrize("p", KEEP_P, ids=["p0.1", "p0.5", "p0.5+ulp"])
@pytest.mark.parametrize("D, nq, nkv, splits, causal, nd, bc", KEEP_CASES, ids=[f"D{c[0]}-Nq{c[1]}-Nkv{c[2]}-splits{c[3]}" + ("-causal" if c[4] else "") for c in KEEP_CASES])
def test_the_drop_builds_keep_exactly_the_elements_philox_py_says(hip, D, nq, nkv, splits, causal, nd, bc, p):
  """tests/test_backward_dense_family_gpu.py ``test_the_kernel_keeps_exactly_the_elements_philox_py_says`` for the split-D builds: the assembled boolean
  tensor (``_kept_by_the_kernel``), whole, against ``dropout_keep_mask`` (and the causal mask) — the statement a change to these builds' dropout is checked
  against, KV ranges and their merge included."""
  from ffpa_attn_amd.philox import dropout_keep_mask

  kept, plan = _kept_by_the_kernel(hip, D, nq, nkv, splits, causal, nd, bc, p)
  want = dropout_keep_mask(KEEP_SEED, KEEP_OFFSET, element_index(dict(KEEP_SHAPE, Nq=nq, Nkv=nkv), "cuda"), p)
  share = want.double().mean().item()
  assert abs(share - (1.0 - p)) <= 4.0 * math.sqrt(p * (1.0 - p) / want.numel()), (share, p, want.numel())  # the kept share within four binomial standard deviations
  if causal:
    want = want & mv.causal_mask(nq, nkv, "cuda")
  wrong = int((kept != want).sum())
  assert torch.equal(kept, want), f"{wrong} of {want.numel()} keep decisions differ [{plan['kernel']}, splits {plan['splits']}]"


@pytest.mark.parametrize("D, nq, nkv, splits, causal, nd, bc", [c for c in KEEP_CASES if c[3] == 3 and not c[4]], ids=lambda x: str(x))
def test_a_word_that_equals_the_keep_threshold_is_kept(hip, D, nq, nkv, splits, causal, nd, bc):
  """The kernels keep the element of Philox word w when w >= T, T the smallest word with u(w) = (float(w) + 1) 2^-32 > p.  No p of the test above has a T
  that a launch of a few 10^5 elements draws: `>` for `>=` would pass it.  Here p is made for the launch: u steps once per 256 words of the top binade, so
  about one drawn word in 256 is the first of its step — take one with u in (0.3, 0.7) and the fp32 number just below its u as p.  Then T is that word,
  the element that drew it is kept, and the whole tensor still is ``dropout_keep_mask``."""
  from ffpa_attn_amd.philox import dropout_keep_mask, philox4x32_10

  idx = element_index(dict(KEEP_SHAPE, Nq=nq, Nkv=nkv), "cuda")
  e = idx + KEEP_OFFSET
  w4 = philox4x32_10(KEEP_SEED, e >> 2)
  lane = e & 3
  word = torch.where(lane == 0, w4[0], torch.where(lane == 1, w4[1], torch.where(lane == 2, w4[2], w4[3])))
  u = lambda w: (w.to(torch.float32) + 1.0) * 2.3283064365386963e-10
  first = (u(word) > u(word - 1)) & (u(word) > 0.3) & (u(word) < 0.7)
  assert int(first.sum()) > 0
  at = tuple(int(i) for i in first.nonzero()[0])
  p = float(np.nextafter(np.float32(u(word[at]).item()), np.float32(0.0)))
  want = dropout_keep_mask(KEEP_SEED, KEEP_OFFSET, idx, p)
  assert bool(want[at]) and not bool((u(word[at] - 1) > p).item())  # T is this word
  kept, plan = _kept_by_the_kernel(hip, D, nq, nkv, splits, causal, nd, bc, p)
  assert bool(kept[at]), f"p = {p!r}: the element {at} drew the threshold word {int(word[at])} and was dropped [{plan['kernel']}]"
  assert torch.equal(kept, want), f"{int((kept != want).sum())} of {want.numel()} keep decisions differ [{plan['kernel']}]"
