"""Seeded inputs with the statistics attention sees inside a model — outlier channels, an attention sink, peaked rows, a row maximum that climbs or falls from
one KV tile to the next, logits near +-90, padding masks filled with finfo.min, ALiBi — where every other forward test of the suite draws q, k, v from randn
(logits ~ N(0, 1): a flat softmax, a running maximum that barely moves, |v| < 5); the float64 restatement of the dense forward they are checked against
(``attend``: ``kvcache_ref.check`` takes its result); and the case lists of tests/test_model_values_ref.py (C oracle, no GPU) and
tests/test_fwd_model_values_gpu.py (the kernels).  Plain torch (any device) + numpy.  The families are defined here, from numbers: every constant below is
stated with what it is for, and tests/test_model_values_ref.py asserts the property each docstring promises.

A family is ``f(shape, dtype, seed, **knobs) -> (q, k, v[, bias])`` with ``shape = (B, Hq, Hkv, Nq, Nkv, D)``, q ``[B, Hq, Nq, D]``, k / v ``[B, Hkv, Nkv, D]``
of ``dtype`` (CPU tensors), bias broadcastable to ``[B, Hq, Nq, Nkv]``."""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

LOG2E = 1.4426950408889634
OUTLIER_CHANNELS = (3, -5)   # the same two channels in q and k, as the massive activations of a trained model sit in fixed channels
OUTLIER_SCALE = 12.0
V_OUTLIER_CHANNEL = 7
V_OUTLIER_SCALE = 40.0
SINK_VALUE = 30.0            # key 0 on the outlier channels
SINK_V_SCALE = 0.05
PEAK_SCALE = 2.5             # on q and k: logit std 6.25
LARGE_LOGIT_STD = 20.0       # large_logits: 4.5 sigma = 90 natural units; exp(90) = 1.2e39 > FLT_MAX
MASKED_ROWS = 5              # hf_mask: the first rows of the padded sequence see padding only
BIAS_FLOOR = -2.0 ** 21      # csrc/ffpa_common.h kBiasFloor: finite mask values below it enter the kernels as one saturated score
RESCALE_THRESHOLD = 8.0      # log2 units: the launch's lazy-rescale threshold
STAIR_STEPS = (7.5, 8.5, 16.0)  # just below / just above / twice the threshold


@functools.lru_cache(maxsize=3)
def _randn32(shape, seed: int):
  """The fp32 draw behind ``_randn``, kept for the last q, k and v: a case's bf16 and fp16 twins round the same draw, and the K / V of a short-query case are
  10^8 serial draws each.  Never handed out: ``_randn`` returns the 16-bit copy."""
  g = torch.Generator().manual_seed(seed)
  return torch.randn(shape, generator=g, dtype=torch.float32)


def _randn(shape, seed: int, dtype):
  return _randn32(tuple(shape), seed).to(dtype)


def plain(shape, dtype, seed):
  """randn: what the rest of the suite draws (logit std 1)."""
  B, hq, hkv, nq, nkv, d = shape
  return _randn((B, hq, nq, d), seed, dtype), _randn((B, hkv, nkv, d), seed + 1, dtype), _randn((B, hkv, nkv, d), seed + 2, dtype)


def outliers(shape, dtype, seed):
  """Channels OUTLIER_CHANNELS of q and k x 12, channel V_OUTLIER_CHANNEL of v x 40.  Guarantees (asserted): the largest |v| >= 100 and sits on that
  channel (40 x the largest of >= 333 normal draws), so one misplaced V element is tens of allowances; the two channels carry 2 x 144^2 of the
  D - 2 + 2 x 144^2 units of q.k variance: mean row pmax >= 0.4 (randn: 0.02)."""
  q, k, v = plain(shape, dtype, seed)
  q, k, v = q.float(), k.float(), v.float()
  for c in OUTLIER_CHANNELS:
    q[..., c] *= OUTLIER_SCALE
    k[..., c] *= OUTLIER_SCALE
  v[..., V_OUTLIER_CHANNEL] *= V_OUTLIER_SCALE
  return q.to(dtype), k.to(dtype), v.to(dtype)


def sink(shape, dtype, seed):
  """``outliers`` + an attention sink: key 0 is zero but for the outlier channels, which hold 30, and its V row is scaled by 0.05.  A query scores
  30 x (its two outlier channels, 12 N(0, 1) each) x scale on key 0: 45 N(0, 1) natural units at D = 128, 16 N(0, 1) at D = 1024 — against the largest of
  the other keys' outlier products, which is of the same size.  Guarantees (asserted): mean row pmax >= 0.4 (randn: 0.02), at least 4 % of the rows give
  key 0 p >= 0.5 and at least a quarter of them p <= 1e-6 (the rows whose outlier channels point away from it), and an output computed without key 0 is
  outside the allowance."""
  q, k, v = outliers(shape, dtype, seed)
  k, v = k.float(), v.float()
  k[:, :, 0, :] = 0.0
  for c in OUTLIER_CHANNELS:
    k[:, :, 0, c] = SINK_VALUE
  v[:, :, 0, :] *= SINK_V_SCALE
  return q, k.to(dtype), v.to(dtype)


def peaked(shape, dtype, seed):
  """q and k x 2.5: logits ~ N(0, 6.25^2).  Guarantees: mean row pmax >= 0.5 at every shape of the suite (the largest of a few hundred such logits leads the
  second by ~ 2 natural units; asserted), against ~ 0.02 for randn."""
  q, k, v = plain(shape, dtype, seed)
  return (q.float() * PEAK_SCALE).to(dtype), (k.float() * PEAK_SCALE).to(dtype), v


def _staircase(shape, dtype, seed, block_keys: int, step: float, up: bool, scale: "float | None" = None):
  B, hq, hkv, nq, nkv, d = shape
  scale = d ** -0.5 if scale is None else scale
  q, k, v = plain(shape, dtype, seed)
  q, k = q.float() * 0.125, k.float() * 0.125  # what is left of randn moves a tile's row max by < 0.1 log2 units (logit std 1 / 64)
  tiles = -(-nkv // block_keys)
  t = torch.arange(nkv) // block_keys
  level = (t if up else (tiles - 1 - t)).float()  # 0, 1, 2, ...: exact in 16 bits (at most a few dozen tiles)
  # logit of (row, key) in log2 units = q0 * level * scale * log2(e) + noise: q0 = step / (scale log2 e), rounded once to 16 bits (2^-9 relative: the step is
  # off by < 0.4 % — 7.5 and 8.5 stay on their side of 8)
  q[..., 0] = step / (scale * LOG2E)
  k[..., 0] = level[None, None, :]
  return q.to(dtype), k.to(dtype), v


def staircase_up(shape, dtype, seed, block_keys: int = 64, step: float = 8.5):
  """Keys ordered so that every row's maximum RISES by ``step`` log2 units from one ``block_keys``-wide KV tile to the next (to within 0.25: asserted): the
  lazy rescale fires (step > 8) or is skipped with p up to 2^step against the stale maximum (step < 8) on EVERY tile, not at four planted keys."""
  return _staircase(shape, dtype, seed, block_keys, step, True)


def staircase_down(shape, dtype, seed, block_keys: int = 64, step: float = 8.5):
  """As ``staircase_up`` with the maximum FALLING by ``step`` per tile: the first tile sets a maximum every later tile is tiny against (p = 2^-step, 2^-2 step,
  ... down to 0), so the row sum and O are built from entries many binades apart."""
  return _staircase(shape, dtype, seed, block_keys, step, False)


def large_logits(shape, dtype, seed):
  """q and k x sqrt(20): natural-unit logits ~ N(0, 20^2).  Guarantees: the largest |logit| lies in [55, 140] (asserted) — exp() of it without the max
  subtraction overflows or loses fp32, and |LSE| reaches the same magnitude, where its tolerance is relative."""
  q, k, v = plain(shape, dtype, seed)
  f = math.sqrt(LARGE_LOGIT_STD)
  return (q.float() * f).to(dtype), (k.float() * f).to(dtype), v


MASK_VALUES = ("neg_inf", "finfo_min", "finfo_min_fp32", "minus_1e4", "minus_1e9")


def mask_value(kind: str, dtype):
  """``(value, mask dtype)`` of a padding-mask fill: -inf, finfo(q.dtype).min in q's dtype, finfo(float32).min as an fp32 mask, -1e4, and the -1e9 of older
  model code (fp32 mask: 16-bit floats do not hold it... bf16 does, fp16 does not)."""
  if kind == "neg_inf":
    return float("-inf"), dtype
  if kind == "finfo_min":
    return torch.finfo(dtype).min, dtype
  if kind == "finfo_min_fp32":
    return torch.finfo(torch.float32).min, torch.float32
  if kind == "minus_1e4":
    return -1e4, dtype
  if kind == "minus_1e9":
    return -1e9, torch.float32
  raise ValueError(kind)


def padded_keys(nkv: int) -> int:
  return nkv // 3


def hf_mask(shape, dtype, seed, kind: str = "finfo_min"):
  """B = 2; sequence 1 is left-padded: its first ``Nkv // 3`` key columns carry the mask value for every row, and its first MASKED_ROWS query rows (padding
  tokens themselves) carry it on EVERY key; sequence 0 is unmasked.  bias ``[2, 1, Nq, Nkv]``.  Guarantees (asserted): exactly rows [0, 5) of batch 1 are
  wholly masked; with -inf they see no key, with a finite value every key alike."""
  B, hq, hkv, nq, nkv, d = shape
  assert B == 2
  q, k, v = plain(shape, dtype, seed)
  value, mdt = mask_value(kind, dtype)
  bias = torch.zeros((2, 1, nq, nkv), dtype=torch.float32)
  bias[1, :, :, :padded_keys(nkv)] = value
  bias[1, :, :MASKED_ROWS, :] = value
  return q, k, v, bias.to(mdt)


def key_padding_mask(shape, dtype, seed, kind: str = "finfo_min"):
  """``hf_mask`` as a KEY bias ``[2, 1, 1, Nkv]`` (no row axis: the kernels' key-bias builds): the first ``Nkv // 3`` keys of sequence 0 carry the mask value,
  and EVERY key of sequence 1 does (a sequence that is padding throughout): all its rows are wholly masked."""
  B, hq, hkv, nq, nkv, d = shape
  assert B == 2
  q, k, v = plain(shape, dtype, seed)
  value, mdt = mask_value(kind, dtype)
  bias = torch.zeros((2, 1, 1, nkv), dtype=torch.float32)
  bias[0, :, :, :padded_keys(nkv)] = value
  bias[1] = value
  rows = torch.zeros((2, nq), dtype=torch.bool)
  rows[1] = True
  return q, k, v, bias.to(mdt), rows


def wholly_masked_rows(shape):
  """``[B, Nq]`` bool: the rows ``hf_mask`` masks on every key."""
  B, _, _, nq, _, _ = shape
  m = torch.zeros((B, nq), dtype=torch.bool)
  m[1, :MASKED_ROWS] = True
  return m


def alibi(shape, dtype, seed, bias_dtype=torch.float32):
  """ALiBi: head h adds ``-2^(-8 (h + 1) / Hq) |i + (Nkv - Nq) - j|`` (query i sits at key position i + Nkv - Nq: tail aligned).  bias ``[1, Hq, Nq, Nkv]`` in
  ``bias_dtype`` (fp32, or q's dtype: distances up to 700 round to 8 / 11 bits, and the reference reads the ROUNDED bias).  Guarantees (asserted): the bias
  is 0 on the aligned diagonal, and its most negative entry is -slope_0 x the longest distance."""
  B, hq, hkv, nq, nkv, d = shape
  q, k, v = plain(shape, dtype, seed)
  slopes = torch.tensor([2.0 ** (-8.0 * (h + 1) / hq) for h in range(hq)], dtype=torch.float64)
  dist = (torch.arange(nq)[:, None] + (nkv - nq) - torch.arange(nkv)[None, :]).abs().double()
  bias = -(slopes[:, None, None] * dist[None])[None]
  return q, k, v, bias.to(bias_dtype)


# ----------------------------------------------------------------------------- the float64 reference
def causal_mask(nq: int, nkv: int, device=None):
  """``[Nq, Nkv]`` bool, True = visible: tail-aligned causal (query i sees keys j <= i + Nkv - Nq)."""
  return torch.arange(nkv, device=device)[None, :] <= (torch.arange(nq, device=device)[:, None] + (nkv - nq))


def scores(q, k, bias=None, causal: bool = False, scale: "float | None" = None, fp32_rows=None):
  """``scale q.k + bias`` in float64, ``[B, Hq, Nq, Nkv]``, -inf where the causal mask hides a key.  ``fp32_rows [B, Nq]`` (bool): in those rows the sum is
  formed as ``fp32(fp32(scale s) + bias)`` — what an fp32 implementation (SDPA's math path) computes, and the only thing any fp32 implementation CAN compute
  of a row whose every key carries a large finite mask value: the value absorbs most or all of s, where float64 would keep it."""
  B, hq, nq, d = q.shape
  hkv = k.size(1)
  scale = d ** -0.5 if scale is None else scale
  kk = k.double().repeat_interleave(hq // hkv, dim=1)
  s = torch.matmul(q.double(), kk.transpose(-1, -2)) * scale
  if bias is not None and bias.dtype == torch.bool:
    s = s.masked_fill(~bias, float("-inf"))  # SDPA's boolean mask: True = visible
  elif bias is not None:
    full = s + bias.double()
    if fp32_rows is not None and bool(fp32_rows.any()):
      rounded = (s.float() + bias.float()).double()
      full = torch.where(fp32_rows.to(s.device)[:, None, :, None], rounded, full)
    s = full
  if causal:
    s = s.masked_fill(~causal_mask(nq, k.size(2), s.device), float("-inf"))
  return s


def attend(q, k, v, bias=None, causal: bool = False, scale: "float | None" = None, fp32_rows=None):
  """Float64 softmax attention of q ``[B, Hq, Nq, D]`` over k / v ``[B, Hkv, Nkv, D]`` in the layout ``kvcache_ref.check`` takes:
  ``(o [B, Nq, Hq, D], lse [B, Hq, Nq], pmax [B, Hq, Nq], p2sum [B, Hq, Nq])``; rows without a visible key: O = 0, LSE = -inf, statistics 0."""
  s = scores(q, k, bias, causal, scale, fp32_rows)
  vv = v.double().repeat_interleave(q.size(1) // k.size(1), dim=1)
  m = s.amax(dim=-1, keepdim=True)
  live = torch.isfinite(m)
  e = torch.exp(s - torch.where(live, m, torch.zeros_like(m)))
  l = e.sum(dim=-1, keepdim=True)
  p = torch.where(live, e / torch.where(live, l, torch.ones_like(l)), torch.zeros_like(e))
  o = torch.matmul(p, vv)
  lse = torch.where(live, m + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, float("-inf")))[..., 0]
  return o.transpose(1, 2).contiguous(), lse, p.amax(dim=-1), p.pow(2).sum(dim=-1)


def attend_each_batch(q, k, v, bias=None, causal: bool = False):
  """``attend``, one batch entry at a time: the float64 copies of K and V of a short-query case (16 x 8 x 2000 x 1024) are 2 GB each when made at once."""
  pick = lambda t, b: None if t is None else t[b:b + 1] if t.size(0) > 1 else t
  parts = [attend(q[b:b + 1], k[b:b + 1], v[b:b + 1], pick(bias, b), causal) for b in range(q.size(0))]
  return tuple(torch.cat([p[i] for p in parts]) for i in range(4))


def fp32_ulp(x: float) -> float:
  return float(np.spacing(np.float32(abs(x))))


def absorbed_margin(value: float, ref, v, dtype=None):
  """What a row masked wholly by the finite value ``value`` may differ by from ``attend(..., fp32_rows=...)``, per row ``[B, Hq, Nq]`` (numpy): both sides put
  their scores on an fp32 grid at |value|, but not the same one — the reference adds in natural units (spacing ulp(value)), the kernels in log2 units
  (ulp(value log2 e) ln 2) or, the 16x16x32 build, in units of 1 / scale (ulp(value / scale) scale): each within a factor 2 of ulp(value).  A score moves by
  up to half a spacing on either side, so p_j by the relative d_j, |d_j| <= (1 + 2) ulp / 2, independent from key to key, and O by sum_j p_j d_j (v_j - O): five
  sigma of it = 5 x (3 ulp / 2) / sqrt 3 x sqrt(sum p^2) x rms v.  0 for a value below BIAS_FLOOR (both sides absorb s whole: every key alike) and for -inf."""
  if not np.isfinite(value) or value < BIAS_FLOOR:
    return np.zeros(ref[3].shape)
  vrms = float(v.detach().double().pow(2).mean().sqrt())
  return 5.0 * (1.5 * fp32_ulp(value)) / math.sqrt(3.0) * np.sqrt(ref[3].detach().cpu().numpy()) * vrms


# ----------------------------------------------------------------------------- the cases
HEAD_DIMS = (128, 320, 512, 1024)          # prefill runs the 16x16x32 kernel at all four (FFPA_M16_MIN_D = 128): one wave per head dim / two (1024: head dim split across waves)
SMALL_HEAD_DIMS = (40, 64)                 # prefill runs the 32x32x16 split-D kernel's ND = 1 builds (head dims <= 64); 40: the 64 build with d_valid < D
SEQ_SHAPES = ((64, 700), (33, 333), (129, 513))
BIAS_SEQ_SHAPES = ((129, 520),)            # the bias-carrying variants only: Nkv a multiple of 8, so the rows of a 16-bit bias start 16-byte aligned and are staged through LDS
SPLIT_SEQ_SHAPE = (129, 3100)              # 25 tiles of 128 keys: the shortest KV axis a prefill launch at head dims <= 64 cuts into 3 ranges (a range holds at least 8 tiles)
HEADS = ((2, 2), (4, 1))
DTYPES = (torch.bfloat16, torch.float16)

# variant name -> (family, knobs, whether the family carries a bias).  Families without a mask run plain and tail-aligned causal.
VARIANTS = {
  "outliers": ("outliers", {}, False),
  "sink": ("sink", {}, False),
  "peaked": ("peaked", {}, False),
  "large_logits": ("large_logits", {}, False),
  **{f"staircase_up_{s}": ("staircase_up", {"step": s}, False) for s in STAIR_STEPS},
  **{f"staircase_down_{s}": ("staircase_down", {"step": s}, False) for s in STAIR_STEPS},
  **{f"hf_mask_{kind}": ("hf_mask", {"kind": kind}, True) for kind in MASK_VALUES},
  "alibi_fp32": ("alibi", {"bias_dtype": torch.float32}, True),
  "alibi_16bit": ("alibi", {"bias_dtype": None}, True),
}
FAMILIES = {"plain": plain, "outliers": outliers, "sink": sink, "peaked": peaked, "staircase_up": staircase_up, "staircase_down": staircase_down,
            "large_logits": large_logits, "hf_mask": hf_mask, "alibi": alibi}
SHORT_QUERY_VARIANTS = ("sink", "peaked", "staircase_up_8.5", "large_logits")
# head dim -> (waves the head dim is split over, keys per tile) of the short-query build that serves it (csrc/ffpa_common.h ``splitd_block_keys``): all four
# tile shapes, twice over
SHORT_QUERY_TILES = {64: (2, 32), 128: (4, 64), 320: (2, 64), 512: (4, 64), 576: (2, 32), 1024: (4, 32)}
SHORT_QUERY_HEAD_DIMS = tuple(SHORT_QUERY_TILES)
SHORT_QUERY_NKV = 2000
SHORT_QUERY_HEADS = ((8, 2), (4, 4))       # (8, 2): the four heads of a KV group are packed into the rows of one tile (4 rows at Nq = 1, 28 at Nq = 7)
SHORT_QUERY_BATCH = {1: 16, 7: 4}          # Nq -> B: enough rows (64 ... 224) for ``assert_short_query_property`` to be a statement about the case
# (variant, D, Nq, Hq, dtype name) -> how far past its base ``77 + Nq + Hq`` the seed of a short-query case lies: the first seed at which
# ``assert_short_query_property`` holds (tests/test_model_values_ref.py walks them again).  Cases not listed hold at the base.
SHORT_QUERY_SEED_STEPS = {
  ("sink", 576, 1, 4, "bf16"): 6, ("sink", 576, 1, 4, "fp16"): 6,    # 64 rows: seeds 82 ... 87 give fewer than 3 sink rows
  ("sink", 1024, 1, 8, "bf16"): 1, ("sink", 1024, 1, 8, "fp16"): 1,  # 128 rows: seed 86 does
}
# (variant, D, Nq, Hq) -> a further seed step, both dtypes: at the seed above, the C ORACLE ALONE leaves the allowance in fp16 (1.02 at D = 576, 1.01 and — one
# seed on — 1.13 at D = 1024; 0.88 ... 0.93 at the seeds taken).  The top of the staircase is the last, half-filled tile of 32 keys: 16 entries of p = 1 / 16,
# whose rounding to fp16 the allowance bounds by its cap of 4e-4 — five sigma of it is 2.5e-4 on top of the flips, and these cases have 1.3e5 ... 2.3e5 elements.
SHORT_QUERY_SEED_MOVES = {("staircase_up_8.5", 576, 7, 8): 1, ("staircase_up_8.5", 1024, 7, 8): 2}


def dense_cases(variant: str, D: int):
  """The dense cases of a variant at head dim D (HEAD_DIMS or SMALL_HEAD_DIMS): every (Nq, Nkv) x heads x dtype (x plain / causal where the family has no
  mask) of the grid; the bias-carrying variants run BIAS_SEQ_SHAPES as well."""
  family, knobs, has_bias = VARIANTS[variant]
  out = []
  for nq, nkv in SEQ_SHAPES + (BIAS_SEQ_SHAPES if has_bias else ()):
    for hq, hkv in HEADS:
      for dtype in DTYPES:
        for causal in ((False,) if has_bias else (False, True)):
          B = 2 if family == "hf_mask" else 1
          out.append({"variant": variant, "family": family, "knobs": dict(knobs), "shape": (B, hq, hkv, nq, nkv, D), "dtype": dtype, "causal": causal,
                      "seed": 1000 + 7 * nq + hq + (1 if causal else 0)})
  return out


def split_cases(variant: str, D: int):
  """The cases of a bias-free variant at head dim D (SMALL_HEAD_DIMS) on SPLIT_SEQ_SHAPE: heads x dtype x plain / causal, for an under-filled prefill launch
  with ``num_splits=3``."""
  family, knobs, has_bias = VARIANTS[variant]
  assert not has_bias
  nq, nkv = SPLIT_SEQ_SHAPE
  return [{"variant": variant, "family": family, "knobs": dict(knobs), "shape": (1, hq, hkv, nq, nkv, D), "dtype": dtype, "causal": causal,
           "seed": 1000 + 7 * nq + hq + (1 if causal else 0)} for hq, hkv in HEADS for dtype in DTYPES for causal in (False, True)]


SPLIT_VARIANTS = ("sink", "staircase_up_8.5", "large_logits")


def short_query_cases(variant: str, D: int):
  """The short-query cases of a variant at head dim D (SHORT_QUERY_HEAD_DIMS): Nq in {1, 7} against 2000 keys x SHORT_QUERY_HEADS x dtype, B rows enough
  (SHORT_QUERY_BATCH) and the seed that makes ``assert_short_query_property`` hold (SHORT_QUERY_SEED_STEPS; ``first_seed``: before SHORT_QUERY_SEED_MOVES).  ``causal`` is False; the launches that run
  the Nq = 7 cases tail-aligned causal too do so on the same tensors (key 0 and the staircase's lower tiles stay visible to every row)."""
  family, knobs, has_bias = VARIANTS[variant]
  assert variant in SHORT_QUERY_VARIANTS and D in SHORT_QUERY_TILES and not has_bias
  out = []
  for nq in (1, 7):
    for hq, hkv in SHORT_QUERY_HEADS:
      for dtype in DTYPES:
        step = SHORT_QUERY_SEED_STEPS.get((variant, D, nq, hq, "bf16" if dtype == torch.bfloat16 else "fp16"), 0)
        move = SHORT_QUERY_SEED_MOVES.get((variant, D, nq, hq), 0)
        out.append({"variant": variant, "family": family, "knobs": dict(knobs), "shape": (SHORT_QUERY_BATCH[nq], hq, hkv, nq, SHORT_QUERY_NKV, D), "dtype": dtype,
                    "causal": False, "seed": 77 + nq + hq + step + move, "first_seed": 77 + nq + hq + step, "block_keys": SHORT_QUERY_TILES[D][1]})
  return out


def short_query_property(case: dict, q, k, bias=None) -> dict:
  """The figures ``assert_short_query_property`` judges, from the float64 scores of every row the case computes (one batch entry at a time: K of the
  largest case is 0.5 GB in float64)."""
  p0, pm, top, diffs = [], [], 0.0, []
  bc = case["block_keys"]
  for b in range(q.size(0)):
    s = scores(q[b:b + 1], k[b:b + 1], None if bias is None else bias[b:b + 1] if bias.size(0) > 1 else bias, case["causal"])
    p = torch.softmax(s, dim=-1)
    p0.append(p[..., 0].flatten())
    pm.append(p.amax(dim=-1).flatten())
    top = max(top, float(s[torch.isfinite(s)].abs().max()))
    if case["family"].startswith("staircase"):
      s2 = (s * LOG2E).flatten(0, 2)
      tmax = torch.stack([s2[:, i * bc:(i + 1) * bc].amax(dim=-1) for i in range(-(-s2.size(-1) // bc))], dim=-1)
      diffs.append(((tmax[:, 1:] - tmax[:, :-1]) * (1 if case["family"] == "staircase_up" else -1)).flatten())
  p0, pm = torch.cat(p0), torch.cat(pm)
  fig = {"rows": int(pm.numel()), "mean pmax": float(pm.mean()), "top |s|": top, "sink rows": int((p0 >= 0.5).sum()), "rows blind to key 0": int((p0 <= 1e-6).sum())}
  if diffs:
    d = torch.cat(diffs)
    fig.update({"tile steps": int(d.numel()), "worst |step - want|": float((d - case["knobs"]["step"]).abs().max()),
                "steps on their side of the threshold": bool(((d > RESCALE_THRESHOLD) == (case["knobs"]["step"] > RESCALE_THRESHOLD)).all())})
  return fig


def short_query_property_holds(case: dict, fig: dict) -> bool:
  family = case["family"]
  if family == "sink":
    return fig["sink rows"] >= 3 and 4 * fig["rows blind to key 0"] >= fig["rows"]
  if family == "peaked":
    return fig["mean pmax"] >= 0.5
  if family == "large_logits":
    return 55.0 <= fig["top |s|"] <= 140.0
  if family.startswith("staircase"):
    return fig["tile steps"] >= fig["rows"] and fig["worst |step - want|"] <= 0.25 and fig["steps on their side of the threshold"]
  raise ValueError(family)


def assert_short_query_property(case: dict, q, k, bias=None) -> dict:
  """What a short-query case is there for, asserted on the float64 scores of the rows it computes — a few dozen rows do not have a family's property by
  the law of large numbers, as the ``SEQ_SHAPES`` cases do; the thresholds are those of tests/test_model_values_ref.py:

  * sink: at least 3 rows give key 0 (the first KV range of a split launch) p >= 0.5, and at least a quarter of the rows p <= 1e-6;
  * peaked: mean row pmax >= 0.5;
  * large_logits: the largest |score| lies in [55, 140];
  * staircases: every row's maximum steps by the knob, to within 0.25 log2 units, between neighbouring KV tiles of the launch's ``block_keys``
    (``case["block_keys"]``: what the tensors must have been built for), on its side of the rescale threshold.

  -> the figures it read (``short_query_property``)."""
  fig = short_query_property(case, q, k, bias)
  assert short_query_property_holds(case, fig), (case["variant"], case["shape"], case["dtype"], case["seed"], fig)
  return fig


def build(case: dict, block_keys: int = 64):
  """The tensors of a case (CPU) -> ``(q, k, v, bias | None, fp32_rows | None, mask value | None)``.  ``block_keys``: the launch's KV tile (the staircases)."""
  knobs = dict(case["knobs"])
  if case["family"].startswith("staircase"):
    knobs["block_keys"] = block_keys
  if case["family"] == "alibi" and knobs.get("bias_dtype") is None:
    knobs["bias_dtype"] = case["dtype"]
  out = FAMILIES[case["family"]](case["shape"], case["dtype"], case["seed"], **knobs)
  q, k, v = out[:3]
  bias = out[3] if len(out) > 3 else None
  rows = value = None
  if case["family"] == "hf_mask":
    value = float(mask_value(knobs["kind"], case["dtype"])[0])
    if np.isfinite(value) and abs(value) >= 65504.0:  # a large finite value: its rows are compared on the fp32 grid (``scores``)
      rows = wholly_masked_rows(case["shape"])
  return q, k, v, bias, rows, value


# ----------------------------------------------------------------------------- the comparison
def _row_mask(case, rows=None):
  """``[B, Nq, Hq, 1]`` bool (numpy): the wholly masked rows of a masked case (``rows [B, Nq]``; default: ``hf_mask``'s), in the layout of ``kvcache_ref.check``'s output."""
  B, hq, _, nq, _, _ = case["shape"]
  rows = wholly_masked_rows(case["shape"]) if rows is None else rows
  return np.broadcast_to(rows.cpu().numpy()[:, :, None, None], (B, nq, hq, 1))


def check_case(out, lse, ref, case, *, v, value=None, name: str = "", rows=None, judge_absorbed_rows: bool = True) -> float:
  """A forward's ``out [B, Hq, Nq, D]`` (16 bits) and ``lse [B, Hq, Nq] | None`` against ``ref = attend(...)`` through ``kvcache_ref.check``, every element,
  with what the wholly masked rows of an ``hf_mask`` case (mask value ``value``) are owed:

  * -inf: the forward's contract is SDPA's — the row is NaN (asserted here), its LSE is not a finite number; ``check`` then sees the 0 / -inf of ``attend``;
  * a finite value below BIAS_FLOOR: the output is compared like any other (the plain mean of V), the LSE is not — ``value`` times log2 e is not an fp32
    number, so the kernels carry one saturated score instead: asserted finite and below -2^60, then taken from the reference;
  * a finite value above it: ``absorbed_margin`` on top of the allowance — or, with ``judge_absorbed_rows=False``, asserted finite and not compared (the
    caller compares them in a test of their own: tests/test_fwd_model_values_gpu.py ``test_rows_masked_wholly_by_a_large_finite_value``)."""
  import kvcache_ref as kr

  out = out.detach().transpose(1, 2).clone()
  lse = None if lse is None else lse.detach().double().clone()
  extra = None
  if value is not None:
    rows = _row_mask(case, rows)
    rows_t = torch.from_numpy(np.ascontiguousarray(rows[..., 0])).to(out.device)  # [B, Nq, Hq]
    if value == float("-inf"):
      assert bool(torch.isnan(out[rows_t]).all()), f"{name}: a row whose every key is -inf is not NaN"
      out[rows_t] = 0
      if lse is not None:
        assert not bool(torch.isfinite(lse.transpose(1, 2)[rows_t]).any()), f"{name}: finite LSE in a row whose every key is -inf"
        lse.transpose(1, 2)[rows_t] = float("-inf")
    elif value < BIAS_FLOOR:
      if lse is not None:
        got = lse.transpose(1, 2)[rows_t]
        assert bool(torch.isfinite(got).all()) and bool((got < -2.0 ** 60).all()), f"{name}: LSE of a row masked wholly by {value:g}: {got.flatten()[:4]}"
        lse.transpose(1, 2)[rows_t] = ref[1].to(lse.device).transpose(1, 2)[rows_t]
    elif not judge_absorbed_rows:
      assert bool(torch.isfinite(out[rows_t]).all()), f"{name}: a row masked wholly by {value:g} is not finite"
      out[rows_t] = ref[0].to(out.device)[rows_t].to(out.dtype)
      if lse is not None:
        assert bool(torch.isfinite(lse.transpose(1, 2)[rows_t]).all()), f"{name}: LSE of a row masked wholly by {value:g}"
        lse.transpose(1, 2)[rows_t] = ref[1].to(lse.device).transpose(1, 2)[rows_t]
    else:
      margin = absorbed_margin(value, ref, v)                       # [B, Hq, Nq]
      extra = np.where(rows, np.transpose(margin, (0, 2, 1))[..., None], 0.0)
  return kr.check(out, lse, ref, v=v, dtype=case["dtype"], name=name, extra=extra)


def masked_rows_need(out, ref, case, *, v, value) -> float:
  """Worst (error - allowance) / ``absorbed_margin`` over the wholly masked rows: how much of the margin a result needs (<= 0: none of it)."""
  import kvcache_ref as kr

  o_ref, _, pmax, p2sum = (t.detach().cpu().numpy() for t in ref)
  got = out.detach().transpose(1, 2).double().cpu().numpy()
  stat = lambda t: np.transpose(t, (0, 2, 1))
  half_ulp, flip = kr.allowance(o_ref, stat(pmax), stat(p2sum), v, case["dtype"], noise=True)
  margin = stat(absorbed_margin(value, ref, v))[..., None]
  rows = np.broadcast_to(_row_mask(case), got.shape)
  need = (np.abs(got - o_ref) - half_ulp - flip) / np.maximum(margin, 1e-300)
  return float(need[rows].max())
