"""What tests/test_kvcache_mla_contract_gpu.py draws on the CPU, so that it can be checked without a GPU (tests/test_kvcache_mla_contract.py): the row-chunk
shapes of the latent-cache call with the chunk counts the plan must report, and the model-like cases (tests/model_values.py families laid out as latent rows)
with the property every family's docstring promises, asserted on a float64 reference.  Plain torch + numpy."""

from __future__ import annotations

import math

import torch

import model_values as mv

D, DV = 576, 512
BLOCK_ROWS, BLOCK_KEYS = 64, 32  # the latent kernel's tile: 64 rows x 32 keys
MODEL_SCALE = D ** -0.5          # the scale the families of model_values are built for (the staircases fold it into q)

# ----------------------------------------------------------------------------- row chunks
# (Hq, Hkv, Sq): what the rows of a (sequence, KV head) are cut into
ROW_SHAPES = (
  (32, 1, 3),    # 96 rows: two chunks, the last 32 rows; the boundary at row 64 = head 21, token 1
  (24, 1, 3),    # 72: the last chunk 8 rows
  (40, 1, 5),    # 200: four chunks, the last 8 rows
  (48, 2, 3),    # 72 per KV head: two KV heads, each with a partial chunk
  (16, 1, 70),   # 1120: 18 chunks, each holding part of one or two heads' tokens; the last 32 rows
  (1, 1, 70),    # unpacked: two row tiles
  (4, 4, 130),   # unpacked: three row tiles per head
)


def row_lens(sq: int) -> list:
  """The key lengths of the row-chunk cases: the empty sequence, one key, odd and even tile counts, and Sq - 1, Sq, Sq + 1 (under causal Sq - 1 leaves the first
  token without a key)."""
  return sorted({0, 1, 33, 64, 97, 300, max(sq - 1, 0), sq, sq + 1})


def packed(hq: int, hkv: int) -> bool:
  return hq // hkv > 1


def row_tiles(hq: int, hkv: int, sq: int) -> int:
  """ceil(group x Sq / 64) when the group's heads are packed into rows, ceil(Sq / 64) when rows are tokens."""
  group = hq // hkv
  return math.ceil((group * sq if group > 1 else sq) / BLOCK_ROWS)


def live_rows_of_last_chunk(hq: int, hkv: int, sq: int) -> int:
  group = hq // hkv
  rows = group * sq if group > 1 else sq
  return rows - (row_tiles(hq, hkv, sq) - 1) * BLOCK_ROWS


# ----------------------------------------------------------------------------- model-like values
MODEL_VARIANTS = ("outliers", "sink", "large_logits") + tuple(f"staircase_{d}_{s}" for d in ("up", "down") for s in mv.STAIR_STEPS)
MODEL_HEADS = ((16, 1), (32, 1))
MODEL_SQ = (1, 3)          # 3: causal
MODEL_LENS = (389, 513)    # 13 and 17 tiles of 32 keys, the last one partial (5 keys / 1 key)
MODEL_BATCH = 3            # 48 ... 288 rows per case: enough for the families' row fractions


def model_cases(variant: str, dtype) -> list:
  family, knobs, _ = mv.VARIANTS[variant]
  out = []
  for hq, hkv in MODEL_HEADS:
    for sq in MODEL_SQ:
      for L in MODEL_LENS:
        out.append({"variant": variant, "family": family, "knobs": dict(knobs), "heads": (hq, hkv), "sq": sq, "L": L, "causal": sq > 1, "dtype": dtype,
                    "shape": (MODEL_BATCH, hq, hkv, sq, L, D), "seed": 3000 + 13 * hq + 5 * sq + L})
  return out


def build_model_case(case: dict):
  """-> ``(q [B, Hq, Sq, D], latent rows k [B, Hkv, L, D])`` (CPU) of the family: its ``k`` are the latent rows — keys in all D columns, values in the first DV —
  and its ``v`` is not used.  The staircases step from one 32-key tile to the next."""
  knobs = dict(case["knobs"])
  if case["family"].startswith("staircase"):
    knobs["block_keys"] = BLOCK_KEYS
  q, k, _ = mv.FAMILIES[case["family"]](case["shape"], case["dtype"], case["seed"], **knobs)
  return q, k


def model_reference(case: dict, q, k):
  """float64 attention of the case on the CPU, in ``kvcache_ref.check``'s layout (value columns ``[:DV]``)."""
  o, lse, pmax, p2sum = mv.attend(q, k, k, None, case["causal"], MODEL_SCALE)
  return o[..., :DV].contiguous(), lse, pmax, p2sum


def assert_family_property(case: dict, q, k, ref) -> None:
  """The property the family's docstring promises (the thresholds of tests/test_model_values_ref.py), on the case's float64 reference ``ref = (o, lse [B, Hq, Sq],
  pmax [B, Hq, Sq], p2sum)`` and its float64 scores: a case that cannot show it is not a test."""
  family, name = case["family"], f"{case['variant']} {case['shape']} causal={case['causal']}"
  s = mv.scores(q, k, None, case["causal"], MODEL_SCALE)  # [B, Hq, Sq, L], -inf where causal hides a key (key 0 is visible to every row: L >= Sq)
  pmax, lse = ref[2].detach().cpu(), ref[1].detach().cpu()
  if family in ("outliers", "sink"):
    assert float(pmax.mean()) >= 0.4, (name, float(pmax.mean()))
  if family == "outliers":
    # the key outlier channel inside the value columns is a value outlier: the largest |value| sits on it
    vals = k[..., :DV].float().abs()
    assert float(vals[..., mv.OUTLIER_CHANNELS[0]].max()) == float(vals.max()) and float(vals.max()) >= 30.0, (name, float(vals.max()))
  if family == "sink":
    p0 = torch.softmax(s, dim=-1)[..., 0]
    assert float((p0 >= 0.5).double().mean()) >= 0.04, (name, float((p0 >= 0.5).double().mean()))
    assert float((p0 <= 1e-6).double().mean()) >= 0.25, (name, float((p0 <= 1e-6).double().mean()))
    assert float(k[:, :, 0].float().abs().sum()) == 2 * mv.SINK_VALUE * k.size(0) * k.size(1), name
  if family == "large_logits":
    top = float(s[torch.isfinite(s)].abs().max())
    assert 55.0 <= top <= 140.0, (name, top)
    assert float(lse.abs().max()) >= 40.0, (name, float(lse.abs().max()))
  if family.startswith("staircase"):
    step, up = case["knobs"]["step"], family == "staircase_up"
    s2 = s * mv.LOG2E
    tiles = -(-case["L"] // BLOCK_KEYS)
    tmax = torch.stack([s2[..., t * BLOCK_KEYS:(t + 1) * BLOCK_KEYS].amax(dim=-1) for t in range(tiles)], dim=-1)
    diff = (tmax[..., 1:] - tmax[..., :-1]) * (1 if up else -1)
    both = torch.isfinite(tmax[..., 1:]) & torch.isfinite(tmax[..., :-1])  # (causal: the last tile of L = 513 is one key, hidden from the first two tokens)
    assert int(both.sum()) >= both.numel() - case["shape"][0] * case["shape"][1] * (case["sq"] - 1), name
    assert float((diff[both] - step).abs().max()) <= 0.25, (name, float((diff[both] - step).abs().max()))
    assert bool(((diff[both] > mv.RESCALE_THRESHOLD) == (step > mv.RESCALE_THRESHOLD)).all()), name
