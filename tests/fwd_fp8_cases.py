"""Inputs and references of the FP8 forward's tests, stated once: the float64 reference and the derived allowance (moved here unchanged from
tests/test_fwd_fp8_gpu.py), and ONE builder of exact integer-code cases that the GPU tests run and tests/test_fwd_fp8_cases.py checks without a GPU.

An exact case (``exact_case``): q codes hold one 1 per row, on column ``(37 row + 11 head + 5 batch) % D``; k codes are random in {-1, 0} with +1 on the row's
own column AT THE ROW'S LAST VISIBLE KEY (its carrier: the diagonal ``min(row + Nkv - Nq, Nkv - 1)`` under causal, ``Nkv - 1`` otherwise); v codes are
integers in [-4, 4]; ``q_scale`` in {2, 4} per (batch, head, row tile), ``k_scale`` in {1, 1/2} per (batch, KV head, key tile), ``v_scale`` in {1/2, 1, 2} per
channel.  Raw scores lie in [-1, 1], scaled scores are integers in [-4, 4]: the spread is at most 8 = FP8_P_SHIFT, every p 2^shift is a power of two that e4m3
holds, every sum stays below 2^24 — each step of the kernel is exact in fp32 and its output is the float64 quotient rounded once to fp32 and once to the
output dtype.  The carrier on the limit is what makes a limit that is off by one visible: without it the row loses its largest score."""

import functools
from typing import NamedTuple

import numpy as np
import torch

import kvcache_ref as kr
import model_values as mv
from ffpa_attn_amd import pack_attn_fp8_k, pack_attn_fp8_q, pack_attn_fp8_vt, quantize_attn_fp8
from ffpa_attn_amd.interface import FP8_BLOCK_KEYS as K, FP8_BLOCK_ROWS as R, FP8_P_SHIFT

E4M3 = torch.float8_e4m3fn
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def attend2(qh, kh, vh, causal):
  """Float64 attention in the exp2 domain: ``qh [B, Hq, Nq, D]``, ``kh`` / ``vh [B, Hkv, Nkv, D]`` -> ``(o, p / l, row has a key)``; tail-aligned causal."""
  g = qh.size(1) // kh.size(1)
  s = qh.double() @ kh.double().repeat_interleave(g, 1).transpose(-1, -2)
  if causal:
    s = s.masked_fill(~mv.causal_mask(qh.size(2), kh.size(2)), float("-inf"))
  m = s.amax(-1, keepdim=True)
  live = torch.isfinite(m)
  p = torch.exp2(s - torch.where(live, m, torch.zeros_like(m)))
  l = torch.where(live, p.sum(-1, keepdim=True), torch.ones_like(m))
  p = torch.where(live, p, torch.zeros_like(p))
  # (numerator first, ONE division: on integer operands the float64 numerator and l are exact, and the quotient is the exact one rounded once)
  return (p @ vh.double().repeat_interleave(g, 1)) / l, p / l, live, s


def fp8_allowance(p, vh, group):
  """``sum_j max(2^-4 p_j, 2^-(10 + shift)) |v_jd|``, p = P / l: P's rounding to three mantissa bits, and half a subnormal step of p 2^shift below 2^-6."""
  per_key = torch.maximum(p * 2.0 ** -4, p.new_full((), 2.0 ** -(10 + FP8_P_SHIFT)))
  return per_key @ vh.double().abs().repeat_interleave(group, 1)


def check_against_dequantised(out, q, k, v, scale, causal, smooth_k, name):
  """-> ``(worst error / allowance, the allowance per element, the reference)`` of ``out`` against float64 attention over the helper's dequantised operands;
  every element judged."""
  h = quantize_attn_fp8(q, k, v, scale, smooth_k)
  qh = h.q_codes.double() * h.q_scale.repeat_interleave(R, -1)[..., : q.size(2), None]
  kh = h.k_codes.double() * h.k_scale.repeat_interleave(K, -1)[..., : k.size(2), None]
  vh = h.v_codes.double() * h.v_scale[:, :, None, :]
  want, p, live, _ = attend2(qh, kh, vh, causal)
  half_ulp, flip = kr.allowance(want.numpy(), p.amax(-1).numpy(), p.pow(2).sum(-1).numpy(), vh, q.dtype, noise=False)
  bound = half_ulp + flip + fp8_allowance(p, vh, q.size(1) // k.size(1)).numpy()
  got = out.double().cpu().numpy()
  assert np.isfinite(got).all() and (got[~live.expand_as(want).numpy()] == 0).all(), name
  ratio = float((np.abs(got - want.numpy()) / bound).max())
  print(f"{name}: worst error / allowance {ratio:.3f}")
  return ratio, bound, want


# ----------------------------------------------------------------------------- the exact cases
class ExactCase(NamedTuple):
  """Integer codes (float32, ``[B, H, N, D]``), the power-of-two scales, each row's limit (its last visible key; negative: the row sees no key), each
  (batch, head, row)'s carrier key (-1: none) and the float64 reference with the rows that see a key."""

  name: str
  causal: bool
  qc: torch.Tensor
  kc: torch.Tensor
  vc: torch.Tensor
  q_scale: torch.Tensor
  k_scale: torch.Tensor
  v_scale: torch.Tensor
  limits: torch.Tensor
  carrier: torch.Tensor
  want: torch.Tensor
  live: torch.Tensor


def row_limits(nq: int, nkv: int, causal: bool) -> torch.Tensor:
  """The last key row i sees: ``i + Nkv - Nq`` under the tail-aligned causal mask (never past ``Nkv - 1``; negative: no key), else ``Nkv - 1``."""
  return torch.arange(nq) + (nkv - nq) if causal else torch.full((nq,), nkv - 1)


def _varied(draw, shape):
  """A draw of two values over ``shape`` that differs along EVERY axis longer than one: a kernel that drops an index of the scale reads another value."""
  for _ in range(64):
    x = draw(shape)
    if all(x.size(a) == 1 or bool((x.narrow(a, 0, x.size(a) - 1) != x.narrow(a, 1, x.size(a) - 1)).any()) for a in range(x.dim())):
      return x
  raise AssertionError(f"no varied draw over {shape}")


def dequantised(c: ExactCase):
  nq, nkv = c.qc.size(2), c.kc.size(2)
  return (c.qc * c.q_scale.repeat_interleave(R, -1)[..., :nq, None], c.kc * c.k_scale.repeat_interleave(K, -1)[..., :nkv, None], c.vc * c.v_scale[:, :, None, :])


def attend_limits(c: ExactCase, limits: torch.Tensor):
  """The float64 reference of a case with row i seeing the keys ``j <= limits[i]``: ``(o, row has a key, scores)``.  The weights are ``2^(s + shift / 2)``
  with no maximum taken out: on integer scores in [-4, 4] they, the numerator and the row sum are exact integers, and the one division rounds the same exact
  quotient ``attend2`` rounds (tests/test_fwd_fp8_cases.py asserts the two equal bit for bit on the true limits)."""
  qh, kh, vh = dequantised(c)
  g = qh.size(1) // kh.size(1)
  s = qh.double() @ kh.double().repeat_interleave(g, 1).transpose(-1, -2)
  seen = torch.arange(kh.size(2))[None, :] <= limits[:, None]
  w = torch.where(seen, torch.exp2(s + FP8_P_SHIFT / 2), torch.zeros_like(s))
  l = w.sum(-1, keepdim=True)
  live = l > 0
  return (w @ vh.double().repeat_interleave(g, 1)) / torch.where(live, l, torch.ones_like(l)), live, s.masked_fill(~seen, float("-inf"))


@functools.lru_cache(maxsize=None)
def exact_case(B: int, hq: int, hkv: int, nq: int, nkv: int, D: int, causal: bool, seed: int = 0) -> ExactCase:
  """The case of the module docstring; its conditions (``assert_exact_conditions``) are asserted before it is handed out.  Cached: the GPU tests of both
  output dtypes and the CPU test share one build, and nobody writes to it."""
  group = hq // hkv
  g = torch.Generator().manual_seed(1000 * D + 7 * nq + 3 * nkv + 2 * group + int(causal) + 100003 * seed)
  rows, heads, batches = torch.arange(nq), torch.arange(hq), torch.arange(B)
  col = (rows[None, None] * 37 + heads[None, :, None] * 11 + batches[:, None, None] * 5) % D  # [B, hq, nq]: the heads of one GQA group differ by 11
  qc = torch.zeros(B, hq, nq, D)
  qc.scatter_(-1, col[..., None], 1.0)
  kc = -torch.randint(0, 2, (B, hkv, nkv, D), generator=g).float()
  limits = row_limits(nq, nkv, causal)
  carrier = torch.where(limits >= 0, limits, torch.full_like(limits, -1))[None, None].expand(B, hq, nq).contiguous()
  for b in range(B):
    for h in range(hq):
      has = limits >= 0
      kc[b, h // group, limits[has], col[b, h, has]] = 1.0
  vc = torch.randint(-4, 5, (B, hkv, nkv, D), generator=g).float()
  tiles = lambda n, blk: -(-n // blk)
  q_scale = _varied(lambda s: 2.0 ** torch.randint(1, 3, s, generator=g).float(), (B, hq, tiles(nq, R)))
  k_scale = _varied(lambda s: 2.0 ** -torch.randint(0, 2, s, generator=g).float(), (B, hkv, tiles(nkv, K)))
  v_scale = 2.0 ** torch.randint(-1, 2, (B, hkv, D), generator=g).float()
  c = ExactCase(f"B{B} Hq{hq} Hkv{hkv} Nq{nq} Nkv{nkv} D{D} causal={causal}", causal, qc, kc, vc, q_scale, k_scale, v_scale, limits, carrier, None, None)
  want, live, s = attend_limits(c, limits)
  c = c._replace(want=want, live=live)
  assert_exact_conditions(c, s)
  return c


def assert_exact_conditions(c: ExactCase, s: torch.Tensor) -> None:
  """Conditions 1 and 2: integer scores, a spread of at most FP8_P_SHIFT in every row, sums below 2^24 units; scales that vary wherever there is more than one
  row tile, key tile, head or batch."""
  fin = torch.isfinite(s)
  assert bool((s[fin] == s[fin].round()).all()) and float(s[fin].abs().max()) <= FP8_P_SHIFT / 2, c.name  # (attend_limits' weights count on [-4, 4])
  if bool(c.live.any()):
    spread = (s.amax(-1) - torch.where(fin, s, s.new_full((), float("inf"))).amin(-1))[c.live[..., 0]].max()
    assert spread <= FP8_P_SHIFT, (c.name, float(spread))
  assert c.kc.size(2) * 4 * 2 ** FP8_P_SHIFT < 2 ** 24, c.name
  assert float(c.qc.abs().max()) <= 1 and float(c.kc.abs().max()) <= 1 and float(c.vc.abs().max()) <= 4
  for t, values in ((c.q_scale, {2.0, 4.0}), (c.k_scale, {1.0, 0.5})):
    seen = set(t.unique().tolist())
    assert seen <= values and (t.numel() == 1 or seen == values), (c.name, t)


def expected(c: ExactCase, dtype: torch.dtype) -> torch.Tensor:
  """What the kernel must store, bit for bit: the float64 quotient rounded to fp32 (the kernel's one IEEE division), then to the output dtype."""
  return c.want.float().to(dtype)


def mutation_blind_rows(c: ExactCase, dtype: torch.dtype) -> dict:
  """Condition 3.  For the limits moved by +1 and by -1 (clamped to ``Nkv - 1``; below 0: no key) -> the number of (batch, head, row) whose set of visible
  keys changes while the mutated reference, rounded to ``dtype``, equals the true one in EVERY channel.  A sharp case answers 0 and 0."""
  nkv = c.kc.size(2)
  true = expected(c, dtype)
  blind = {}
  for step in (+1, -1):
    moved = (c.limits + step).clamp(max=nkv - 1)
    changed = moved.clamp(min=-1) != c.limits.clamp(min=-1)
    o, _, _ = attend_limits(c, moved)
    same = (o.float().to(dtype) == true).all(-1)  # [B, hq, nq]
    blind[step] = int((same & changed[None, None]).sum())
    blind[f"rows {step:+d}"] = int(changed.sum())
  return blind


def scratch(c: ExactCase, device="cpu"):
  """The six tensors ``ffpa_attn_fp8_codes`` takes, packed by the public helpers."""
  return tuple(t.to(device) for t in (pack_attn_fp8_q(c.qc.to(E4M3)), c.q_scale, pack_attn_fp8_k(c.kc.to(E4M3)), c.k_scale, pack_attn_fp8_vt(c.vc.to(E4M3)), c.v_scale))


# ----------------------------------------------------------------------------- the cases the GPU tests run (tests/test_fwd_fp8_edges_gpu.py), by group
HEAD_DIMS = (256, 320, 384, 448, 512)
EVERY_BUILD_SHAPES = {"tile+tail": (R + 5, 2 * K + 3), "Nq > Nkv": (2 * R + 3, R - 3)}


def every_build_cases():
  """B1: ``(id, exact_case arguments)`` over every head dim, causal and not, group 1 and 4, two shapes; B = 2, Hkv = 2."""
  return [(f"D{D}-{'causal' if causal else 'full'}-g{group}-{shape}", (2, 2 * group, 2, *EVERY_BUILD_SHAPES[shape], D, causal))
          for D in HEAD_DIMS for causal in (False, True) for group in (1, 4) for shape in EVERY_BUILD_SHAPES]


SEAM_DIMS = (256, 448)
SEAM_NQ = (1, 63, 64, 65, 128)
SEAM_NKV = (1, 127, 128, 129, 256, 257)
# (192, 128): the first row tile sees nothing and the second starts on key 0; (130, 64): a third row tile of two rows; (64, 192): row0 + off = 128 exactly —
# key tile 0 is wholly visible to every row and needs no element test, key tile 1 holds the diagonal
SEAM_EXTRA = ((192, 128), (130, 64), (64, 192))
SEAM_FULL = tuple((nq, nkv) for nq in (1, 64) for nkv in (1, 128, 129))


def seam_groups():
  """B2: ``{group id: [exact_case arguments]}`` — per head dim one group per Nq under causal (its six Nkv), one of the three extra causal shapes, one of the
  non-causal shapes; B = 1, Hq = Hkv = 2."""
  groups = {}
  for D in SEAM_DIMS:
    for nq in SEAM_NQ:
      groups[f"D{D}-causal-Nq{nq}"] = [(1, 2, 2, nq, nkv, D, True) for nkv in SEAM_NKV]
    groups[f"D{D}-causal-extra"] = [(1, 2, 2, nq, nkv, D, True) for nq, nkv in SEAM_EXTRA]
    groups[f"D{D}-full"] = [(1, 2, 2, nq, nkv, D, False) for nq, nkv in SEAM_FULL]
  return groups


O_STRIDE_CASE = (2, 4, 2, R + 5, 2 * K + 3, 320, True)  # B6
# B7: K8 and V8T of B x ceil(Nkv / 128) tiles of 128 x 512 bytes each: 264 x 125 x 65536 = 2 162 688 000 > 2^31 bytes per tensor; only the LAST batch holds a case
WIDE_B, WIDE_CASE = 264, (1, 1, 1, 1, 16000, 512, False)


def all_gpu_cases():
  """Every distinct ``exact_case`` argument tuple a GPU test runs."""
  args = [a for _, a in every_build_cases()] + [a for group in seam_groups().values() for a in group] + [O_STRIDE_CASE, WIDE_CASE]
  return sorted(set(args), key=args.index)
